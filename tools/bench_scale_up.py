"""Latency of the scale-up simulation (ksg_scale_up) against the route a caller had before it.

Shape: a cfg3-shaped synthetic cluster (--nodes nodes, 4,096 queue pods; every 5th
queue pod is also bound to a node as a DaemonSet-owned pod, so templates carry a base
load).  Templates in {1, 64, 256}, spread over the nodes; pod lists of 256 and 4,096
queue pods, largest cpu request first (the autoscaler's order).
  device route: ksg_scale_up(pods, templates, max_nodes = 1024) -- every template's
                packing in one call, 32 bytes per template back.  The first call after
                the load is timed apart: it compiles the queue's programs.
  host route:   the route a caller had before: a second context loaded with clones of the
                template (each with the base pods), then per listed pod
                ksg_cycle(commit = 0), ksg_filter_codes and ksg_reserve on the lowest
                passed clone.  Timed per template on --host-templates templates (one for
                the long list), the load of the clone context timed apart and not counted.
                The clone count is the node count the device plan opens plus one (at most
                1,024), which favours the host route; the device plan it is compared with
                (outside the timed part) is taken at that max_nodes.  Its per-template
                median times the template count is recorded as an extrapolation and named
                as one.
Warm-up calls, then --calls timed calls, a host clock around the C calls (each ends in a
device synchronise) with Python's collector off; median and p10-p90.

usage: python tools/bench_scale_up.py [--calls 20] [--warmup 3] [--nodes 1024]
                                      [--out profiles/scale_up_latency.json]"""
import argparse
import copy
import ctypes
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))

PASSED, NOT_EVALUATED = 0xFFFFFFFF, 0xFFFFFFFE
TEMPLATES = (1, 64, 256)
LISTS = (256, 4096)


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def cpu_milli(pod):
    total = 0
    for c in pod["spec"]["containers"]:
        v = str(c.get("resources", {}).get("requests", {}).get("cpu", "0"))
        total += int(v[:-1]) if v.endswith("m") else int(v) * 1000
    return total


def build_doc(n_nodes):
    from ksg import generator as g
    doc = g.generate(3, n_nodes=n_nodes, n_pods=max(LISTS))
    names = [n["metadata"]["name"] for n in doc["nodes"]]
    for i, p in enumerate(doc["queue"][::5]):  # a base load: DaemonSet-owned copies, bound round-robin
        d = copy.deepcopy(p)
        d["metadata"]["name"] = f"ds-{i:05d}"
        d["metadata"]["ownerReferences"] = [{"apiVersion": "apps/v1", "kind": "DaemonSet", "name": "ds", "uid": "u-ds",
                                             "controller": True}]
        d["spec"]["nodeName"] = names[(7 * i) % n_nodes]
        doc["pods"].append(d)
    return doc


def clone_doc(doc, t, k):
    """k clones of node t, each with copies of t's DaemonSet-owned pods."""
    name = doc["nodes"][t]["metadata"]["name"]
    base = [p for p in doc["pods"] if p["spec"].get("nodeName") == name and p["metadata"].get("ownerReferences")]
    nodes, pods = [], []
    for i in range(k):
        n = copy.deepcopy(doc["nodes"][t])
        n["metadata"]["name"] = f"clone-{i:04d}"
        nodes.append(n)
        for p in base:
            p = copy.deepcopy(p)
            p["metadata"]["name"] += f"-c{i}"
            p["spec"]["nodeName"] = n["metadata"]["name"]
            pods.append(p)
    return {"profile": doc["profile"], "nodes": nodes, "pods": pods, "queue": []}


def host_route(doc, t, k, pods, fit_pos):
    """(load us, route us, bins): negative bins are -1 closed, -2 refused by NodeResourcesFit (too big or
    over the cap: the route cannot tell them apart once every clone is opened)."""
    from ksg import Scheduler
    c = Scheduler(doc["profile"])
    load_us, _ = timed(lambda: c.load_cluster(clone_doc(doc, t, k)))

    def route():
        bins = []
        for i, pod in enumerate(pods):
            p = {"metadata": dict(pod["metadata"], name=f"{pod['metadata']['name']}-i{i}"), "spec": pod["spec"]}
            q, _ = c.cycle(p, commit=False)
            codes = c.filter_codes(q)
            dest = next((n for n, code in enumerate(codes) if code == PASSED), -1)
            if dest >= 0:
                c.reserve(q, dest)
                bins.append(dest)
            else:
                bins.append(-1 if codes[0] == NOT_EVALUATED or codes[0] >> 24 != fit_pos else -2)
        return bins
    us, bins = timed(route)
    c.close()
    return load_us, us, bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--host-templates", type=int, default=3, help="templates the host route is timed on (short list)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_up_latency.json"))
    a = ap.parse_args()
    from ksg import Scheduler
    from ksg.engine import _ScaleUp, SCALE_MAX
    doc = build_doc(a.nodes)
    fit_pos = doc["profile"]["plugins"].index("NodeResourcesFit")
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    at = {s.queue_pod(q): q for q in range(s.queue_len)}
    order = sorted(range(len(doc["queue"])), key=lambda i: (-cpu_milli(doc["queue"][i]), i))
    s.scale_up([], [])  # (binds the argument types)
    res = {"config": 3, "nodes": a.nodes, "queue_pods": len(doc["queue"]), "bound_pods": len(doc["pods"]),
           "max_nodes": SCALE_MAX, "calls_timed": a.calls, "warmup_calls": a.warmup, "shapes": [],
           "note": "host wall per call, each ending in a device synchronise; device route = one ksg_scale_up over all "
                   "templates; host route per template = a second context of clones, then per pod ksg_cycle(commit=0) + "
                   "ksg_filter_codes + ksg_reserve on the lowest passed clone, on a sample of templates, its bins equal to "
                   "ksg_scale_up_plan at the same clone count (the clone context's load is timed apart and not counted); "
                   "host_route_extrapolated_all_templates_us is an extrapolation, not a measurement"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    first_us = None
    for n_list in LISTS:
        listed = order[:n_list]
        lst = [at[(doc["queue"][i]["metadata"].get("namespace") or "default") + "/" + doc["queue"][i]["metadata"]["name"]]
               for i in listed]
        p = (ctypes.c_uint32 * n_list)(*lst)
        host = None
        for n_t in TEMPLATES:
            tm = [((2 * k + 1) * a.nodes) // (2 * n_t) for k in range(n_t)]  # (the midpoints: one template is the middle node)
            t = (ctypes.c_uint32 * n_t)(*tm)
            arr = (_ScaleUp * n_t)()
            gc.disable()
            dt, rc = timed(lambda: s.L.ksg_scale_up(s.h, p, n_list, t, n_t, SCALE_MAX, arr))
            assert rc == 0
            if first_us is None:
                first_us = dt
            ref = bytes(arr)
            us = []
            for i in range(a.warmup + a.calls):
                dt, rc = timed(lambda: s.L.ksg_scale_up(s.h, p, n_list, t, n_t, SCALE_MAX, arr))
                assert rc == 0 and bytes(arr) == ref
                if i >= a.warmup:
                    us.append(dt)
            gc.enable()
            got = s.scale_up(lst, tm)
            med = statistics.median(us)
            shape = {"templates": n_t, "pods": n_list, "scale_up": spread(us),
                     "pairs_per_s": n_t * n_list / (med * 1e-6),
                     "satisfied_templates": sum(1 for x in got if x.satisfied),
                     "templates_with_closed": sum(1 for x in got if x.closed),
                     "templates_with_too_big": sum(1 for x in got if x.too_big),
                     "templates_with_over_cap": sum(1 for x in got if x.over_cap),
                     "templates_with_base_pods": sum(1 for x in got if x.base_pods),
                     "max_nodes_opened": max(x.nodes for x in got), "scale_up_us": us}
            if host is None:  # the host route, once per list length, on a sample of the 256 templates' nodes
                n_host = a.host_templates if n_list == LISTS[0] else 1
                sample = [((2 * k + 1) * a.nodes) // (2 * n_host) for k in range(n_host)]
                host = {"us": [], "load_us": [], "clones": []}
                for x in sample:
                    k = min(SCALE_MAX, s.scale_up(lst, [x])[0].nodes + 1)
                    plan = s.scale_up_plan(lst, x, k)
                    load_us, route_us, bins = host_route(doc, x, k, [doc["queue"][i] for i in listed], fit_pos)
                    assert [b if b >= -1 else -2 for b in plan] == bins, (x, plan, bins)
                    host["us"].append(route_us)
                    host["load_us"].append(load_us)
                    host["clones"].append(k)
            hm = statistics.median(host["us"])
            shape["host_route_per_template"] = {"median_us": hm, "min_us": min(host["us"]), "max_us": max(host["us"])}
            shape["host_route_templates_timed"] = len(host["us"])
            shape["host_route_clones"] = host["clones"]
            shape["host_route_clone_context_load_us"] = host["load_us"]
            shape["host_route_bins_agree"] = True
            shape["host_route_extrapolated_all_templates_us"] = hm * n_t  # an extrapolation: per-template median x templates
            shape["host_extrapolated_over_device_median"] = hm * n_t / med
            res["shapes"].append(shape)
            res["first_call_after_load_us"] = first_us
            with open(a.out, "w") as f:  # (after every shape: a later one may not fit the time given)
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps({k: v for k, v in shape.items() if k != "scale_up_us"}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
