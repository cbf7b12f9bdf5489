"""Latency of the drain simulation (ksg_drain) against the route a caller had before it.

Shapes, as tools/bench_bound_fit.py: cfg3-shaped documents from ksg_synth_cluster at
5,000, 20,000 and 50,000 nodes with five queue pods per node; the queue is scheduled
on the device and compacted, so the placed pods are the bound pods.  A freshly
scheduled cluster is LOOSE: most subjects find a node in the first tile of the walk.
One TIGHT shape is recorded beside them and named as such (--tight-nodes): before the
load every node's pod limit is set to the pods per node, every 16th node's to twice
that, so after the queue run most nodes are full and a subject walks until it meets
one of the open nodes, which the earlier subjects of the same drain fill up.
  device route: ksg_drain(0, nodes) -- every node's drain in one call, 32 bytes per
                node back.  The first call after the load is timed apart: it compiles
                every bound pod's program and uploads the store.
  host route:   per subject of a node, apply_events(removePod), ksg_cycle(pod without
                spec.nodeName, commit = 0), ksg_filter_codes, the lowest passed node
                other than the candidate, apply_events(addPod there) -- timed per node on
                --host-nodes nodes spread over the range, after the device route; the
                moves are compared with ksg_drain_plan taken just before (outside the
                timed part).  Its per-node median times the node count is recorded as
                an extrapolation and named as one.
Warm-up calls, then --calls timed calls, a host clock around the C calls (each ends in a
device synchronise) with Python's collector off; median and p10-p90.

usage: python tools/bench_drain.py [--calls 20] [--warmup 3] [--shapes 5000,20000,50000]
                                   [--tight-nodes 5000] [--out profiles/drain_latency.json]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))

PASSED = 0xFFFFFFFF


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def run_shape(n_nodes, a, tight):
    from ksg import Scheduler, generator as g
    from ksg.engine import _Drain
    n_pods = n_nodes * a.pods_per_node
    doc = g.generate_native(3, n_nodes=n_nodes, n_pods=n_pods)
    print(f"[bench_drain] document built: {n_nodes} nodes, {n_pods} pods, {len(doc) >> 20} MiB"
          f"{' (tight)' if tight else ''}", file=sys.stderr, flush=True)
    prof = json.loads(doc[:doc.index(b',"nodes":[')] + b"}")["profile"]
    if tight:
        d = json.loads(doc)
        for i, n in enumerate(d["nodes"]):
            for k in ("allocatable", "capacity"):
                n["status"][k]["pods"] = str(a.pods_per_node * (2 if i % 16 == 15 else 1))
        by_name = {"default/" + p["metadata"]["name"]: p for p in d["queue"]}
        doc = json.dumps(d, separators=(",", ":")).encode()
        del d
    else:
        j = doc.rindex(b'"queue":[')
        by_name = {"default/" + p["metadata"]["name"]: p for p in json.loads(b"{" + doc[j:])["queue"]}
    s = Scheduler(prof)
    s.load_cluster(doc)
    del doc
    s.schedule()
    s.compact()
    nb = s.bound_count
    print(f"[bench_drain] {nb} bound pods", file=sys.stderr, flush=True)
    arr = (_Drain * n_nodes)()
    s.drain(0, 0)  # (binds the argument types)
    gc.disable()
    first_us, rc = timed(lambda: s.L.ksg_drain(s.h, 0, n_nodes, arr))
    assert rc == 0
    first = bytes(arr)
    us = []
    for i in range(a.warmup + a.calls):
        dt, rc = timed(lambda: s.L.ksg_drain(s.h, 0, n_nodes, arr))
        assert rc == 0 and bytes(arr) == first
        if i >= a.warmup:
            us.append(dt)
    gc.enable()
    drains = s.drain()
    mid = next(x for x in range(n_nodes // 2, n_nodes) if drains[x].placed + drains[x].unplaced)  # (a node with subjects)
    one_us = [timed(lambda: s.drain_plan(mid))[0] for _ in range(a.warmup + a.calls)][a.warmup:]
    med = statistics.median(us)
    subjects = sum(d.placed + d.unplaced for d in drains)
    out = {"nodes": n_nodes, "shape": "tight" if tight else "loose", "queue_pods": n_pods, "bound_pods": nb,
           "subjects_simulated": subjects, "calls_timed": a.calls, "warmup_calls": a.warmup,
           "first_call_after_load_us": first_us, "drain_all_nodes": spread(us), "nodes_per_s": n_nodes / (med * 1e-6),
           "subjects_per_s": subjects / (med * 1e-6), "drain_plan_one_node": spread(one_us),
           "drainable_nodes": sum(1 for d in drains if d.drainable),
           "nodes_with_unplaced": sum(1 for d in drains if d.unplaced),
           "unplaced_subjects": sum(d.unplaced for d in drains),
           "max_dest_nodes": max(d.dest_nodes for d in drains), "drain_us": us}
    # the host route, on a sample of nodes
    sample = sorted({(k * n_nodes) // a.host_nodes + 1 for k in range(min(a.host_nodes, n_nodes))})
    host_us, host_subjects = [], 0
    for x in sample:
        plan = s.drain_plan(x)  # (just before: the earlier nodes' moves are part of the snapshot)
        pods = [by_name[bound_name(s, b)] for b, _ in plan]

        def route():
            moves = []
            for pod in pods:
                free = {"metadata": pod["metadata"], "spec": {k: v for k, v in pod["spec"].items() if k != "nodeName"}}
                s.apply_events([{"op": "removePod", "name": pod["metadata"]["name"], "namespace": "default"}])
                q, _ = s.cycle(free, commit=False)
                codes = s.filter_codes(q)
                dest = next((n for n, c in enumerate(codes) if c == PASSED and n != x), -1)
                back = {"metadata": pod["metadata"],
                        "spec": dict(pod["spec"], nodeName=f"node-{dest if dest >= 0 else x:07d}")}
                s.apply_events([{"op": "addPod", "pod": back}])
                moves.append(dest)
            return moves
        dt, moves = timed(route)
        assert moves == [d for _, d in plan], (x, moves, plan)
        if pods:
            host_us.append(dt)
            host_subjects += len(pods)
    hm = statistics.median(host_us)
    out["host_route_per_node"] = {"median_us": hm, "min_us": min(host_us), "max_us": max(host_us)}  # (a handful: no deciles)
    out["host_route_nodes_timed"] = len(host_us)
    out["host_route_subjects_timed"] = host_subjects
    out["host_route_plans_agree"] = True
    out["host_route_extrapolated_all_nodes_us"] = hm * n_nodes  # an extrapolation: per-node median x nodes
    out["host_extrapolated_over_device_median"] = hm * n_nodes / med
    s.close()
    return out


def bound_name(s, b):
    import ctypes
    n, node = ctypes.c_size_t(), ctypes.c_int32()
    buf = ctypes.create_string_buffer(1024)
    s.L.ksg_bound_pod.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
    assert s.L.ksg_bound_pod(s.h, b, buf, 1024, ctypes.byref(n), ctypes.byref(node)) == 0
    return buf.raw[:n.value].decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-nodes", type=int, default=4, help="nodes the host route is timed on")
    ap.add_argument("--pods-per-node", type=int, default=5)
    ap.add_argument("--shapes", default="5000,20000,50000")
    ap.add_argument("--tight-nodes", type=int, default=5000, help="node count of the tight shape (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drain_latency.json"))
    a = ap.parse_args()
    res = {"config": 3, "shapes": [],
           "note": "host wall per call, each ending in a device synchronise; device route = ksg_drain(0, nodes); host "
                   "route per node = per subject removePod + ksg_cycle(commit=0) + ksg_filter_codes + addPod on the "
                   "destination, on a sample of nodes, its moves equal to ksg_drain_plan; "
                   "host_route_extrapolated_all_nodes_us is an extrapolation, not a measurement; shape loose: "
                   "freshly scheduled, most subjects hit in the first tile; shape tight: pod limits set so that "
                   "15 of 16 nodes are full after the queue run and scans run long"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    todo = [(int(v), False) for v in a.shapes.split(",") if v] + ([(a.tight_nodes, True)] if a.tight_nodes else [])
    for n, tight in todo:
        res["shapes"].append(run_shape(n, a, tight))
        with open(a.out, "w") as f:  # (after every shape: a later one may not fit the time given)
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in res["shapes"][-1].items() if k != "drain_us"}), flush=True)


if __name__ == "__main__":
    main()
