"""Latency of the eviction fit (ksg_bound_fit) against the route a caller had before it.

Shapes: cfg3-shaped documents from ksg_synth_cluster at 5,000, 20,000 and 50,000
nodes with five queue pods per node; the queue is scheduled on the device and
compacted, so the placed pods are the bound pods (their count is recorded: pods
that found no node are dropped).
  device route: ksg_bound_fit(0, bound) -- every (bound pod, node) pair in one call, 16 bytes
                per pod back.  The first call after the load is timed apart: it compiles
                every bound pod's program and uploads the store.
  host route:   per pod, apply_events(removePod), ksg_cycle(pod without spec.nodeName,
                commit = 0), ksg_filter_codes, apply_events(addPod) -- timed on --host-pods
                bound pods spread over the range, after the device route (an event batch
                moves the snapshot generation, so the next device call would pay the
                compile again).  Its per-pod median times the bound count is recorded as an
                extrapolation and named as one; the sample's codes are compared with
                ksg_bound_fit_nodes taken before the removal.
Warm-up calls, then --calls timed calls, a host clock around the C calls (each ends in a
device synchronise) with Python's collector off; median and p10-p90.  pairs/s = bound x
nodes / median.

usage: python tools/bench_bound_fit.py [--calls 20] [--warmup 3] [--shapes 5000,20000,50000]
                                       [--out profiles/bound_fit_latency.json]"""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def run_shape(n_nodes, a):
    from ksg import Scheduler, generator as g
    from ksg.engine import _BoundFit, _NodeEvict
    n_pods = n_nodes * a.pods_per_node
    doc = g.generate_native(3, n_nodes=n_nodes, n_pods=n_pods)
    print(f"[bench_bound_fit] document built: {n_nodes} nodes, {n_pods} pods, {len(doc) >> 20} MiB", file=sys.stderr,
          flush=True)
    prof = json.loads(doc[:doc.index(b',"nodes":[')] + b"}")["profile"]
    j = doc.rindex(b'"queue":[')
    by_name = {"default/" + p["metadata"]["name"]: p for p in json.loads(b"{" + doc[j:])["queue"]}
    s = Scheduler(prof)
    s.load_cluster(doc)
    del doc
    s.schedule()
    s.compact()
    nb = s.bound_count
    print(f"[bench_bound_fit] {nb} bound pods", file=sys.stderr, flush=True)
    # the C calls themselves, into buffers made once (the binding's lists of tuples are not what is timed),
    # with the collector off: a collection over the document's objects would land inside a call
    arr, evarr = (_BoundFit * nb)(), (_NodeEvict * n_nodes)()
    s.bound_fit(0, 0)  # (binds the argument types)
    gc.disable()
    first_us, rc = timed(lambda: s.L.ksg_bound_fit(s.h, 0, nb, arr))
    assert rc == 0
    first = bytes(arr)
    us = []
    for i in range(a.warmup + a.calls):
        dt, rc = timed(lambda: s.L.ksg_bound_fit(s.h, 0, nb, arr))
        assert rc == 0 and bytes(arr) == first
        if i >= a.warmup:
            us.append(dt)
    s.L.ksg_node_evictability.argtypes = [ctypes.c_void_p, ctypes.POINTER(_NodeEvict), ctypes.c_uint32]
    ev_us = [timed(lambda: s.L.ksg_node_evictability(s.h, evarr, n_nodes))[0]
             for _ in range(a.warmup + a.calls)][a.warmup:]
    gc.enable()
    fits, ev = s.bound_fit(0, nb), s.node_evictability()
    one_us = [timed(lambda: s.bound_fit_nodes(nb // 2))[0] for _ in range(a.warmup + a.calls)][a.warmup:]
    med = statistics.median(us)
    out = {"nodes": n_nodes, "queue_pods": n_pods, "bound_pods": nb, "pairs": nb * n_nodes, "calls_timed": a.calls,
           "warmup_calls": a.warmup, "first_call_after_load_us": first_us, "bound_fit": spread(us),
           "pairs_per_s": nb * n_nodes / (med * 1e-6), "node_evictability": spread(ev_us),
           "bound_fit_nodes_one_pod": spread(one_us),
           "own_node_would_not_admit": sum(1 for f in fits if f.own_code != 0xFFFFFFFF),
           "nowhere_else": sum(1 for f in fits if f.other_nodes == 0),
           "nodes_with_stuck_pods": sum(1 for e in ev if e.stuck), "bound_fit_us": us}
    # the host route, on a sample
    names = s.bound_pods()
    # (descending: a pod removed and added again moves to the end, which leaves the indices below it alone)
    sample = sorted({(k * nb) // a.host_pods for k in range(min(a.host_pods, nb))}, reverse=True)
    rows = {b: s.bound_fit_nodes(b) for b in sample}  # (before the first event batch moves the generation)
    host_us = []
    for b in sample:
        name, node = names[b]
        pod, want = by_name[name], rows[b]
        free = {"metadata": pod["metadata"], "spec": {k: v for k, v in pod["spec"].items() if k != "nodeName"}}
        back = {"metadata": pod["metadata"], "spec": dict(pod["spec"], nodeName=f"node-{node:07d}")}

        def route():
            s.apply_events([{"op": "removePod", "name": pod["metadata"]["name"], "namespace": "default"}])
            q, _ = s.cycle(free, commit=False)
            codes = s.filter_codes(q)
            s.apply_events([{"op": "addPod", "pod": back}])
            return codes
        dt, codes = timed(route)
        assert codes == want, name
        host_us.append(dt)
    hm = statistics.median(host_us)
    out["host_route_per_pod"] = spread(host_us) if len(host_us) > 1 else {"median_us": hm}
    out["host_route_pods_timed"] = len(host_us)
    out["host_route_extrapolated_all_bound_us"] = hm * nb  # an extrapolation: per-pod median x bound pods
    out["host_extrapolated_over_device_median"] = hm * nb / med
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-pods", type=int, default=16, help="bound pods the host route is timed on")
    ap.add_argument("--pods-per-node", type=int, default=5)
    ap.add_argument("--shapes", default="5000,20000,50000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_fit_latency.json"))
    a = ap.parse_args()
    res = {"config": 3, "shapes": [], "headroom_pairs_per_s_recorded": 4.1e10,
           "note": "host wall per call, each ending in a device synchronise; device route = ksg_bound_fit(0, bound); "
                   "host route per pod = removePod + ksg_cycle(commit=0) + ksg_filter_codes + addPod on a sample; "
                   "host_route_extrapolated_all_bound_us is an extrapolation, not a measurement"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in (int(v) for v in a.shapes.split(",")):
        res["shapes"].append(run_shape(n, a))
        with open(a.out, "w") as f:  # (after every shape: a later one may not fit the time given)
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in res["shapes"][-1].items() if k != "bound_fit_us"}), flush=True)


if __name__ == "__main__":
    main()
