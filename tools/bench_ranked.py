"""Latency of the ranked-candidates call against the route a caller had before it.

The cfg4 cluster at bench size (50,000 nodes, 200,000 bound pods), plugin mode:
one ksg_cycle(commit = 0) per pod, then for that pod
  device route: ksg_ranked_nodes(q, 64) -- the select on the device, <= 512 bytes back;
  host route:   ksg_filter_codes + ksg_normalized_scores for every scoring position
                (N x (4 + 8 P) bytes over the host link), the weighted sum, the seeded
                tie-break hash and a numpy partial sort on the host;
then ksg_reserve on the engine's choice.  Both routes run for every pod in one
process, alternating which goes first; each is timed once per pod (its first call:
the host layer caches a pod's outputs, so a repeat would time the cache) with a host
clock around calls that end in a device synchronise; the first pods are warm-up and
discarded; the two lists must be equal.  Raw per-call times, medians and spread go
to the output file.

usage: python tools/bench_ranked.py [--nodes 50000] [--pods 40] [--warmup 8] [--out profiles/ranked_latency.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))

SCORERS = {"NodeResourcesFit", "NodeResourcesBalancedAllocation", "TaintToleration", "NodeAffinity",
           "PodTopologySpread", "InterPodAffinity", "ImageLocality"}
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
K = 64


def host_route(s, q, plugins, seed, n):
    """The ranked list from the per-node exports (what a caller could do before ksg_ranked_nodes)."""
    L, u64 = s.L, np.uint64
    codes = np.empty(n, np.uint32)
    s._chk(L.ksg_filter_codes(s.h, q, codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n), "ksg_filter_codes")
    feas = np.flatnonzero(codes == 0xFFFFFFFF)
    if len(feas) == 0:
        return []
    total = np.zeros(n, np.int64)
    if len(feas) > 1:
        norm = np.empty(n, np.int64)
        for pos, pl in enumerate(plugins):
            if pl in SCORERS and (s.prescore_status(q, pos)[0] == 0 or pl == "ImageLocality"):
                s._chk(L.ksg_normalized_scores(s.h, q, pos, norm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n),
                       "ksg_normalized_scores")
                total += norm * s.plugin_weights(pos)[0]
    with np.errstate(over="ignore"):  # splitmix64 of seed ^ q * GOLDEN ^ node, top 20 bits
        z = (u64(seed) ^ u64((q * GOLDEN) & M64) ^ feas.astype(u64)) + u64(GOLDEN)
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        h20 = (z ^ (z >> u64(31))) >> u64(44)
        keys = (total[feas].astype(u64) << u64(40)) | ((u64(0xFFFFF) - h20) << u64(20)) | feas.astype(u64)
    k = min(K, len(keys))
    top = np.partition(keys, len(keys) - k)[len(keys) - k:]
    top = np.sort(top)[::-1]
    return [(int(x) & 0xFFFFF, int(x) >> 40) for x in top]


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--pods", type=int, default=40, help="timed pods")
    ap.add_argument("--warmup", type=int, default=8, help="pods before them, both routes run, times discarded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranked_latency.json"))
    a = ap.parse_args()
    from ksg import Scheduler, generator as g  # (no device: ksg_create fails, nothing is measured)
    doc = json.loads(g.generate_native(4, n_nodes=a.nodes, n_pods=a.pods + a.warmup))
    print(f"[bench_ranked] document built: {len(doc['nodes'])} nodes, {len(doc['pods'])} bound pods", file=sys.stderr,
          flush=True)
    s = Scheduler(doc["profile"])
    s.load_cluster(dict(doc, queue=[]))
    n, plugins, seed = s.n_nodes, doc["profile"]["plugins"], doc["profile"]["seed"]
    dev_us, host_us, feasible = [], [], []
    for i, pod in enumerate(doc["queue"]):
        q, r = s.cycle(pod, commit=False)
        got = {}
        for route in (("device", "host") if i % 2 == 0 else ("host", "device")):
            t0 = time.perf_counter()
            got[route] = s.ranked_nodes(q, K) if route == "device" else host_route(s, q, plugins, seed, n)
            dt = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                (dev_us if route == "device" else host_us).append(dt)
        assert got["device"] == got["host"], (i, got["device"][:3], got["host"][:3])
        if r.status == 0:
            assert got["device"][0] == (r.selected, r.total), (i, got["device"][0], r)
            s.reserve(q, r.selected)
        if i >= a.warmup:
            feasible.append(r.feasible)
    positions = sum(1 for pl in plugins if pl in SCORERS)
    out = {"config": 4, "nodes": n, "bound_pods": len(doc["pods"]), "k": K, "pods_timed": len(dev_us), "warmup_pods": a.warmup,
           "scoring_positions": positions, "host_route_bytes_per_pod": n * (4 + 8 * positions),
           "feasible_median": statistics.median(feasible),
           "device_route": spread(dev_us), "host_route": spread(host_us),
           "host_over_device_median": statistics.median(host_us) / statistics.median(dev_us),
           "lists_equal": True,
           "note": "host wall per call, each ending in a device synchronise; one call of each route per pod, order "
                   "alternating; device route = ksg_ranked_nodes(q, 64); host route = ksg_filter_codes + "
                   "ksg_normalized_scores per scoring position + weighted sum + hash + numpy partial sort",
           "device_us": dev_us, "host_us": host_us}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("device_us", "host_us", "note")}))


if __name__ == "__main__":
    main()
