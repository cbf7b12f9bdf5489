"""Latency of the FitError sentence against the route a caller had before it.

The cfg4 cluster at bench size (50,000 nodes, 200,000 bound pods), plugin mode:
one ksg_cycle(commit = 0) per pod, every pod made unschedulable by an oversized
cpu request, then for that pod
  device route: ksg_fit_error(q) -- the per-reason counts on the device, a few
                hundred bytes back, the sentence rendered by the library;
  host route:   ksg_filter_codes (N x 4 bytes over the host link), a numpy
                unique-count, one ksg_filter_status per distinct code for its
                message, and the same string assembly in Python.
Both routes run for every pod in one process, alternating which goes first, timed
with a host clock around calls that end in a device synchronise; the first pods
are warm-up and discarded; the two strings must be equal for every pod.  Raw
per-call times, medians and spread go to the output file.

usage: python tools/bench_diagnosis.py [--nodes 50000] [--pods 40] [--warmup 8] [--out profiles/diagnosis_latency.json]"""
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

PASSED, NOT_EVALUATED = 0xFFFFFFFF, 0xFFFFFFFE


def host_route(s, q, n_positions, n_local, n_all):
    """FitError.Error() from the per-node export (what a caller could do before ksg_fit_error;
    these pods pass every PreFilter, so the sentence comes from the nodes)."""
    codes = np.empty(n_local, np.uint32)
    s._chk(s.L.ksg_filter_codes(s.h, q, codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n_local),
           "ksg_filter_codes")
    uniq, first, counts = np.unique(codes, return_index=True, return_counts=True)
    reasons = {}
    for code, node, cnt in zip(uniq.tolist(), first.tolist(), counts.tolist()):
        if code in (PASSED, NOT_EVALUATED):
            continue
        for pos in range(n_positions):  # the failing position's Status.Message() on one such node
            st, msg = s.filter_status(q, pos, node)
            if st > 0:
                break
        for r in msg.split(", "):
            reasons[r] = reasons.get(r, 0) + cnt
    out = f"0/{n_all} nodes are available:"
    entries = sorted(f"{c} {r}".encode() for r, c in reasons.items())
    if entries:
        out += " " + b", ".join(entries).decode() + "."
    return out


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--pods", type=int, default=40, help="timed pods")
    ap.add_argument("--warmup", type=int, default=8, help="pods before them, both routes run, times discarded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnosis_latency.json"))
    a = ap.parse_args()
    from ksg import Scheduler, generator as g  # (no device: ksg_create fails, nothing is measured)
    doc = json.loads(g.generate_native(4, n_nodes=a.nodes, n_pods=a.pods + a.warmup))
    print(f"[bench_diagnosis] document built: {len(doc['nodes'])} nodes, {len(doc['pods'])} bound pods", file=sys.stderr,
          flush=True)
    s = Scheduler(doc["profile"])
    s.load_cluster(dict(doc, queue=[]))
    n, n_positions = s.n_nodes, len(doc["profile"]["plugins"])
    dev_us, host_us, reasons = [], [], []
    for i, pod in enumerate(doc["queue"]):
        c0 = pod["spec"]["containers"][0]
        c0.setdefault("resources", {}).setdefault("requests", {})["cpu"] = "10000"  # no node has 10,000 cpus
        q, r = s.cycle(pod, commit=False)
        assert r.status == 1 and r.feasible == 0, (i, r)
        got = {}
        for route in (("device", "host") if i % 2 == 0 else ("host", "device")):
            t0 = time.perf_counter()
            got[route] = s.fit_error(q) if route == "device" else host_route(s, q, n_positions, n, n)
            dt = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                (dev_us if route == "device" else host_us).append(dt)
        assert got["device"] == got["host"], (i, got["device"][:200], got["host"][:200])
        if i >= a.warmup:
            reasons.append(got["device"].count(", ") + 1)
    out = {"config": 4, "nodes": n, "bound_pods": len(doc["pods"]), "pods_timed": len(dev_us), "warmup_pods": a.warmup,
           "host_route_bytes_per_pod": n * 4, "reasons_median": statistics.median(reasons),
           "diag_routes_device_host": list(s.diag_routes()),
           "device_route": spread(dev_us), "host_route": spread(host_us),
           "host_over_device_median": statistics.median(host_us) / statistics.median(dev_us),
           "strings_equal": True, "example": got["device"],
           "note": "host wall per call, each ending in a device synchronise; one call of each route per pod, order "
                   "alternating; device route = ksg_fit_error(q); host route = ksg_filter_codes + numpy unique-count + "
                   "ksg_filter_status per distinct code + the string assembly in Python",
           "device_us": dev_us, "host_us": host_us}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("device_us", "host_us", "note", "example")}))


if __name__ == "__main__":
    main()
