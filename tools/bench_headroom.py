"""Latency of the headroom call against the route a caller had before it.

Shapes: one pod at 5,000 and at 50,000 nodes, and a 4,096-pod batch at cfg5's
1,000,000 nodes (cfg5 documents from ksg_synth_cluster).
  device route: ksg_headroom(first, count) -- one launch for the range, 64 bytes per pod back;
  host route:   ksg_node_requested (every requested row and the pod counts over the host
                link) plus numpy floor division over the DOCUMENT's allocatable,
                NodeResourcesFit only: min(room, min_r floor(free_r / request_r)) summed
                per pod.  This is what a caller could do before the call; it ignores
                taints, node affinity, spec.nodeName and cordoned nodes, so its replica
                counts are an upper bound of the device route's and are not compared
                beyond that.  It is a baseline, not the code under test.
Warm-up calls of both routes, then at least 20 timed calls each, alternating, a host
clock around calls that end in a device synchronise.  At the batch shape a host-route
call covers --host-pods pods of the batch (the whole batch would take minutes per
call); its per-pod time times the batch size is recorded as an extrapolation and named
as one.  The device route's kernel bytes are the node rows a block reads,
(2 R x 8 + 8) bytes per node per pod tile of 32 pods.

usage: python tools/bench_headroom.py [--calls 20] [--warmup 3] [--shapes 5000x1,50000x1,1000000x4096]
                                      [--out profiles/headroom_latency.json]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))

UNIT = {"Ki": 1 << 10, "Mi": 1 << 20, "Gi": 1 << 30, "Ti": 1 << 40}
ALLOC = re.compile(rb'"allocatable":\{"cpu":"([0-9m]+)","memory":"([0-9A-Za-z]+)","pods":"([0-9]+)"\}')


def quantity(name, s):
    s = s.decode() if isinstance(s, bytes) else str(s)
    if s[-2:] in UNIT:
        return int(s[:-2]) * UNIT[s[-2:]]
    if s.endswith("m"):
        return int(s[:-1])
    return int(s) * (1000 if name == "cpu" else 1)


def allocatable(doc_bytes, n):
    """(cpu milli, memory bytes, pods) of every node from the document text (cfg5 nodes carry these three)."""
    rows = [(quantity("cpu", m.group(1)), quantity("memory", m.group(2)), int(m.group(3)))
            for m in ALLOC.finditer(doc_bytes)]
    assert len(rows) == n, (len(rows), n)
    a = np.array(rows, dtype=np.int64)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def queue_requests(doc_bytes):
    """(cpu milli, memory bytes) of every queue pod, summed over its containers."""
    j = doc_bytes.rindex(b'"queue":[')
    queue = json.loads(b"{" + doc_bytes[j:])["queue"]
    out = []
    for p in queue:
        cpu = mem = 0
        for c in p["spec"]["containers"]:
            rq = c.get("resources", {}).get("requests", {})
            cpu += quantity("cpu", rq["cpu"]) if "cpu" in rq else 0
            mem += quantity("memory", rq["memory"]) if "memory" in rq else 0
        out.append((cpu, mem))
    return out


def host_route(s, alloc, reqs, first, count):
    """Replicas per pod from ksg_node_requested and the document's allocatable (Fit only)."""
    n = s.n_nodes
    requested = np.empty((8, n), np.int64)
    podcnt = np.empty(n, np.int32)
    s._chk(s.L.ksg_node_requested(s.h, requested.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  podcnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 8, n), "ksg_node_requested")
    room = np.maximum(alloc[2] - podcnt, 0)
    free = (np.maximum(alloc[0] - requested[0], -1), np.maximum(alloc[1] - requested[1], -1))
    out = []
    for q in range(first, first + count):
        cnt = room
        for r in (0, 1):
            if reqs[q][r] > 0:
                cnt = np.minimum(cnt, np.where(free[r] < 0, 0, free[r] // reqs[q][r]))
        out.append(int(cnt.sum()))
    return out


def spread(us):
    qs = statistics.quantiles(us, n=10)
    return {"median_us": statistics.median(us), "p10_us": qs[0], "p90_us": qs[-1], "min_us": min(us), "max_us": max(us)}


def run_shape(n_nodes, n_pods, a):
    from ksg import Scheduler, generator as g
    doc = g.generate_native(5, n_nodes=n_nodes, n_pods=n_pods)
    print(f"[bench_headroom] document built: {n_nodes} nodes, {n_pods} pods, {len(doc) >> 20} MiB", file=sys.stderr,
          flush=True)
    alloc, reqs = allocatable(doc, n_nodes), queue_requests(doc)
    prof = json.loads(doc[:doc.index(b',"nodes":[')] + b"}")["profile"]
    s = Scheduler(prof)
    s.load_cluster(doc)
    del doc
    assert s.n_nodes == n_nodes and s.queue_len == n_pods
    host_pods = min(n_pods, a.host_pods)
    R = len(s.resource_names())
    dev_us, host_us, dev, host = [], [], None, None
    for i in range(a.warmup + a.calls):
        for route in (("device", "host") if i % 2 == 0 else ("host", "device")):
            t0 = time.perf_counter()
            if route == "device":
                dev = s.headroom(0, n_pods)
            else:
                host = host_route(s, alloc, reqs, 0, host_pods)
            dt = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                (dev_us if route == "device" else host_us).append(dt)
    # the host route ignores the static filters: an upper bound of the device route's replicas,
    # equal where every node is open
    for q in range(host_pods):
        assert dev[q].replicas <= host[q], (q, dev[q], host[q])
        if dev[q].open_nodes == n_nodes:
            assert dev[q].replicas == host[q], (q, dev[q], host[q])
    dm, hm = statistics.median(dev_us), statistics.median(host_us)
    tiles = (n_pods + 31) // 32
    out = {"nodes": n_nodes, "pods": n_pods, "resource_columns": R, "calls_timed": a.calls, "warmup_calls": a.warmup,
           "device_route": spread(dev_us), "host_route": spread(host_us), "host_route_pods_per_call": host_pods,
           "device_kernel_row_bytes": tiles * n_nodes * (2 * R * 8 + 8),
           "host_route_link_bytes_per_call": n_nodes * (8 * R + 4),
           "replicas_first_pod": dev[0].replicas, "open_nodes_first_pod": dev[0].open_nodes,
           "device_us": dev_us, "host_us": host_us}
    if host_pods == n_pods:
        out["host_over_device_median"] = hm / dm
    else:  # named for what it is: the measured per-pod host time times the batch size
        out["host_route_extrapolated_batch_us"] = hm / host_pods * n_pods
        out["host_extrapolated_over_device_median"] = hm / host_pods * n_pods / dm
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each route per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-pods", type=int, default=16, help="pods a host-route call covers at a batch shape")
    ap.add_argument("--shapes", default="5000x1,50000x1,1000000x4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headroom_latency.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")]
    res = {"config": 5, "shapes": [run_shape(n, p, a) for n, p in shapes],
           "note": "host wall per call, each ending in a device synchronise; routes alternate; device route = "
                   "ksg_headroom(0, pods); host route = ksg_node_requested + numpy floor division over the "
                   "document's allocatable, NodeResourcesFit only (no static filters): a baseline"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for sh in res["shapes"]:
        print(json.dumps({k: v for k, v in sh.items() if k not in ("device_us", "host_us")}))


if __name__ == "__main__":
    main()
