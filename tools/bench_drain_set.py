"""Latency of the set drain (ksg_drain_sets, ksg_drain_prefixes) against the routes a
caller had before it.

Shapes, as tools/bench_drain.py: cfg3-shaped documents from ksg_synth_cluster at 5,000,
20,000 and 50,000 nodes with five queue pods per node, scheduled on the device and
compacted (LOOSE: most subjects find a node in the first tile), and one TIGHT shape
(--tight-nodes): pod limits set so that 15 of 16 nodes are full after the queue run.
  ksg_drain_sets:     256 sets of 16 consecutive nodes (nodes [16 i, 16 i + 16)), one call.
  ksg_drain_prefixes: the prefixes of 100 nodes spread over the range, one call.
  ksg_drain:          ksg_drain over the same 4,096 nodes, one call.  It answers a weaker
                      question -- every node alone, the other members open as destinations
                      -- and is recorded as the cost of the device walk without the set.
  event route:        per subject of a set, apply_events(removePod), ksg_cycle(pod without
                      spec.nodeName, commit = 0), ksg_filter_codes, the lowest passed node
                      outside the set, apply_events(addPod there) -- timed on --host-sets sets of
                      --host-set-nodes nodes (a subject costs this route 0.07 to 1.2 s), after
                      the device calls; the moves are compared with ksg_drain_set_plan taken
                      just before (outside the timed part).  Its time per subject times the
                      subjects of the 256 sets is recorded as an extrapolation and named one.
Warm-up calls, then --calls timed calls, a host clock around the C call (each ends in a
device synchronise) with Python's collector off; median and p10-p90.

usage: python tools/bench_drain_set.py [--calls 20] [--warmup 3] [--shapes 5000,20000,50000]
                                       [--tight-nodes 5000] [--out profiles/drain_set_latency.json]"""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_drain import PASSED, bound_name, spread, timed  # noqa: E402

N_SETS, SET_SIZE, N_PREFIX = 256, 16, 100


def series(a, call, check):
    us = []
    for i in range(a.warmup + a.calls):
        dt, rc = timed(call)
        assert rc == 0 and check()
        if i >= a.warmup:
            us.append(dt)
    return us


def run_shape(n_nodes, a, tight):
    from ksg import Scheduler, generator as g
    from ksg.engine import _Drain, _DrainSet
    n_pods = n_nodes * a.pods_per_node
    doc = g.generate_native(3, n_nodes=n_nodes, n_pods=n_pods)
    print(f"[bench_drain_set] document built: {n_nodes} nodes, {n_pods} pods, {len(doc) >> 20} MiB"
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
    print(f"[bench_drain_set] {nb} bound pods", file=sys.stderr, flush=True)
    sets = [list(range(SET_SIZE * i, SET_SIZE * i + SET_SIZE)) for i in range(N_SETS)]
    prefix = [(k * n_nodes) // N_PREFIX for k in range(N_PREFIX)]
    s.drain(0, 0)  # (binds the argument types)
    s.drain_sets([])
    s.drain_prefixes([])
    n_flat = N_SETS * SET_SIZE
    flat = (ctypes.c_uint32 * n_flat)(*range(n_flat))
    start = (ctypes.c_uint32 * (N_SETS + 1))(*range(0, n_flat + 1, SET_SIZE))
    pre = (ctypes.c_uint32 * N_PREFIX)(*prefix)
    o_sets, o_pre, o_drain = (_DrainSet * N_SETS)(), (_DrainSet * N_PREFIX)(), (_Drain * n_flat)()
    gc.disable()
    first_us, rc = timed(lambda: s.L.ksg_drain_sets(s.h, flat, start, N_SETS, o_sets))
    assert rc == 0
    first = bytes(o_sets)
    us_sets = series(a, lambda: s.L.ksg_drain_sets(s.h, flat, start, N_SETS, o_sets), lambda: bytes(o_sets) == first)
    assert s.L.ksg_drain_prefixes(s.h, pre, N_PREFIX, o_pre) == 0
    first_pre = bytes(o_pre)
    us_pre = series(a, lambda: s.L.ksg_drain_prefixes(s.h, pre, N_PREFIX, o_pre), lambda: bytes(o_pre) == first_pre)
    us_drain = series(a, lambda: s.L.ksg_drain(s.h, 0, n_flat, o_drain), lambda: True)
    gc.enable()
    got, pres, alone = s.drain_sets(sets), s.drain_prefixes(prefix), s.drain(0, n_flat)
    med = statistics.median(us_sets)
    subjects = sum(d.placed + d.unplaced for d in got)
    out = {"nodes": n_nodes, "shape": "tight" if tight else "loose", "queue_pods": n_pods, "bound_pods": nb,
           "sets": N_SETS, "set_size": SET_SIZE, "prefix_nodes": N_PREFIX, "calls_timed": a.calls,
           "warmup_calls": a.warmup, "first_call_after_load_us": first_us,
           "drain_sets_256x16": spread(us_sets), "sets_per_s": N_SETS / (med * 1e-6),
           "subjects_simulated": subjects, "subjects_per_s": subjects / (med * 1e-6),
           "drain_prefixes_100": spread(us_pre),
           "prefix_subjects_simulated": sum(d.placed + d.unplaced for d in pres),
           "ksg_drain_same_4096_nodes": spread(us_drain),
           "drain_sets_over_ksg_drain_median": med / statistics.median(us_drain),
           "removable_sets": sum(1 for d in got if d.removable),
           "sets_blocked_though_every_member_drainable": sum(
               1 for i, d in enumerate(got) if not d.removable and all(alone[x].drainable for x in sets[i])),
           "removable_prefixes": sum(1 for d in pres if d.removable),
           "max_dest_nodes": max(d.dest_nodes for d in got + pres), "max_skipped": max(d.skipped for d in got + pres),
           "drain_sets_us": us_sets, "drain_prefixes_us": us_pre, "ksg_drain_us": us_drain}
    # the event route, on a few sets
    host_us, host_subjects = [], 0
    for i in sorted({(k * N_SETS) // a.host_sets for k in range(a.host_sets)}):
        nodes = sets[i][:a.host_set_nodes]
        plan = s.drain_set_plan(nodes)  # (just before: the earlier sets' moves are part of the snapshot)
        pods = [(by_name[name], x) for name, x in (bound_pod(s, b) for b, _ in plan)]

        def route():
            moves = []
            for pod, x in pods:
                free = {"metadata": pod["metadata"], "spec": {k: v for k, v in pod["spec"].items() if k != "nodeName"}}
                s.apply_events([{"op": "removePod", "name": pod["metadata"]["name"], "namespace": "default"}])
                q, _ = s.cycle(free, commit=False)
                codes = s.filter_codes(q)
                dest = next((n for n, c in enumerate(codes) if c == PASSED and n not in nodes), -1)
                back = {"metadata": pod["metadata"],
                        "spec": dict(pod["spec"], nodeName=f"node-{dest if dest >= 0 else x:07d}")}
                s.apply_events([{"op": "addPod", "pod": back}])
                moves.append(dest)
            return moves
        dt, moves = timed(route)
        assert moves == [d for _, d in plan], (nodes, moves, plan)
        if pods:
            host_us.append(dt)
            host_subjects += len(pods)
    per_subject = sum(host_us) / host_subjects
    out["event_route_per_set"] = {"median_us": statistics.median(host_us), "min_us": min(host_us),
                                  "max_us": max(host_us)}  # (a few: no deciles)
    out["event_route_set_nodes"] = a.host_set_nodes
    out["event_route_sets_timed"] = len(host_us)
    out["event_route_subjects_timed"] = host_subjects
    out["event_route_per_subject_us"] = per_subject
    out["event_route_plans_agree"] = True
    # an extrapolation: the time per subject x the subjects the 256 x 16 call simulated
    out["event_route_extrapolated_256_sets_us"] = per_subject * subjects
    out["event_extrapolated_over_device_median"] = per_subject * subjects / med
    s.close()
    return out


def bound_pod(s, b):
    node = ctypes.c_int32()
    n = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(1024)
    name = bound_name(s, b)
    assert s.L.ksg_bound_pod(s.h, b, buf, 1024, ctypes.byref(n), ctypes.byref(node)) == 0
    return name, node.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sets", type=int, default=2, help="sets the event route is timed on")
    ap.add_argument("--host-set-nodes", type=int, default=4, help="nodes of each such set (the first of a 16-node set)")
    ap.add_argument("--pods-per-node", type=int, default=5)
    ap.add_argument("--shapes", default="5000,20000,50000")
    ap.add_argument("--tight-nodes", type=int, default=5000, help="node count of the tight shape (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drain_set_latency.json"))
    a = ap.parse_args()
    res = {"config": 3, "shapes": [],
           "note": "host wall per call, each ending in a device synchronise; drain_sets_256x16 = ksg_drain_sets over 256 "
                   "sets of 16 consecutive nodes; drain_prefixes_100 = ksg_drain_prefixes over 100 nodes spread over the "
                   "range; ksg_drain_same_4096_nodes answers a weaker question (every node alone); event route per set = "
                   "per subject removePod + ksg_cycle(commit=0) + ksg_filter_codes + addPod on the destination, on a few "
                   "sets of event_route_set_nodes nodes, its moves equal to ksg_drain_set_plan; event_route_extrapolated_256_sets_us is an "
                   "extrapolation, not a measurement; shape loose: freshly scheduled, most subjects hit in the first "
                   "tile; shape tight: pod limits set so that 15 of 16 nodes are full after the queue run"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    todo = [(int(v), False) for v in a.shapes.split(",") if v] + ([(a.tight_nodes, True)] if a.tight_nodes else [])
    for n, tight in todo:
        res["shapes"].append(run_shape(n, a, tight))
        with open(a.out, "w") as f:  # (after every shape: a later one may not fit the time given)
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in res["shapes"][-1].items() if not k.endswith("_us") or k.startswith("first")}),
              flush=True)


if __name__ == "__main__":
    main()
