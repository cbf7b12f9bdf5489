"""Scale-up simulation (ksg_scale_up / ksg_scale_up_plan, include/ksg.h): the
references the GPU tests use, checked against each other on the CPU.

A list of queue pods, in the caller's order, is packed onto fresh nodes shaped
like a template node: a pod that a node of this shape never admits is closed; an
open pod goes to the lowest opened bin with room, else opens the next bin, unless
an empty fresh node does not admit it (too big) or the cap is reached (over cap).
A fresh node starts with the template's DaemonSet-owned and mirror pods.

1. The model (pack): a few lines of Python first fit over
   test_headroom_model.pod_requests, test_bound_fit_model's static verdicts
   (static_open with its STATIC plugins, prefilter_nodes) and test_drain_model.stays.
2. Hand-written literals for a 6-template, 13-pod cluster (HAND, HAND_PLANS).
3. The ORACLE as an experiment (oracle_plan): a document of clones of the
   template, each with the base pods; one oracle cycle per listed pod; the pod is
   bound to the lowest feasible clone before the next is judged.

No GPU and no engine call.  The document builders of the GPU tests live here.
"""
import copy
import functools
from collections import namedtuple

import pytest

from ksg import generator as g
from test_headroom_model import columns, pod_requests, quantity, static_open
import test_bound_fit_model as bf
import test_drain_model as dm

ScaleUp = namedtuple("ScaleUp", "nodes packed closed too_big over_cap first_unpacked base_pods")
SCALE_MAX = 1024
CLOSED, TOO_BIG, OVER_CAP = -1, -2, -3
GPU = bf.GPU


def is_open(doc, pod, node):
    """A node of this shape may admit the pod: no PreFilterResult node set (and no rejection), no
    spec.nodeName under NodeName, and the static Filters of the eviction fit pass on the template."""
    plugins = doc["profile"]["plugins"]
    if bf.prefilter_nodes(pod, plugins) is not None:
        return False
    if "NodeName" in plugins and pod["spec"].get("nodeName"):
        return False
    return static_open(pod, node, tuple(p for p in bf.STATIC if p in plugins))


def base_pods(doc, t):
    name = doc["nodes"][t]["metadata"]["name"]
    return [p for p in doc["pods"] if p["spec"]["nodeName"] == name and dm.stays(p)]


def empty_node(doc, t):
    """(free per column, pod room) of a fresh node of template t, and its base pod count."""
    cols, alloc, base = columns(doc), doc["nodes"][t]["status"]["allocatable"], base_pods(doc, t)
    free = {c: quantity(c, alloc.get(c, 0)) - sum(pod_requests(p)[c] for p in base) for c in cols}
    return free, quantity("pods", alloc["pods"]) - len(base), len(base)


def admits(free, room, want):
    if room < 1:
        return False
    if not any(v > 0 for v in want.values()):
        return True
    return all(v <= free[c] for c, v in want.items() if v > 0)


def pack(doc, pods, t, max_nodes=SCALE_MAX):
    """(ScaleUp, plan) of the queue positions `pods`, in this order, on template t."""
    free0, room0, n_base = empty_node(doc, t)
    bins, plan = [], []
    for q in pods:
        pod = doc["queue"][q]
        want = pod_requests(pod)
        if not is_open(doc, pod, doc["nodes"][t]):
            plan.append(CLOSED)
            continue
        j = next((j for j, (free, room) in enumerate(bins) if admits(free, room[0], want)), None)
        if j is None:
            if not admits(free0, room0, want):
                plan.append(TOO_BIG)
                continue
            if len(bins) == max_nodes:
                plan.append(OVER_CAP)
                continue
            j = len(bins)
            bins.append((dict(free0), [room0]))
        for c, v in want.items():
            bins[j][0][c] -= v
        bins[j][1][0] -= 1
        plan.append(j)
    out = [i for i, b in enumerate(plan) if b < 0]
    return ScaleUp(len(bins), sum(b >= 0 for b in plan), plan.count(CLOSED), plan.count(TOO_BIG), plan.count(OVER_CAP),
                   out[0] if out else -1, n_base), plan


def satisfied(s, n_pods):
    return s.packed == n_pods


def clone_doc(doc, t, k, queue=()):
    """k clones of template t, clone-0000.. in index order, its labels, taints and flags verbatim, each with
    copies of the base pods; no other node and no other pod."""
    nodes, pods = [], []
    for i in range(k):
        n = copy.deepcopy(doc["nodes"][t])
        n["metadata"]["name"] = f"clone-{i:04d}"
        nodes.append(n)
        for p in base_pods(doc, t):
            p = copy.deepcopy(p)
            p["metadata"]["name"] += f"-c{i}"
            p["spec"]["nodeName"] = n["metadata"]["name"]
            pods.append(p)
    return {"profile": doc["profile"], "nodes": nodes, "pods": pods, "queue": list(queue)}


def replica(doc, q, i):
    """Queue pod q as the i-th entry of a list: its own name (an index listed twice is two replicas)."""
    p = copy.deepcopy(doc["queue"][q])
    p["metadata"]["name"] += f"-i{i}"
    return p


def oracle_plan(doc, pods, t, max_nodes):
    """The same plan from oracle cycles on max_nodes clones: before entry i the earlier entries are bound to
    their clones; entry i runs one cycle; the lowest feasible clone is its bin.  Without one: closed when a
    clone's verdict is not NodeResourcesFit's (every clone gives the same static verdict); too big when an
    empty clone (one beyond the opened, or a document of one clone) refuses it; else over the cap."""
    d = clone_doc(doc, t, max_nodes)
    plan, opened = [], 0
    for i, q in enumerate(pods):
        pod = replica(doc, q, i)
        pod["spec"]["nodeName"] = "none"  # (oracle_verdicts unbinds its subject)
        verdicts = bf.oracle_verdicts(dict(d, pods=d["pods"] + [pod]), len(d["pods"]))
        dest = next((n for n, v in enumerate(verdicts) if v == "passed"), -1)
        if dest >= 0:
            assert dest <= opened
            opened = max(opened, dest + 1)
            pod["spec"]["nodeName"] = d["nodes"][dest]["metadata"]["name"]
            d["pods"].append(pod)
            plan.append(dest)
        elif all(v is None or v[0] != bf.FIT for v in verdicts):
            plan.append(CLOSED)
        else:
            assert all(v is not None and v[0] == bf.FIT for v in verdicts)
            if opened == max_nodes:
                e = clone_doc(doc, t, 1)
                verdicts = bf.oracle_verdicts(dict(e, pods=e["pods"] + [pod]), len(e["pods"]))
            plan.append(OVER_CAP if opened == max_nodes and verdicts[0] == "passed" else TOO_BIG)
    return plan


# ------------------------------------------------------------------ the hand-built cluster
PLAIN, TAINTED, GPUS, LIMIT2, BASE, CORDONED = range(6)


@functools.lru_cache(maxsize=None)
def hand_doc():
    """6 templates; the profile of test_bound_fit_model's hand cluster (NodeName included).
      0  plain      4000m 8Gi, 8 pods
      1  tainted    dedicated=gpu:NoSchedule: only `tol` is open
      2  gpu        as 0 with 2 example.com/gpu
      3  limit2     8000m 16Gi, 2 pods
      4  base       4000m 8Gi, 5 pods; bound there: ds4 (DaemonSet, 500m 1Gi), mir4 (mirror, 500m 1Gi) and
                    app4 (2000m 2Gi, does not count): a fresh node has 3000m 6Gi and room for 3
      5  cordoned   no pod tolerates it
    13 queue pods, all of one priority, listed by LIST (14 entries: small-a twice):
      big 3000m 2Gi; med-a, med-b 2000m 2Gi; small-a, small-b 1000m 1Gi; zero (no requests); huge 16000m (too
      big everywhere); named (required affinity on metadata.name = node 0: a PreFilterResult, closed);
      gpu1, gpu2 1000m 1Gi and 1 / 2 gpus; tol 1000m 1Gi, tolerates the taint; mem 500m 5Gi; tiny 500m 512Mi"""
    names = [f"node-{i:07d}" for i in range(6)]
    nodes = [g.node_obj(names[0], 4000, 8 * g.Gi, pods=8),
             g.node_obj(names[1], 4000, 8 * g.Gi, pods=8, taints=[dict(bf.GPU_TAINT)]),
             g.node_obj(names[2], 4000, 8 * g.Gi, pods=8, scalars={GPU: 2}),
             g.node_obj(names[3], 8000, 16 * g.Gi, pods=2),
             g.node_obj(names[4], 4000, 8 * g.Gi, pods=5),
             g.node_obj(names[5], 4000, 8 * g.Gi, pods=8, unschedulable=True)]
    pods = [dm.daemon_owned(g.pod_obj("ds4", [g.req(500, g.Gi)], node=names[4])),
            dm.mirror(g.pod_obj("mir4", [g.req(500, g.Gi)], node=names[4])),
            g.pod_obj("app4", [g.req(2000, 2 * g.Gi)], node=names[4])]
    tol = [{"key": "dedicated", "operator": "Equal", "value": "gpu", "effect": "NoSchedule"}]
    one = [g.req(1000, g.Gi)]
    queue = [g.pod_obj("big", [g.req(3000, 2 * g.Gi)]),
             g.pod_obj("med-a", [g.req(2000, 2 * g.Gi)]), g.pod_obj("med-b", [g.req(2000, 2 * g.Gi)]),
             g.pod_obj("small-a", one), g.pod_obj("small-b", one),
             g.pod_obj("zero", [{}]),
             g.pod_obj("huge", [g.req(16000, g.Gi)]),
             g.pod_obj("named", [g.req(500, 512 * g.Mi)], affinity=bf.named_affinity([names[0]])),
             g.pod_obj("gpu1", [g.req(1000, g.Gi, {GPU: "1"})]), g.pod_obj("gpu2", [g.req(1000, g.Gi, {GPU: "2"})]),
             g.pod_obj("tol", one, tolerations=tol),
             g.pod_obj("mem", [g.req(500, 5 * g.Gi)]),
             g.pod_obj("tiny", [g.req(500, 512 * g.Mi)])]
    return {"profile": g.make_profile(bf.HAND_PLUGINS, 7), "nodes": nodes, "pods": pods, "queue": queue}


LIST = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 3]
# per template: ScaleUp(nodes, packed, closed, too_big, over_cap, first_unpacked, base_pods) and the bins
HAND = [
    ScaleUp(4, 10, 1, 3, 0, 6, 0),   # the gpu pods are too big for a node without the column
    ScaleUp(1, 1, 13, 0, 0, 0, 0),   # tol alone
    ScaleUp(4, 12, 1, 1, 0, 6, 0),   # gpu2 opens a bin: bin 2 has one gpu left; mem fills bin 2's 5Gi exactly
    ScaleUp(5, 10, 1, 3, 0, 6, 0),   # two pods a bin, whatever they ask
    ScaleUp(5, 10, 1, 3, 0, 6, 2),   # big fills 3000m alone; zero takes bin 0's pod room
    ScaleUp(0, 0, 14, 0, 0, 0, 0),
]
HAND_PLANS = [
    [0, 1, 1, 0, 2, 0, -2, -1, -2, -2, 2, 2, 2, 3],
    [-1] * 10 + [0] + [-1] * 3,
    [0, 1, 1, 0, 2, 0, -2, -1, 2, 3, 2, 2, 3, 3],
    [0, 0, 1, 1, 2, 2, -2, -1, -2, -2, 3, 3, 4, 4],
    [0, 1, 2, 1, 2, 0, -2, -1, -2, -2, 3, 3, 4, 4],
    [-1] * 14,
]
# template 0 under max_nodes = 2: what would open bin 2 or 3 is over the cap; huge stays too big
CAP2 = ScaleUp(2, 5, 1, 3, 5, 4, 0)
CAP2_PLAN = [0, 1, 1, 0, -3, 0, -2, -1, -2, -2, -3, -3, -3, -3]


def test_hand_literals():
    doc = hand_doc()
    assert columns(doc) == ["cpu", "memory", "ephemeral-storage", GPU]
    assert len(doc["nodes"]) == len(HAND) == len(HAND_PLANS) == 6 and len(doc["queue"]) == 13 and len(LIST) == 14
    for t in range(6):
        s, plan = pack(doc, LIST, t)
        assert s == HAND[t], (t, s)
        assert plan == HAND_PLANS[t], (t, plan)
        assert not satisfied(s, len(LIST))
    assert pack(doc, LIST, PLAIN, 2) == (CAP2, CAP2_PLAN)
    # a list the plain template satisfies; an empty list; the base is counted either way
    s, plan = pack(doc, [1, 2, 3, 4, 5], PLAIN)
    assert s == ScaleUp(2, 5, 0, 0, 0, -1, 0) and plan == [0, 0, 1, 1, 0] and satisfied(s, 5)
    assert pack(doc, [], BASE) == (ScaleUp(0, 0, 0, 0, 0, -1, 2), [])
    # without its base the fifth template would pack like the plain one with 5 pods a node
    assert empty_node(doc, BASE)[:2] == ({"cpu": 3000, "memory": 6 * g.Gi, "ephemeral-storage": 0, GPU: 0}, 3)
    # the order is the caller's: the same pods smallest first need another node count on the limit-2 template
    assert pack(doc, [12, 11, 5, 0], LIMIT2)[1] == [0, 0, 1, 1] and pack(doc, [0, 12, 11, 5], BASE)[1] == [0, 1, 1, 0]


@pytest.mark.parametrize("t", range(6))
def test_hand_oracle_experiment(t):
    doc = hand_doc()
    assert oracle_plan(doc, LIST, t, 6) == HAND_PLANS[t]


def test_cap_oracle_experiment():
    doc = hand_doc()
    assert oracle_plan(doc, LIST, PLAIN, 2) == CAP2_PLAN
    assert oracle_plan(doc, [0, 12, 11, 5], BASE, 2) == [0, 1, 1, 0]


# ------------------------------------------------------------------ bin edges (closed forms, no oracle)
def limit1_doc(n_pods):
    """One template with a pod limit of 1: every pod opens a bin."""
    nodes = [g.node_obj("node-0000000", 64000, 64 * g.Gi, pods=1)]
    queue = [g.pod_obj(f"p{i:04d}", [g.req(100, 64 * g.Mi)]) for i in range(n_pods)]
    return {"profile": g.make_profile(bf.HAND_PLUGINS, 7), "nodes": nodes, "pods": [], "queue": queue}


def backfill_doc(n_large=300, n_small=301):
    """A template of 1000m; n_large pods of 900m, then n_small pods of 100m: each large pod opens a bin and
    leaves room for exactly one small pod, so the small pods land in bins 0.. in order and the one after the
    last large bin opens a new one."""
    nodes = [g.node_obj("node-0000000", 1000, 64 * g.Gi, pods=8)]
    queue = ([g.pod_obj(f"l{i:04d}", [g.req(900, 64 * g.Mi)]) for i in range(n_large)] +
             [g.pod_obj(f"s{i:04d}", [g.req(100, 64 * g.Mi)]) for i in range(n_small)])
    return {"profile": g.make_profile(bf.HAND_PLUGINS, 7), "nodes": nodes, "pods": [], "queue": queue}


def test_bin_edge_shapes():
    for n in (63, 65, 257):
        s, plan = pack(limit1_doc(n), range(n), 0)
        assert s == ScaleUp(n, n, 0, 0, 0, -1, 0) and plan == list(range(n))
    s, plan = pack(limit1_doc(5), range(5), 0, 4)
    assert s == ScaleUp(4, 4, 0, 0, 1, 4, 0) and plan == [0, 1, 2, 3, -3]
    s, plan = pack(backfill_doc(), range(601), 0)
    assert s == ScaleUp(301, 601, 0, 0, 0, -1, 0) and plan == list(range(300)) + list(range(300)) + [300]
    doc = backfill_doc(3, 4)
    assert oracle_plan(doc, range(7), 0, 5) == pack(doc, range(7), 0)[1] == [0, 1, 2, 0, 1, 2, 3]


# ------------------------------------------------------------------ a generated cluster
@functools.lru_cache(maxsize=None)
def many_doc():
    """300 cfg3-shaped nodes (test_drain_model.family_doc: DaemonSet-owned and mirror pods among the bound,
    drifted taints, cordons, cuts) with a queue of 200 pods."""
    return dm.family_doc(3, 300, per_node=2, n_queue=200)


@functools.lru_cache(maxsize=None)
def many_list():
    """64 queue positions: cfg3's pods carry node selectors and tolerations, so no pod is open on every
    template; the list is taken from the pods open on the template that is open for most of them (the lowest
    such), largest cpu request first (the autoscaler's order), ties by position.  That template can be
    satisfied; every other one meets closed pods."""
    doc = many_doc()
    n = len(doc["queue"])
    is_op = [[is_open(doc, p, node) for p in doc["queue"]] for node in doc["nodes"]]
    best = max(range(len(doc["nodes"])), key=lambda t: (sum(is_op[t]), -t))
    return tuple(sorted((q for q in range(n) if is_op[best][q]),
                        key=lambda q: (-pod_requests(doc["queue"][q])["cpu"], q))[:64])


@functools.lru_cache(maxsize=None)
def many_model():
    doc = many_doc()
    pods = many_list()
    return [pack(doc, pods, t) for t in range(len(doc["nodes"]))]


def test_generated_cluster():
    doc, model = many_doc(), many_model()
    pods = many_list()
    assert len(doc["nodes"]) == 300 and len(pods) == 64
    ss = [s for s, _ in model]
    assert any(s.closed for s in ss) and any(s.too_big for s in ss) and any(s.base_pods for s in ss)
    assert any(satisfied(s, 64) and s.nodes >= 2 for s in ss)
    # two templates against the oracle: the first satisfied one and the first with pods of every kind left out
    want = [next(t for t, s in enumerate(ss) if satisfied(s, 64) and s.nodes >= 2),
            next(t for t, s in enumerate(ss) if s.closed and s.packed and s.base_pods)]
    for t in want:
        assert oracle_plan(doc, pods, t, ss[t].nodes + 1) == model[t][1], t
