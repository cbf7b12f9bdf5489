"""Eviction fit (ksg_bound_fit, include/ksg.h): the references the GPU tests use,
checked against each other on the CPU.

For bound pod b on node o a verdict per node: None (not evaluated: the PreFilter
rejected the pod, or the node is outside its PreFilterResult), "passed", or
(failing plugin, Fit's reasons) for the first Filter in profile order that fails,
with b taken off the snapshot and its spec.nodeName cleared.

1. The ORACLE as an experiment (oracle_verdicts): the document without b, its
   queue the one pod b without spec.nodeName; one cycle; the verdicts from the
   filter-result annotation, `feasible` from the result.
2. A few lines of Python integers over the document (reference): the static
   filters restated from the v1.Pod / v1.Node fields with NodeName skipped, and
   NodeResourcesFit over allocatable minus the other bound pods' requests.
3. Hand-written literals for a 12-node, 18-pod cluster (HAND, HAND_ROWS, HAND_EVICT).

No GPU and no engine call.  The document builders of the GPU tests live here, so
every shape they use is checked against the oracle on the CPU.
"""
import copy
import functools
import json
from collections import Counter, namedtuple

import pytest

from _oracle import Oracle
from ksg import generator as g
from test_headroom_model import columns, pod_requests, quantity, static_open

P = "kube-scheduler-simulator.sigs.k8s.io/"
PASSED, NOT_EVALUATED = 0xFFFFFFFF, 0xFFFFFFFE
FIT = "NodeResourcesFit"
STATIC = ("TaintToleration", "NodeAffinity", "NodeUnschedulable")  # (NodeName: not applied to a bound pod)
PODS = "Too many pods"
BoundFit = namedtuple("BoundFit", "node own other_nodes first_other")


def unbound(pod):
    p = copy.deepcopy(pod)
    del p["spec"]["nodeName"]
    return p


def node_index(doc, name):
    return next((i for i, n in enumerate(doc["nodes"]) if n["metadata"]["name"] == name), -1)


def prefilter_nodes(pod, plugins):
    """NodeAffinity's PreFilterResult: None (every node), or the set of node names; empty: rejected."""
    if "NodeAffinity" not in plugins:
        return None
    req = pod["spec"].get("affinity", {}).get("nodeAffinity", {}).get("requiredDuringSchedulingIgnoredDuringExecution")
    if req is None:
        return None
    names = set()
    for t in req["nodeSelectorTerms"]:
        mine = None
        for f in t.get("matchFields", []):
            if f["key"] == "metadata.name" and f["operator"] == "In":
                mine = set(f["values"]) if mine is None else mine & set(f["values"])
        if mine is None:
            return None  # a term without a node name: the terms name no node set
        names |= mine
    return names


def usage(doc):
    used, cnt = Counter(), Counter()
    for p in doc["pods"]:
        cnt[p["spec"]["nodeName"]] += 1
        for k, v in pod_requests(p).items():
            used[(p["spec"]["nodeName"], k)] += v
    return used, cnt


def reference(doc, b, state=None):
    """The verdict of bound pod b on every node of the document (state: usage(doc), shared by a caller's loop)."""
    plugins, cols = doc["profile"]["plugins"], columns(doc)
    assert FIT in plugins
    used, cnt = state or usage(doc)
    pod = doc["pods"][b]
    own, free_pod, want = pod["spec"]["nodeName"], unbound(pod), pod_requests(pod)
    zero = not any(v > 0 for v in want.values())
    names = prefilter_nodes(free_pod, plugins)
    out = []
    for node in doc["nodes"]:
        name, alloc = node["metadata"]["name"], node["status"]["allocatable"]
        if names is not None and name not in names:
            out.append(None)
            continue
        verdict = "passed"
        for plugin in plugins:
            if plugin in STATIC and not static_open(free_pod, node, (plugin,)):
                verdict = (plugin, frozenset())
            elif plugin == FIT:
                home = name == own
                why = set()
                if cnt[name] - (1 if home else 0) + 1 > quantity("pods", alloc["pods"]):
                    why.add(PODS)
                for col in ([] if zero else cols):
                    taken = used[(name, col)] - (want[col] if home else 0)
                    if want[col] > 0 and want[col] > quantity(col, alloc.get(col, 0)) - taken:
                        why.add("Insufficient " + col)
                if why:
                    verdict = (FIT, frozenset(why))
            if verdict != "passed":
                break
        out.append(verdict)
    return out


def summary(doc, b, verdicts):
    own = node_index(doc, doc["pods"][b]["spec"]["nodeName"])
    others = [i for i, v in enumerate(verdicts) if v == "passed" and i != own]
    return BoundFit(own, verdicts[own] if own >= 0 else None, len(others), others[0] if others else -1)


def oracle_verdicts(doc, b):
    """The same from one oracle cycle of b, unbound, on the document without b."""
    d = {"profile": doc["profile"], "nodes": doc["nodes"], "pods": doc["pods"][:b] + doc["pods"][b + 1:],
         "queue": [unbound(doc["pods"][b])]}
    o = Oracle(d)
    assert o.n_queue == 1
    o.schedule(record=3)
    _, feasible, _ = o.result(0)
    rows = json.loads(o.annotations(0)[P + "filter-result"])
    out = []
    for node in doc["nodes"]:
        row = rows.get(node["metadata"]["name"])
        if row is None:
            out.append(None)
            continue
        bad = [(k, v) for k, v in row.items() if v != "passed"]
        assert len(bad) <= 1
        if not bad:
            out.append("passed")
        else:
            k, v = bad[0]
            out.append((k, frozenset(v.split(", ")) if k == FIT else frozenset()))
    assert feasible == sum(1 for v in out if v == "passed")
    return out


def check_pod(doc, b, state=None):
    """The reference equals the oracle experiment for bound pod b; returns the verdicts."""
    ref = reference(doc, b, state)
    assert ref == oracle_verdicts(doc, b), b
    return ref


def code_matches(doc, got, verdict):
    """Does filter code `got` say `verdict`?  Position and, for NodeResourcesFit, the reason bits are
    compared; the detail of another plugin (TaintToleration's index into the engine's taint vocabulary) is
    the engine's own and is compared code for code with ksg_filter_codes by the GPU test."""
    plugins = doc["profile"]["plugins"]
    if verdict is None:
        return got == NOT_EVALUATED
    if verdict == "passed":
        return got == PASSED
    if got in (PASSED, NOT_EVALUATED):
        return False
    plugin, why = verdict
    if got >> 24 != plugins.index(plugin):
        return False
    if plugin != FIT:
        return True
    cols = columns(doc)
    bits = sum(1 if w == PODS else 1 << (1 + cols.index(w[len("Insufficient "):])) for w in why)
    return got & 0xFFFFFF == bits


def evictability(doc, fits):
    """(pods, stuck, drifted) per node from the per-pod summaries."""
    out = [[0, 0, 0] for _ in doc["nodes"]]
    for f in fits:
        if f.node < 0:
            continue
        out[f.node][0] += 1
        out[f.node][1] += f.other_nodes == 0
        out[f.node][2] += f.own != "passed"
    return [tuple(x) for x in out]


# ------------------------------------------------------------------ the hand-built cluster
GPU = "example.com/gpu"
GPU_TAINT = {"key": "dedicated", "value": "gpu", "effect": "NoSchedule"}
HAND_PLUGINS = [("NodeUnschedulable", 1), ("NodeName", 1), ("TaintToleration", 3), ("NodeAffinity", 2),
                (FIT, 1), ("NodeResourcesBalancedAllocation", 1)]


def named_affinity(*terms):
    """Required node affinity: one term per argument, a list of node names, each a matchFields requirement."""
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [v]} for v in t]} for t in terms]}}}


@functools.lru_cache(maxsize=None)
def hand_doc():
    """12 nodes, 18 bound pods; NodeUnschedulable, NodeName, TaintToleration, NodeAffinity, Fit, BA.
    What is left on each node (cpu milli, memory Gi, gpu, pod room), and who lives there:
      0  7000 31 - 6  a0 (1 cpu, 1Gi), z0 (no requests)
      1 -2000 30 - 6  over-committed: 4 cpu allocatable, o1a and o1b ask 3 each
      2  6000 30 - 6  gained the taint dedicated=gpu: t2a does not tolerate it, t2b does
      3  7000 30 - 0  exactly at its pod limit of 2: l3a, l3b (500m, 1Gi)
      4  6000 30 0 6  2 gpu, g4a and g4b hold one each
      5  7000 31 0 7  2 gpu, g5 holds both
      6  7000 31 - 7  cordoned since c6 arrived
      7  7000 31 - 7  lost its disk=ssd label; s7 selects it
      8 14000 60 - 7  f8 (2 cpu, 4Gi) names nodes 8 and 10 in two affinity terms
      9  7000 31 - 7  r9's one term names nodes 8 and 10 at once: its PreFilter rejects it
      10 15000 1 - 7  2Gi of memory, m10 holds one
      11 1000  8 - 6  p11 (2 cpu, 4Gi), big11 (5 cpu, 20Gi)"""
    ssd, big = {"disk": "ssd"}, 32 * g.Gi
    names = [f"node-{i:07d}" for i in range(12)]
    nodes = [g.node_obj(names[0], 8000, big, pods=8, labels=ssd),
             g.node_obj(names[1], 4000, big, pods=8, labels=ssd),
             g.node_obj(names[2], 8000, big, pods=8, labels=ssd, taints=[dict(GPU_TAINT)]),
             g.node_obj(names[3], 8000, big, pods=2, labels=ssd),
             g.node_obj(names[4], 8000, big, pods=8, labels=ssd, scalars={GPU: 2}),
             g.node_obj(names[5], 8000, big, pods=8, labels=ssd, scalars={GPU: 2}),
             g.node_obj(names[6], 8000, big, pods=8, labels=ssd, unschedulable=True),
             g.node_obj(names[7], 8000, big, pods=8),
             g.node_obj(names[8], 16000, 64 * g.Gi, pods=8, labels=ssd),
             g.node_obj(names[9], 8000, big, pods=8, labels=ssd),
             g.node_obj(names[10], 16000, 2 * g.Gi, pods=8, labels=ssd),
             g.node_obj(names[11], 8000, big, pods=8, labels=ssd)]
    one = [g.req(1000, g.Gi)]
    tol = [{"key": "dedicated", "operator": "Equal", "value": "gpu", "effect": "NoSchedule"}]

    def on(i, name, containers, **kw):
        return g.pod_obj(name, containers, node=names[i], **kw)

    pods = [on(0, "a0", one), on(0, "z0", [{}]),
            on(1, "o1a", [g.req(3000, g.Gi)]), on(1, "o1b", [g.req(3000, g.Gi)]),
            on(2, "t2a", one), on(2, "t2b", one, tolerations=tol),
            on(3, "l3a", [g.req(500, g.Gi)]), on(3, "l3b", [g.req(500, g.Gi)]),
            on(4, "g4a", [g.req(1000, g.Gi, {GPU: "1"})]), on(4, "g4b", [g.req(1000, g.Gi, {GPU: "1"})]),
            on(5, "g5", [g.req(1000, g.Gi, {GPU: "2"})]),
            on(6, "c6", one),
            on(7, "s7", one, nodeSelector=ssd),
            on(8, "f8", [g.req(2000, 4 * g.Gi)], affinity=named_affinity([names[8]], [names[10]])),
            on(9, "r9", one, affinity=named_affinity([names[8], names[10]])),
            on(10, "m10", one),
            on(11, "p11", [g.req(2000, 4 * g.Gi)]), on(11, "big11", [g.req(5000, 20 * g.Gi)])]
    queue = [g.pod_obj("q-small", [g.req(500, 512 * g.Mi)]), g.pod_obj("q-zero", [{}]),
             g.pod_obj("q-gpu", [g.req(500, 512 * g.Mi, {GPU: "1"})])]
    return {"profile": g.make_profile(HAND_PLUGINS, 7), "nodes": nodes, "pods": pods, "queue": queue}


def fit(*why):
    return (FIT, frozenset(why))


OK, CPU, MEM, NOGPU = "passed", "Insufficient cpu", "Insufficient memory", "Insufficient " + GPU
CORDON, TAINT, AFF = ("NodeUnschedulable", frozenset()), ("TaintToleration", frozenset()), ("NodeAffinity", frozenset())
# (node, own verdict, other nodes that pass, the lowest of them), in the order of hand_doc()["pods"]
HAND = [
    BoundFit(0, OK, 7, 4),          # a0: 4 5 7 8 9 10 11 (1: cpu, 2: taint, 3: pods, 6: cordon)
    BoundFit(0, OK, 8, 1),          # z0: the room alone, so the over-committed node 1 too
    BoundFit(1, fit(CPU), 7, 0),    # o1a: -2000 + 3000 < 3000 at home; 0 4 5 7 8 9 10 (11: 1000 < 3000)
    BoundFit(1, fit(CPU), 7, 0),    # o1b
    BoundFit(2, TAINT, 8, 0),       # t2a: 0 4 5 7 8 9 10 11
    BoundFit(2, OK, 8, 0),          # t2b
    BoundFit(3, OK, 8, 0),          # l3a: at home the count drops to 1 of 2; 0 4 5 7 8 9 10 11
    BoundFit(3, OK, 8, 0),          # l3b
    BoundFit(4, OK, 0, -1),         # g4a: no other node has a gpu left
    BoundFit(4, OK, 0, -1),         # g4b
    BoundFit(5, OK, 0, -1),         # g5
    BoundFit(6, CORDON, 8, 0),      # c6: 0 4 5 7 8 9 10 11
    BoundFit(7, AFF, 7, 0),         # s7: 0 4 5 8 9 10 11 (7 has no label)
    BoundFit(8, OK, 0, -1),         # f8: node 10 has 1Gi for its 4Gi
    BoundFit(9, None, 0, -1),       # r9: rejected
    BoundFit(10, OK, 7, 0),         # m10: 0 4 5 7 8 9 11
    BoundFit(11, OK, 6, 0),         # p11: 0 4 5 7 8 9 (10: memory)
    BoundFit(11, OK, 6, 0),         # big11: 0 4 5 7 8 9
]
HAND_ROWS = {  # whole rows of four pods, by bound index
    2: [OK, fit(CPU), TAINT, fit(PODS), OK, OK, CORDON, OK, OK, OK, OK, fit(CPU)],
    8: [fit(NOGPU), fit(CPU, NOGPU), TAINT, fit(PODS, NOGPU), OK, fit(NOGPU), CORDON, fit(NOGPU), fit(NOGPU),
        fit(NOGPU), fit(NOGPU), fit(NOGPU)],
    13: [None] * 8 + [OK, None, fit(MEM), None],
    14: [None] * 12,
}
# (pods, stuck, drifted) per node; r9's own node never evaluated it: drifted
HAND_EVICT = [(2, 0, 0), (2, 0, 2), (2, 0, 1), (2, 0, 0), (2, 2, 0), (1, 1, 0), (1, 0, 1), (1, 0, 1), (1, 1, 0),
              (1, 1, 1), (1, 0, 0), (2, 0, 0)]
# filter codes of the same rows: (position << 24) | detail; NodeResourcesFit is position 4, its detail
# bit 0 the pod limit and bit 1 + r column r of cpu, memory, ephemeral-storage, example.com/gpu;
# NodeUnschedulable is position 0 without detail.  (TaintToleration's detail is an engine index: no literal.)
HAND_CODES = {
    2: {0: PASSED, 1: 0x04000002, 3: 0x04000001, 6: 0x00000000, 11: 0x04000002},
    8: {0: 0x04000010, 1: 0x04000012, 3: 0x04000011, 4: PASSED, 5: 0x04000010, 6: 0x00000000},
    13: {0: NOT_EVALUATED, 8: PASSED, 10: 0x04000004},
}


def test_hand_literals():
    doc = hand_doc()
    assert columns(doc) == ["cpu", "memory", "ephemeral-storage", GPU]
    assert len(doc["nodes"]) == 12 and len(doc["pods"]) == len(HAND) == 18
    fits = []
    for b in range(len(doc["pods"])):
        v = reference(doc, b)
        fits.append(summary(doc, b, v))
        assert fits[-1] == HAND[b], (b, fits[-1])
        if b in HAND_ROWS:
            assert v == HAND_ROWS[b], b
        for n, code in HAND_CODES.get(b, {}).items():
            assert code_matches(doc, code, v[n]), (b, n)
    assert evictability(doc, fits) == HAND_EVICT
    assert not code_matches(doc, 0x04000003, fit(CPU)) and not code_matches(doc, PASSED, None)
    assert not code_matches(doc, 0x03000000, TAINT) and code_matches(doc, 0x02000005, TAINT)


def test_hand_oracle_experiment():
    doc = hand_doc()
    for b in range(len(doc["pods"])):
        v = oracle_verdicts(doc, b)
        assert summary(doc, b, v) == HAND[b], b
        if b in HAND_ROWS:
            assert v == HAND_ROWS[b], b
        assert v == reference(doc, b), b


# ------------------------------------------------------------------ generated clusters
def family_doc(cfg, n_nodes, n_bound, n_queue=24, seed=None):
    """A cfg2- / cfg3-shaped generated cluster whose first n_bound queue pods the oracle has placed (they
    become bound pods behind the generator's own), and which then drifted: pod limits of 2..5 were set
    before the placement; afterwards every 7th node gains a taint, every 11th is cordoned, every 5th loses
    60% of its cpu, every 9th has its pod limit cut to 1, and every 13th loses its labels (cfg3: node
    selectors stop matching)."""
    doc = g.generate(cfg, n_nodes=n_nodes, n_pods=n_bound + n_queue, **({} if seed is None else {"seed": seed}))
    for i, n in enumerate(doc["nodes"]):
        for k in ("allocatable", "capacity"):
            n["status"][k]["pods"] = str(2 + i % 4)
    o = Oracle(doc)
    order = o.ordered_queue(doc)
    o.schedule(n_bound, record=0)
    placed = []
    for q in range(n_bound):
        sel, _, st = o.result(q)
        if st == 0 and sel >= 0:
            p = copy.deepcopy(order[q])
            p["spec"]["nodeName"] = doc["nodes"][sel]["metadata"]["name"]
            placed.append(p)
    doc = {"profile": doc["profile"], "nodes": copy.deepcopy(doc["nodes"]), "pods": doc["pods"] + placed,
           "queue": order[n_bound:]}
    for i, n in enumerate(doc["nodes"]):
        if i % 7 == 3:
            n["spec"].setdefault("taints", []).append({"key": "drift", "value": "x", "effect": "NoSchedule"})
        if i % 11 == 5:
            n["spec"]["unschedulable"] = True
        if i % 5 == 1:
            for k in ("allocatable", "capacity"):
                n["status"][k]["cpu"] = f"{quantity('cpu', n['status'][k]['cpu']) * 4 // 10}m"
        if i % 9 == 4:
            for k in ("allocatable", "capacity"):
                n["status"][k]["pods"] = "1"
        if i % 13 == 2:
            n["metadata"]["labels"] = {g.HOSTNAME: n["metadata"]["name"]}
    return doc


@functools.lru_cache(maxsize=None)
def cfg2_doc():
    return family_doc(2, 200, 260)


@functools.lru_cache(maxsize=None)
def cfg3_doc():
    return family_doc(3, 240, 200)


@functools.lru_cache(maxsize=None)
def tile_doc(n_nodes, n_bound):
    """The tile-edge clusters of the GPU test: cfg3-shaped nodes at a node count beside the kernel's node
    tile, with n_bound hand-placed bound pods whose own nodes include the first node, index 1024 (the first
    of a second block) where it exists, and the last, ragged node."""
    doc = g.generate(3, n_nodes=n_nodes, n_pods=n_bound + 4, seed=4321 + n_nodes)
    nodes = doc["nodes"]
    want = [0, n_nodes - 1] + ([1024] if n_nodes > 1024 else []) + [n_nodes // 2]
    pods = []
    for j in range(n_bound):
        p = copy.deepcopy(doc["queue"][j])
        p["spec"]["nodeName"] = nodes[want[j] if j < len(want) else (j * 37) % n_nodes]["metadata"]["name"]
        pods.append(p)
    return {"profile": doc["profile"], "nodes": nodes, "pods": pods, "queue": doc["queue"][n_bound:]}


def shape_of(doc, b, verdicts):
    """(request shape, toleration and affinity shape, own-node kind) of bound pod b."""
    pod = doc["pods"][b]
    spec = pod["spec"]
    na = spec.get("affinity", {}).get("nodeAffinity", {})
    own = summary(doc, b, verdicts).own
    return (tuple(sorted(k for k, v in pod_requests(pod).items() if v > 0)), len(spec["containers"]),
            bool(spec.get("tolerations")), bool(spec.get("nodeSelector")),
            "requiredDuringSchedulingIgnoredDuringExecution" in na, own if own in (None, "passed") else own[0])


def sample_pods(doc):
    """The first bound pod of every distinct shape, with the references of all of them."""
    state = usage(doc)
    seen, out, refs = set(), [], []
    for b in range(len(doc["pods"])):
        refs.append(reference(doc, b, state))
        s = shape_of(doc, b, refs[-1])
        if s not in seen:
            seen.add(s)
            out.append(b)
    return out, refs


@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_generated_families(family):
    doc = cfg2_doc() if family == "cfg2" else cfg3_doc()
    sample, refs = sample_pods(doc)
    owns = {summary(doc, b, refs[b]).own for b in range(len(doc["pods"]))}
    assert "passed" in owns and any(o not in (None, "passed") and o[0] == FIT for o in owns)
    if family == "cfg3":
        assert any(o not in (None, "passed") and o[0] == "TaintToleration" for o in owns)
    assert len(sample) >= 4
    for b in sample:
        assert refs[b] == oracle_verdicts(doc, b), b


@pytest.mark.parametrize("n_nodes,n_bound", [(1023, 33), (1024, 33), (1025, 33), (2100, 33), (1025, 1), (1025, 31),
                                             (1025, 32)])
def test_tile_shapes(n_nodes, n_bound):
    """The tile-edge builders: the pods on the first, the last and (where it exists) node 1024 against the oracle."""
    doc = tile_doc(n_nodes, n_bound)
    assert len(doc["pods"]) == n_bound
    state = usage(doc)
    for b in range(min(n_bound, 3)):
        check_pod(doc, b, state)
