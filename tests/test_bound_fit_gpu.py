"""Eviction fit (ksg_bound_fit / ksg_bound_fit_nodes / ksg_node_evictability /
ksg_bound_pod; Scheduler.bound_fit / bound_fit_nodes / node_evictability /
bound_pods): which bound pods their node would admit again, and where else
they fit.

No expected value comes from the calls under test.  The references are those of
test_bound_fit_model: the ORACLE as an experiment (the pod unbound, one cycle on
the document without it), a few lines of Python integers over the document,
and hand-written literals, pinned against each other there on the CPU; and, on
the GPU, the engine's existing route (removePod, ksg_cycle(commit=0),
ksg_filter_codes, addPod), code for code.

Kernel constants (csrc/snapshot_query.hip): a block of 256 threads owns kSqTile = 1024
nodes (4 per thread) and walks kSqPods = 32 bound pods over them.
"""
import copy
import ctypes

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import KsgError, _BoundFit, _NodeEvict
import test_bound_fit_model as m

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -4
TILE, POD_TILE = 1024, 32


def load(doc):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    return s


def full_name(pod):
    return (pod["metadata"].get("namespace") or "default") + "/" + pod["metadata"]["name"]


_refs = {}


def references(doc, n_subjects=None):
    """(verdicts, summary) of every subject; computed once for the shared, unchanging documents."""
    n = len(doc["pods"]) if n_subjects is None else n_subjects
    state = m.usage(doc)
    out = []
    for b in range(n):
        v = m.reference(doc, b, state)
        out.append((v, m.summary(doc, b, v)))
    return out


def shared_references(key, doc):
    if key not in _refs:
        _refs[key] = references(doc)
    return _refs[key]


def check_all(s, doc, refs=None, n_subjects=None, rows_of=()):
    """The structs of one call over every bound pod, the rows of rows_of and the node rows equal the Python
    reference.  The first n_subjects of doc["pods"] are the engine's bound pods, in its order; the rest is
    load the device rows hold (queue pods placed since the last encode)."""
    refs = references(doc, n_subjects) if refs is None else refs
    names = s.bound_pods()
    assert s.bound_count == len(names) == len(refs)
    got = s.bound_fit()
    assert len(got) == len(refs)
    for b, (v, f) in enumerate(refs):
        assert names[b] == (full_name(doc["pods"][b]), f.node), b
        assert (got[b].node, got[b].other_nodes, got[b].first_other) == (f.node, f.other_nodes, f.first_other), \
            (b, got[b], f)
        assert m.code_matches(doc, got[b].own_code, f.own), (b, hex(got[b].own_code), f.own)
        if b in rows_of:
            row = s.bound_fit_nodes(b)
            assert len(row) == len(v)
            bad = [(n, hex(c), w) for n, (c, w) in enumerate(zip(row, v)) if not m.code_matches(doc, c, w)]
            assert not bad, (b, bad[:4])
            assert row[f.node] == got[b].own_code
    assert s.node_evictability() == m.evictability(doc, [f for _, f in refs])
    return got


# ------------------------------------------------------------------ 1: the hand-built cluster
def test_hand_cluster():
    doc = m.hand_doc()
    s = load(doc)
    got = s.bound_fit()
    for b, want in enumerate(m.HAND):
        assert (got[b].node, got[b].other_nodes, got[b].first_other) == (want.node, want.other_nodes, want.first_other), b
        assert m.code_matches(doc, got[b].own_code, want.own), (b, hex(got[b].own_code))
        row = s.bound_fit_nodes(b)
        want_row = m.HAND_ROWS[b] if b in m.HAND_ROWS else m.oracle_verdicts(doc, b)
        assert all(m.code_matches(doc, c, w) for c, w in zip(row, want_row)), (b, [hex(c) for c in row])
        for n, code in m.HAND_CODES.get(b, {}).items():
            assert row[n] == code, (b, n, hex(row[n]))
        assert m.summary(doc, b, m.oracle_verdicts(doc, b))[2:] == (got[b].other_nodes, got[b].first_other)
    assert got[2].own_code == got[3].own_code == 0x04000002      # over-committed: Insufficient cpu
    assert got[4].own_code >> 24 == 2                             # TaintToleration's position
    assert got[11].own_code == 0 and got[12].own_code == 0x03000000
    assert got[14].own_code == m.NOT_EVALUATED and got[0].own_code == got[1].own_code == m.PASSED
    assert s.node_evictability() == m.HAND_EVICT
    assert s.bound_pods() == [(full_name(p), m.node_index(doc, p["spec"]["nodeName"])) for p in doc["pods"]]
    assert s.bound_fit(5, 9) == got[5:14] and s.bound_fit(17, 1) == got[17:]
    check_all(s, doc, rows_of=range(18))


def test_equivalence_with_the_event_and_cycle_route():
    """removePod, a cycle of the pod without spec.nodeName (commit = 0), ksg_filter_codes, addPod: the codes
    equal the row taken before the removal.  The over-committed node's pod, the untolerated taint (its detail
    is the engine's taint index), the zero-request pod, the pod-limit node, the gpu, the named affinity, the
    rejected pod, and the last node."""
    doc = m.hand_doc()
    s = load(doc)
    for name in ("o1a", "t2a", "z0", "l3a", "g4a", "f8", "r9", "big11", "a0"):
        pod = next(p for p in doc["pods"] if p["metadata"]["name"] == name)
        b = [n for n, _ in s.bound_pods()].index(full_name(pod))
        before = s.bound_fit_nodes(b)
        own = s.bound_fit(b, 1)[0]
        s.apply_events([{"op": "removePod", "name": name, "namespace": "default"}])
        q, r = s.cycle(m.unbound(pod), commit=False)
        codes = s.filter_codes(q)
        s.apply_events([{"op": "addPod", "pod": pod}])
        assert codes == before, (name, [hex(c) for c in codes], [hex(c) for c in before])
        assert r.feasible == own.other_nodes + (own.own_code == m.PASSED)
    # the bound pods are the document's again (the re-added ones moved to the end): the same verdicts
    by_name = {n: f for (n, _), f in zip(s.bound_pods(), s.bound_fit())}
    for b, p in enumerate(doc["pods"]):
        f = by_name[full_name(p)]
        assert (f.node, f.other_nodes, f.first_other) == (m.HAND[b].node, m.HAND[b].other_nodes, m.HAND[b].first_other)


# ------------------------------------------------------------------ 2: tile edges
@pytest.mark.parametrize("n_nodes", [TILE - 1, TILE, TILE + 1, 2 * TILE + 52])
def test_node_tile_edges(n_nodes):
    """1024 nodes a block: one short, exact, one node into a second block, two blocks and a ragged third; 33
    bound pods, so the second pod tile holds one.  Pods 0, 1, 2 live on node 0, the last node and node 1024."""
    doc = m.tile_doc(n_nodes, POD_TILE + 1)
    s = load(doc)
    refs = shared_references(("tile", n_nodes, POD_TILE + 1), doc)
    assert refs[0][1].node == 0 and refs[1][1].node == n_nodes - 1
    assert n_nodes <= TILE or refs[2][1].node == TILE
    got = check_all(s, doc, refs, rows_of={0, 1, 2, POD_TILE - 1, POD_TILE})
    assert s.bound_fit(3, POD_TILE - 2) == got[3:POD_TILE + 1]  # a sub-range from inside a tile into the next


@pytest.mark.parametrize("n_bound", [1, POD_TILE - 1, POD_TILE, POD_TILE + 1])
def test_pod_tile_edges(n_bound):
    """32 bound pods a block, over two node blocks (1025 nodes); sub-ranges start inside a tile."""
    doc = m.tile_doc(TILE + 1, n_bound)
    s = load(doc)
    got = check_all(s, doc, shared_references(("tile", TILE + 1, n_bound), doc), rows_of={0, n_bound - 1})
    if n_bound > 2:
        assert s.bound_fit(1, n_bound - 2) == got[1:n_bound - 1]
    assert s.bound_fit(n_bound - 1, 1) == got[n_bound - 1:]


# ------------------------------------------------------------------ 3: families
@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_families(family):
    doc = m.cfg2_doc() if family == "cfg2" else m.cfg3_doc()
    s = load(doc)
    refs = shared_references(family, doc)
    got = check_all(s, doc, refs, rows_of=set(m.sample_pods(doc)[0]))
    assert any(f.own_code != m.PASSED for f in got) and any(f.own_code == m.PASSED for f in got)


# ------------------------------------------------------------------ 4: the snapshot moves
def bind(doc, pod, node_index, name=None):
    p = copy.deepcopy(pod)
    p["spec"]["nodeName"] = doc["nodes"][node_index]["metadata"]["name"]
    if name:
        p["metadata"]["name"] = name
    return p


def test_snapshot_moves():
    base = m.cfg3_doc()
    doc = {"profile": base["profile"], "nodes": copy.deepcopy(base["nodes"]), "pods": list(base["pods"]),
           "queue": list(base["queue"])}
    subjects, load_only = list(doc["pods"]), []  # the engine's bound pods; what else the device rows hold

    def check(rows_of):
        doc["pods"] = subjects + load_only
        check_all(s, doc, n_subjects=len(subjects), rows_of=rows_of)

    s = load(doc)
    check({0, 5})
    # a queue run of 20 pods: load on their nodes, not subjects
    by_name = {full_name(p): p for p in doc["queue"]}
    s.schedule(0, 20)
    for q, r in enumerate(s.results(0, 20)):
        if r.status == 0:
            load_only.append(bind(doc, by_name[s.queue_pod(q)], r.selected))
    assert len(load_only) >= 10
    check({1, 6})
    # a cycle without commit, then Reserve; then Unreserve
    extra = g.pod_obj("extra-0", [g.req(700, 900 * g.Mi)])
    q, r = s.cycle(extra, commit=False)
    assert r.status == 0
    check({2})
    s.reserve(q, r.selected)
    load_only.append(bind(doc, extra, r.selected))
    check({3, 7})
    s.unreserve(q)
    load_only.pop()
    check({4})
    # events applied in place: allocatable lowered, a taint some node already carried, a bound pod arrives
    busy = m.node_index(doc, subjects[0]["spec"]["nodeName"])
    upd = copy.deepcopy(doc["nodes"][busy])
    upd["status"]["allocatable"].update(cpu="100m", pods="1")
    other = next(i for i, n in enumerate(doc["nodes"]) if i != busy and any(
        m.node_index(doc, p["spec"]["nodeName"]) == i for p in subjects))
    tainted = copy.deepcopy(doc["nodes"][other])
    tainted["spec"].setdefault("taints", []).append({"key": "drift", "value": "x", "effect": "NoSchedule"})
    added = bind(doc, g.pod_obj("evt-added", [g.req(1500, 3 * g.Gi)]), 8)
    s.apply_events([{"op": "updateNode", "node": upd}, {"op": "updateNode", "node": tainted},
                    {"op": "addPod", "pod": added}])
    doc["nodes"][busy], doc["nodes"][other] = upd, tainted
    subjects.append(added)
    check({0, len(subjects) - 1})
    # compact: the placed queue pods become bound pods, behind the others, in queue order
    s.compact()
    subjects += load_only
    del load_only[:]
    check({len(subjects) - 1})


# ------------------------------------------------------------------ 5: no side effects
def raw(s):
    n = s.bound_count
    arr = (_BoundFit * n)()
    assert s.L.ksg_bound_fit(s.h, 0, n, arr) == 0
    ev = (_NodeEvict * s.n_nodes)()
    assert s.L.ksg_node_evictability(s.h, ev, s.n_nodes) == 0
    return bytes(arr) + bytes(ev)


def test_no_side_effects():
    doc = m.cfg2_doc()
    n, nb = len(doc["queue"]), len(doc["pods"])
    a, b = load(doc), load(doc)
    a.schedule()
    b.bound_fit()
    assert raw(b) == raw(b)
    for q in range(n):  # bound-fit calls between the pods of b's run
        b.bound_fit((7 * q) % nb, min(40, nb - (7 * q) % nb))
        b.bound_fit_nodes((11 * q) % nb)
        if q % 6 == 0:
            b.node_evictability()
        b.schedule(q, 1)
    assert a.results() == b.results()
    assert a.node_requested() == b.node_requested()
    assert raw(a) == raw(b)
    assert raw(a) == raw(a)


# ------------------------------------------------------------------ 6: errors
def test_errors_leave_the_context_usable():
    doc = m.hand_doc()
    s = load(doc)
    s.bound_fit()  # (binds the argument types)
    s.bound_fit_nodes(0)
    s.node_evictability()
    s.bound_pods()
    before = (raw(s), s.bound_fit_nodes(13))
    out = (_BoundFit * 20)()
    row = (ctypes.c_uint32 * 64)()
    ev = (_NodeEvict * 16)()
    n, node = ctypes.c_size_t(), ctypes.c_int32()
    buf = ctypes.create_string_buffer(64)

    def same():
        assert (raw(s), s.bound_fit_nodes(13)) == before

    assert s.bound_count == 18
    assert s.L.ksg_bound_fit(s.h, 0, 3, None) == E_RANGE
    same()
    assert s.L.ksg_bound_fit(s.h, 16, 3, out) == E_RANGE
    assert s.L.ksg_bound_fit(s.h, 19, 0, out) == E_RANGE
    assert s.L.ksg_bound_fit(s.h, 0xFFFFFFFF, 2, out) == E_RANGE
    assert s.L.ksg_bound_fit_nodes(s.h, 18, row, 12) == E_RANGE
    same()
    assert s.L.ksg_bound_fit_nodes(s.h, 0, row, 11) == E_RANGE
    assert s.L.ksg_bound_fit_nodes(s.h, 0, row, 13) == E_RANGE
    assert s.L.ksg_bound_fit_nodes(s.h, 0, None, 12) == E_RANGE
    assert s.L.ksg_node_evictability(s.h, ev, 11) == E_RANGE
    assert s.L.ksg_node_evictability(s.h, ev, 13) == E_RANGE
    assert s.L.ksg_node_evictability(s.h, None, 12) == E_RANGE
    same()
    out[0].other_nodes = 77
    assert s.L.ksg_bound_fit(s.h, 18, 0, out) == 0 and s.L.ksg_bound_fit(s.h, 0, 0, out) == 0
    assert out[0].other_nodes == 77  # count == 0 writes nothing
    same()
    assert s.L.ksg_bound_pod(s.h, 18, buf, 64, ctypes.byref(n), ctypes.byref(node)) == E_RANGE
    assert s.L.ksg_bound_pod(s.h, 17, buf, 2, ctypes.byref(n), ctypes.byref(node)) == -5 and n.value == len("default/big11")
    assert s.L.ksg_bound_pod(s.h, 17, buf, 64, ctypes.byref(n), ctypes.byref(node)) == 0
    assert (buf.raw[:n.value].decode(), node.value) == ("default/big11", 11)
    same()
    s.schedule()  # the context goes on working
    assert sorted(r.status for r in s.results()) == [0, 0, 1]  # (no gpu is left for q-gpu)


def refused(doc, match, **kw):
    s = Scheduler(doc["profile"], **kw)
    s.load_cluster(doc)
    out = (_BoundFit * 1)()
    s.L.ksg_bound_fit.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_BoundFit)]
    assert s.L.ksg_bound_fit(s.h, 0, 1, out) == E_INVALID
    for call in (lambda: s.bound_fit(0, 1), lambda: s.bound_fit_nodes(0), s.node_evictability):
        with pytest.raises(KsgError, match=match):
            call()
    return s


def test_profiles_outside_the_closed_form():
    cfg4 = g.generate(4, n_nodes=40, n_existing=60, n_pods=8, n_zones=4)
    s = refused(cfg4, "PodTopologySpread")
    s.schedule()  # a queue run still works after the refusal
    assert len(s.results()) == 8
    nofit = dict(m.hand_doc())
    nofit["profile"] = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2)], 7)
    s = refused(nofit, "NodeResourcesFit")
    s.schedule()
    assert len(s.results()) == 3
    refused(m.cfg2_doc(), "sharded", shard_rank=0, shard_count=2)
