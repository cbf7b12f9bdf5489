"""Headroom (ksg_headroom / ksg_headroom_nodes / ksg_resource_name;
Scheduler.headroom / headroom_nodes / resource_names): how many more copies of a
queue pod fit, on which nodes, and which constraint runs out first.

No expected value comes from the calls under test.  The references are those of
test_headroom_model: the ORACLE as a filling experiment (K distinctly named
copies scheduled; every fill asserts that a copy was left over) and a few lines
of Python integers over the document, pinned there against the fill and against
hand-written literals.

Kernel constants (csrc/snapshot_query.hip): a block of 256 threads owns kSqTile = 1024
nodes (kSqNpt = 4 per thread) and walks kSqPods = 32 pods over them; several
node blocks per pod start at 1025 nodes and several pod tiles at 33 pods, so no
tile override exists.
"""
import copy
import ctypes

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import Headroom, KsgError, _Headroom
import test_headroom_model as m

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -4
TILE, POD_TILE = 1024, 32


def load(doc):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    return s


def check_all(s, doc, rows_of=None):
    """One batched call over the whole queue equals the Python reference pod by pod; the per-node rows of
    rows_of (default: every pod) equal it too and sum to the batched structs."""
    got = s.headroom()
    assert len(got) == len(doc["queue"])
    for q, pod in enumerate(doc["queue"]):
        hr, row = m.reference(doc, pod)
        assert got[q] == Headroom(*hr), (q, got[q], hr)
        assert sum(got[q].bound) == got[q].open_nodes
        if rows_of is None or q in rows_of:
            grow = s.headroom_nodes(q)
            assert grow == row, q
            assert (sum(grow), sum(1 for c in grow if c >= 1), max(grow, default=0)) == \
                (got[q].replicas, got[q].nodes, got[q].max_node)
    return got


# ------------------------------------------------------------------ 1: the hand-built cluster
def test_hand_cluster():
    doc = m.hand_doc()
    s = load(doc)
    assert s.resource_names() == ["cpu", "memory", "ephemeral-storage", m.GPU]
    got = s.headroom()
    for q in range(3):
        assert got[q] == Headroom(*m.HAND[q]), (q, got[q])
        assert s.headroom_nodes(q) == m.HAND_ROWS[q], q
        replicas, row = m.oracle_fill(doc, doc["queue"][q], m.HAND[q].replicas + 3)
        assert (replicas, row) == (got[q].replicas, s.headroom_nodes(q))
    assert s.headroom(1, 2) == got[1:]
    assert s.headroom(2, 1) == got[2:]
    check_all(s, doc)


# ------------------------------------------------------------------ 2: families
@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_families(family):
    doc = m.cfg2_doc() if family == "cfg2" else m.cfg3_doc()
    s = load(doc)
    got = check_all(s, doc)
    for q in m.sample_pods(doc):  # the oracle fill for every distinct request shape
        replicas, row = m.oracle_fill(doc, doc["queue"][q], got[q].replicas + 3)
        assert replicas == got[q].replicas and row == s.headroom_nodes(q), q


# ------------------------------------------------------------------ 3: tile edges
@pytest.mark.parametrize("n_nodes", [TILE - 1, TILE, TILE + 1, 2 * TILE + 52])
def test_node_tile_edges(n_nodes):
    """kSqTile = 1024 nodes a block: one node short, exact, one node into a second block, and two blocks
    plus a ragged third; POD_TILE + 1 pods, so the second pod tile holds one pod."""
    doc = m.tile_doc(n_nodes, POD_TILE + 1)
    s = load(doc)
    got = check_all(s, doc, rows_of={0, POD_TILE - 1, POD_TILE})
    replicas, row = m.oracle_fill(doc, doc["queue"][0], got[0].replicas + 3)
    assert replicas == got[0].replicas and row == s.headroom_nodes(0)


@pytest.mark.parametrize("n_pods", [1, POD_TILE - 1, POD_TILE, POD_TILE + 1])
def test_pod_tile_edges(n_pods):
    """kSqPods = 32 pods a block, over two node blocks (1025 nodes); sub-ranges start inside a tile."""
    doc = m.tile_doc(TILE + 1, n_pods)
    s = load(doc)
    got = check_all(s, doc, rows_of={0, n_pods - 1})
    if n_pods > 2:
        assert s.headroom(1, n_pods - 2) == got[1:n_pods - 1]
    assert s.headroom(n_pods - 1, 1) == got[n_pods - 1:]


# ------------------------------------------------------------------ 4: the snapshot moves
def bind(doc, pod, node_index, name=None):
    p = copy.deepcopy(pod)
    p["spec"]["nodeName"] = doc["nodes"][node_index]["metadata"]["name"]
    if name:
        p["metadata"]["name"] = name
    return p


def test_snapshot_moves():
    doc = copy.deepcopy(m.cfg2_doc())
    s = load(doc)
    check_all(s, doc, rows_of={0, 7})
    # a queue run of the first 20 pods
    s.schedule(0, 20)
    for q, r in enumerate(s.results(0, 20)):
        if r.status == 0:
            doc["pods"].append(bind(doc, doc["queue"][q], r.selected))
    check_all(s, doc, rows_of={0, 25})
    # a cycle without commit, then Reserve; then Unreserve
    extra = g.pod_obj("extra-0", [g.req(700, 900 * g.Mi)])
    q, r = s.cycle(extra, commit=False)
    assert r.status == 0
    doc["queue"].append(extra)
    check_all(s, doc, rows_of={q})
    s.reserve(q, r.selected)
    doc["pods"].append(bind(doc, extra, r.selected))
    check_all(s, doc, rows_of={q, 30})
    s.unreserve(q)
    doc["pods"].pop()
    check_all(s, doc, rows_of={q, 30})
    # events applied in place: a bound pod arrives, a node's allocatable changes
    added = bind(doc, g.pod_obj("evt-added", [g.req(1500, 3 * g.Gi)]), 5)
    upd = copy.deepcopy(doc["nodes"][9])
    upd["status"]["allocatable"].update(cpu="3", pods="4")
    s.apply_events([{"op": "addPod", "pod": added}, {"op": "updateNode", "node": upd}])
    doc["pods"].append(added)
    doc["nodes"][9] = upd
    check_all(s, doc, rows_of={q, 31})


# ------------------------------------------------------------------ 5: PreFilter cases
def test_prefilter_cases():
    doc = m.prefilter_doc()
    s = load(doc)
    got = check_all(s, doc)
    two, one, cordon, rejected, plain = got
    assert (two.replicas, two.nodes, two.open_nodes, two.max_node, two.best_node) == (3 + 6, 2, 2, 6, 38)
    assert s.headroom_nodes(0) == [3 if i == 13 else 6 if i == 38 else 0 for i in range(40)]
    assert (one.replicas, one.open_nodes, one.best_node) == (4, 1, 25)
    assert cordon.open_nodes == plain.open_nodes + 3 and cordon.replicas == plain.replicas + 3 * 8
    assert rejected == Headroom(0, 0, 0, 0, -1, (0,) * 9)
    assert s.headroom_nodes(3) == [0] * 40
    for q in (0, 1, 2, 4):
        replicas, row = m.oracle_fill(doc, doc["queue"][q], got[q].replicas + 3)
        assert replicas == got[q].replicas and row == s.headroom_nodes(q), q


# ------------------------------------------------------------------ 6: no side effects
def raw(s, first, count):
    arr = (_Headroom * count)()
    assert s.L.ksg_headroom(s.h, first, count, arr) == 0
    return bytes(arr)


def test_no_side_effects():
    doc = m.cfg2_doc()
    n = len(doc["queue"])
    a, b = load(doc), load(doc)
    a.schedule()
    b.headroom()
    assert raw(b, 0, n) == raw(b, 0, n)
    for q in range(n):  # headroom calls between the pods of b's run
        b.headroom(q, min(3, n - q))
        b.headroom_nodes(q)
        b.schedule(q, 1)
    assert a.results() == b.results()
    assert a.node_requested() == b.node_requested()
    assert raw(a, 0, n) == raw(b, 0, n)
    assert raw(a, 0, n) == raw(a, 0, n)


# ------------------------------------------------------------------ 7: errors
def test_errors_leave_the_context_usable():
    doc = m.hand_doc()
    s = load(doc)
    s.headroom()  # (binds the argument types)
    s.headroom_nodes(0)
    s.resource_names()
    before = (raw(s, 0, 3), s.headroom_nodes(1))
    out = (_Headroom * 4)()
    row = (ctypes.c_int32 * 64)()
    n = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(64)

    def same():
        assert (raw(s, 0, 3), s.headroom_nodes(1)) == before

    assert s.L.ksg_headroom(s.h, 0, 3, None) == E_RANGE
    same()
    assert s.L.ksg_headroom(s.h, 1, 3, out) == E_RANGE
    assert s.L.ksg_headroom(s.h, 4, 0, out) == E_RANGE
    assert s.L.ksg_headroom(s.h, 0xFFFFFFFF, 2, out) == E_RANGE
    assert s.L.ksg_headroom_nodes(s.h, 3, row, 40) == E_RANGE
    same()
    assert s.L.ksg_headroom_nodes(s.h, 0, row, 39) == E_RANGE
    assert s.L.ksg_headroom_nodes(s.h, 0, row, 41) == E_RANGE
    assert s.L.ksg_headroom_nodes(s.h, 0, None, 40) == E_RANGE
    same()
    out[0].replicas = 77
    assert s.L.ksg_headroom(s.h, 3, 0, out) == 0 and s.L.ksg_headroom(s.h, 0, 0, out) == 0
    assert out[0].replicas == 77  # count == 0 writes nothing
    same()
    assert s.L.ksg_resource_name(s.h, 4, buf, 64, ctypes.byref(n)) == E_RANGE
    assert s.L.ksg_resource_name(s.h, 3, buf, 2, ctypes.byref(n)) == -5 and n.value == len(m.GPU)
    assert s.L.ksg_resource_name(s.h, 3, buf, 64, ctypes.byref(n)) == 0 and buf.raw[:n.value].decode() == m.GPU
    same()


def refused(doc, match, **kw):
    s = Scheduler(doc["profile"], **kw)
    s.load_cluster(doc)
    out = (_Headroom * 1)()
    s.L.ksg_headroom.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_Headroom)]
    assert s.L.ksg_headroom(s.h, 0, 1, out) == E_INVALID
    with pytest.raises(KsgError, match=match):
        s.headroom(0, 1)
    with pytest.raises(KsgError, match=match):
        s.headroom_nodes(0)
    return s


def test_profiles_outside_the_closed_form():
    cfg4 = g.generate(4, n_nodes=40, n_existing=60, n_pods=8, n_zones=4)
    s = refused(cfg4, "PodTopologySpread")
    s.schedule()  # the context goes on working
    assert len(s.results()) == 8
    nofit = dict(m.hand_doc())
    nofit["profile"] = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2)], 7)
    refused(nofit, "NodeResourcesFit")
    refused(m.cfg2_doc(), "sharded", shard_rank=0, shard_count=2)
