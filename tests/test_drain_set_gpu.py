"""Set drain (ksg_drain_sets / ksg_drain_prefixes / ksg_drain_set_plan;
Scheduler.drain_sets / drain_prefixes / drain_set_plan): several nodes removed
together, simulated on the device, one block per set.

No expected value comes from the calls under test.  The references are those of
test_drain_set_model -- hand-written literals, a few lines of Python over the
eviction fit's model, and the ORACLE as an experiment, pinned against each other
there on the CPU -- and, on the GPU, the engine's existing routes: ksg_drain and
ksg_drain_plan (the old kernel against the new on one-node sets), and per subject
removePod, ksg_cycle(commit=0), ksg_filter_codes, addPod on the destination.

Kernel constants: one block of 256 threads per set walks the nodes in tiles of
T = kSqTile = 1024; the overlay is a hash table of 2 x KSG_DRAIN_MAX slots, home
slot = local node index & (slots - 1); a set holds at most 128 nodes.
"""
import copy
import ctypes

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import KsgError, _Drain, _DrainMove, _DrainSet
import test_bound_fit_model as bf
import test_drain_model as dm
import test_drain_set_model as m

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE, E_NOBUF = -1, -4, -5
PASSED = bf.PASSED
T = m.TILE
U32P = ctypes.POINTER(ctypes.c_uint32)


def load(doc):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    return s


def full_name(pod):
    return (pod["metadata"].get("namespace") or "default") + "/" + pod["metadata"]["name"]


def check_sets(s, doc, sets, model=None, n_subjects=None, cap=dm.DRAIN_MAX):
    """One ksg_drain_sets over `sets` and every set's plan equal the model."""
    if model is None:
        state = bf.usage(doc)
        model = [m.simulate_set(doc, nodes, cap, n_subjects, state) for nodes in sets]
    got = s.drain_sets(sets)
    assert len(got) == len(sets)
    for i, (d, plan) in enumerate(model):
        assert tuple(got[i]) == tuple(d), (sets[i], got[i], d)
        assert got[i].removable == m.removable(d)
        assert s.drain_set_plan(sets[i]) == plan, sets[i]
    return got


# ------------------------------------------------------------------ 1: the competition cluster
def test_competition_cluster():
    doc = m.rival_doc()
    s = load(doc)
    sets = [nodes for nodes, _, _ in m.SETS]
    got = s.drain_sets(sets)
    assert [tuple(d) for d in got] == [tuple(d) for _, d, _ in m.SETS]
    assert [s.drain_set_plan(nodes) for nodes in sets] == [plan for _, _, plan in m.SETS]
    # both orders of the ordered pair: other plans, other destinations
    a, b = m.ORDERED_PAIR
    assert s.drain_set_plan([a, b]) != s.drain_set_plan([b, a])
    assert sorted(s.drain_set_plan([a, b])) != sorted(s.drain_set_plan([b, a]))
    # nodes 11 and 12 are drainable alone and not removable together
    alone = s.drain()
    assert alone[11].drainable and alone[12].drainable and not s.drain_sets([[11, 12]])[0].removable
    assert s.drain_sets([[11, 12]])[0].first_blocked == 1
    check_sets(s, doc, sets)
    # the same sets on the competition cluster itself
    comp = load(dm.comp_doc())
    mine = [x for x in m.SETS if max(x[0]) < 11]
    assert [tuple(d) for d in comp.drain_sets([n for n, _, _ in mine])] == [tuple(d) for _, d, _ in mine]
    assert [comp.drain_set_plan(n) for n, _, _ in mine] == [p for _, _, p in mine]


# ------------------------------------------------------------------ 2: singletons, the old kernel against the new
@pytest.mark.parametrize("name", ["comp", "cfg2", "cfg3"])
def test_singletons_equal_ksg_drain(name):
    doc = {"comp": dm.comp_doc, "cfg2": dm.cfg2_doc, "cfg3": dm.cfg3_doc}[name]()
    s = load(doc)
    n = s.n_nodes
    old = s.drain()
    new = s.drain_sets([[x] for x in range(n)])
    assert len(new) == n
    for x in range(n):
        assert tuple(new[x]) == tuple(m.as_set(old[x])), x
        assert s.drain_set_plan([x]) == s.drain_plan(x), x
    assert any(d.unplaced for d in old) and any(d.placed >= 2 for d in old)


# ------------------------------------------------------------------ 3: the event route
def test_equivalence_with_the_event_and_cycle_route():
    """Per subject: removePod, a cycle of the pod without spec.nodeName (commit = 0), ksg_filter_codes, the
    lowest passed node outside the set (chosen here), addPod there (an unplaced pod returns to its node):
    the moves equal the plan taken before.  The ordered pair and a set with an unplaced subject."""
    doc = dm.comp_doc()
    s = load(doc)
    by_name = {full_name(p): p for p in doc["pods"]}
    for nodes in ([6, 4], [0, 4]):
        names = s.bound_pods()
        before = [(names[b][0], names[b][1], d) for b, d in s.drain_set_plan(nodes)]
        assert before and [x for _, x, _ in before] == sorted((x for _, x, _ in before), key=nodes.index)
        route = []
        for name, x, _ in before:
            pod = by_name[name]
            s.apply_events([{"op": "removePod", "name": pod["metadata"]["name"], "namespace": "default"}])
            q, _r = s.cycle(bf.unbound(pod), commit=False)
            codes = s.filter_codes(q)
            dest = next((n for n, c in enumerate(codes) if c == PASSED and n not in nodes), -1)
            back = copy.deepcopy(pod)
            back["spec"]["nodeName"] = doc["nodes"][dest if dest >= 0 else x]["metadata"]["name"]
            s.apply_events([{"op": "addPod", "pod": back}])
            route.append((name, x, dest))
        assert route == before, (nodes, route, before)
        s.close()
        s = load(doc)


# ------------------------------------------------------------------ 4: tile edges
@pytest.mark.parametrize("n_nodes", [T - 1, T, T + 1, 2100])
def test_node_tile_edges(n_nodes):
    """Members on nodes 0, T - 1, T and the last node, each the lowest node with room in its tile and no
    destination; destinations directly behind a member across a tile edge; overlay entries in three
    tiles.  The plans are test_drain_set_model.set_edge_cases' literals."""
    for rooms, cands, nodes, plan in m.set_edge_cases(n_nodes):
        doc = dm.edge_doc(n_nodes, rooms, cands)
        s = load(doc)
        assert s.n_nodes == n_nodes
        assert s.drain_set_plan(nodes) == plan, (rooms, nodes)
        gone = [d for _, d in plan if d >= 0]
        lost = [b for b, d in plan if d < 0]
        pos = {b: i for i, x in enumerate(nodes) for b in dm.on_node(doc, x)}
        got = s.drain_sets([nodes, nodes[:1]])
        assert tuple(got[0]) == (len(plan), 0, len(gone), len(lost), 0, lost[0], pos[lost[0]], len(set(gone))), nodes
        assert tuple(got[1]) == tuple(m.as_set(s.drain(nodes[0], 1)[0]))
        s.close()


def test_first_hit_rotation():
    """test_drain_gpu's rotation case as the one-member set: one k_drain_set block, eight subjects over three
    tiles with hits in tile 0, 2, none, 1, 1, 0, 2, none, so the three first-hit words pass every residue of
    the step count with a hit and without one.  The literals are test_drain_model's, checked there against
    the model and the oracle; first_blocked stands where ksg_drain has `reserved`: the one member, position 0."""
    s = load(dm.rotation_doc())
    assert s.n_nodes == 2 * T + 52
    assert s.drain_set_plan([dm.ROTATION_X]) == dm.ROTATION_PLAN
    got = s.drain_sets([[dm.ROTATION_X]])
    assert len(got) == 1
    d, want = got[0], dm.ROTATION_DRAIN
    assert (d.pods, d.daemon, d.placed, d.unplaced, d.skipped) == (want.pods, want.daemon, want.placed, want.unplaced,
                                                                   want.skipped)
    assert d.first_unplaced == want.first_unplaced and d.dest_nodes == want.dest_nodes
    assert d.first_blocked == 0 and not d.removable
    s.close()


# ------------------------------------------------------------------ 5: the hash overlay
@pytest.mark.parametrize("case", sorted(m.HASH_CASES))
def test_hash_overlay(case, monkeypatch):
    """KSG_DRAIN_MAX=4 at ksg_create: 8 slots.  The destinations share a home slot, are pushed along, and
    wrap from slot 7 to slot 0 (test_drain_set_model.test_hash_cases_collide); every later subject has to
    find each entry again to be refused by the lowered rows.  Six subjects on two members: two skipped."""
    dests = m.HASH_CASES[case]
    doc = m.hash_doc(dests)
    monkeypatch.setenv("KSG_DRAIN_MAX", "4")
    s = load(doc)
    monkeypatch.delenv("KSG_DRAIN_MAX")
    plan = s.drain_set_plan([1, 2])
    assert plan == list(zip(range(6), dests + [-2, -2]))
    got = s.drain_sets([[1, 2], [2, 1], [1]])
    assert tuple(got[0]) == (6, 0, 4, 0, 2, -1, 1, 4) and not got[0].removable  # first_blocked: the second member
    check_sets(s, doc, [[1, 2], [2, 1], [1], [2]], cap=m.HASH_CAP)
    assert tuple(got[2]) == tuple(m.as_set(s.drain(1, 1)[0])) and s.drain_set_plan([1]) == s.drain_plan(1)
    s.close()
    # without the override (1024 slots) all six are simulated
    s = load(doc)
    assert s.drain_set_plan([1, 2]) == list(zip(range(6), dests + [-1, -1]))
    assert tuple(s.drain_sets([[1, 2]])[0]) == (6, 0, 4, 2, 0, 4, 1, 4)


# ------------------------------------------------------------------ 6: limits
def raw_sets(s, sets):
    flat = [x for nodes in sets for x in nodes]
    start = [0]
    for nodes in sets:
        start.append(start[-1] + len(nodes))
    out = (_DrainSet * max(len(sets), 1))()
    rc = s.L.ksg_drain_sets(s.h, (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_uint32 * len(start))(*start),
                            len(sets), out)
    return rc, bytes(out)


def test_limits_and_errors_leave_the_context_usable():
    doc = m.limit_doc()
    s = load(doc)
    n = s.n_nodes
    assert n == 140 and m.SET_NODES == 128
    whole = list(range(128))
    check_sets(s, doc, [whole, whole[::-1]])  # a 128-node set is answered
    assert len(s.drain_prefixes(whole)) == 128
    before = raw_sets(s, [whole, [1, 5], []])
    assert before[0] == 0
    assert raw_sets(s, [list(range(129))])[0] == E_RANGE
    assert raw_sets(s, [[1], list(range(129))])[0] == E_RANGE
    nodes = (ctypes.c_uint32 * 130)(*range(130))
    out = (_DrainSet * 130)()
    mv = (_DrainMove * 64)()
    cnt = ctypes.c_uint32(9)
    assert s.L.ksg_drain_prefixes(s.h, nodes, 129, out) == E_RANGE
    assert s.L.ksg_drain_set_plan(s.h, nodes, 129, mv, 64, ctypes.byref(cnt)) == E_RANGE and cnt.value == 0
    # a node listed twice: KSG_E_INVALID, the message names it
    for call in (lambda: s.drain_sets([[1, 2], [5, 9, 5]]), lambda: s.drain_prefixes([3, 5, 9, 5]),
                 lambda: s.drain_set_plan([5, 5])):
        with pytest.raises(KsgError, match=r": -1 .*node 5 \(node-0000005\) is listed twice"):
            call()
    assert raw_sets(s, [[1, 2], [5, 9, 5]])[0] == E_INVALID
    # a node outside the local nodes
    assert raw_sets(s, [[1, n]])[0] == E_RANGE and raw_sets(s, [[0xFFFFFFFF]])[0] == E_RANGE
    assert s.L.ksg_drain_prefixes(s.h, (ctypes.c_uint32 * 2)(1, n), 2, out) == E_RANGE
    # required pointers
    st = (ctypes.c_uint32 * 2)(0, 2)
    assert s.L.ksg_drain_sets(s.h, None, st, 1, out) == E_RANGE
    assert s.L.ksg_drain_sets(s.h, nodes, None, 1, out) == E_RANGE
    assert s.L.ksg_drain_sets(s.h, nodes, st, 1, None) == E_RANGE
    assert s.L.ksg_drain_sets(s.h, nodes, (ctypes.c_uint32 * 3)(0, 4, 2), 2, out) == E_RANGE  # descending
    assert s.L.ksg_drain_prefixes(s.h, None, 2, out) == E_RANGE and s.L.ksg_drain_prefixes(s.h, nodes, 2, None) == E_RANGE
    assert s.L.ksg_drain_set_plan(s.h, nodes, 2, None, 8, ctypes.byref(cnt)) == E_RANGE
    assert s.L.ksg_drain_set_plan(s.h, nodes, 2, mv, 8, None) == E_RANGE
    # nothing asked: nothing written
    out[0].pods = 77
    assert s.L.ksg_drain_sets(s.h, None, None, 0, None) == 0 and s.L.ksg_drain_sets(s.h, nodes, st, 0, out) == 0
    assert s.L.ksg_drain_prefixes(s.h, nodes, 0, out) == 0
    cnt.value = 9
    assert s.L.ksg_drain_set_plan(s.h, nodes, 0, mv, 8, ctypes.byref(cnt)) == 0 and cnt.value == 0
    assert out[0].pods == 77
    assert s.drain_sets([]) == [] and s.drain_prefixes([]) == [] and s.drain_set_plan([]) == []
    # an empty set, alone and between others
    assert [tuple(d) for d in s.drain_sets([[]])] == [tuple(m.EMPTY)]
    got = s.drain_sets([[1], [], [5]])
    assert tuple(got[1]) == tuple(m.EMPTY) and got[0] == got[2] and got[0].placed == 1
    assert s.L.ksg_drain_sets(s.h, None, (ctypes.c_uint32 * 2)(0, 0), 1, out) == 0 and out[0].first_blocked == -1
    # a short plan buffer
    mv[0].bound = 55
    assert s.L.ksg_drain_set_plan(s.h, nodes, 128, mv, 31, ctypes.byref(cnt)) == E_NOBUF and cnt.value == 32
    assert mv[0].bound == 55
    assert s.L.ksg_drain_set_plan(s.h, nodes, 128, mv, 32, ctypes.byref(cnt)) == 0 and cnt.value == 32
    assert [(mv[i].bound, mv[i].dest) for i in range(32)] == m.simulate_set(doc, whole)[1]
    assert raw_sets(s, [whole, [1, 5], []]) == before
    s.schedule()  # the context goes on working
    assert [r.status for r in s.results()] == [0]


# ------------------------------------------------------------------ 7: prefixes
def test_prefixes():
    doc = dm.cfg2_doc()
    nodes = m.prefix_nodes()
    s = load(doc)
    got = s.drain_prefixes(nodes)
    assert len(got) == m.PREFIX_NODES == 24
    assert got == s.drain_sets([nodes[:k + 1] for k in range(len(nodes))])
    assert [tuple(d) for d in got] == [tuple(d) for d in m.prefix_model()]
    assert any(d.removable for d in got) and any(not d.removable for d in got)
    comp = load(m.rival_doc())
    assert [tuple(d) for d in comp.drain_prefixes([6, 4, 11, 12, 0])] == [tuple(d) for d in m.prefixes(
        m.rival_doc(), [6, 4, 11, 12, 0])]


# ------------------------------------------------------------------ 8: families
@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_families(family):
    doc = dm.cfg2_doc() if family == "cfg2" else dm.cfg3_doc()
    sets = m.family_sets(family)
    s = load(doc)
    got = check_sets(s, doc, sets, m.family_set_model(family))
    alone = s.drain()
    blocked = [i for i, d in enumerate(got) if d.unplaced > 0 and all(alone[x].drainable for x in sets[i])]
    assert blocked == m.rivals(family) and blocked


# ------------------------------------------------------------------ 9: the live snapshot, purity
def raw(s, sets):
    out = raw_sets(s, sets)
    assert out[0] == 0
    out = out[1]
    for nodes in sets:
        mv, cnt = (_DrainMove * 64)(), ctypes.c_uint32()
        assert s.L.ksg_drain_set_plan(s.h, (ctypes.c_uint32 * max(len(nodes), 1))(*nodes), len(nodes), mv, 64,
                                      ctypes.byref(cnt)) == 0
        out += bytes(mv)[:8 * cnt.value]
    pre = (_DrainSet * len(sets[0]))()
    assert s.L.ksg_drain_prefixes(s.h, (ctypes.c_uint32 * len(sets[0]))(*sets[0]), len(sets[0]), pre) == 0
    return out + bytes(pre)


def raw_drain(s):
    arr = (_Drain * s.n_nodes)()
    assert s.L.ksg_drain(s.h, 0, s.n_nodes, arr) == 0
    return bytes(arr)


def test_live_snapshot_and_purity():
    base = m.rival_doc()
    doc = {"profile": base["profile"], "nodes": copy.deepcopy(base["nodes"]), "pods": list(base["pods"]),
           "queue": list(base["queue"])}
    sets = [nodes for nodes, _, _ in m.SETS] + [[6, 4, 11, 12, 0]]
    subjects, load_only = list(doc["pods"]), []
    s = load(doc)
    s.drain_sets(sets)  # (binds the argument types)
    s.drain_set_plan(sets[0])
    s.drain_prefixes(sets[0])
    # a queue run: the placed queue pods are load on their nodes, not subjects
    by_name = {full_name(p): p for p in doc["queue"]}
    s.schedule()
    for q, r in enumerate(s.results()):
        assert r.status == 0
        p = copy.deepcopy(by_name[s.queue_pod(q)])
        p["spec"]["nodeName"] = doc["nodes"][r.selected]["metadata"]["name"]
        load_only.append(p)
    doc["pods"] = subjects + load_only
    before, drains = s.node_requested(), raw_drain(s)
    got = check_sets(s, doc, sets, n_subjects=len(subjects))
    assert got[-1].pods == 13
    assert s.node_requested() == before and raw_drain(s) == drains
    # an in-place event batch cordons the ordered pair's first destination: the plans move on
    dest = s.drain_set_plan([6, 4])[1][1]
    assert dest >= 0
    upd = copy.deepcopy(doc["nodes"][dest])
    upd["spec"]["unschedulable"] = True
    s.apply_events([{"op": "updateNode", "node": upd}])
    doc["nodes"][dest] = upd
    before, drains = s.node_requested(), raw_drain(s)
    check_sets(s, doc, sets, n_subjects=len(subjects))
    assert all(d != dest for nodes in sets for _, d in s.drain_set_plan(nodes))
    assert s.node_requested() == before and raw_drain(s) == drains
    # compact: the placed queue pods become bound pods behind the others, and subjects of their nodes
    s.compact()
    assert s.bound_count == len(doc["pods"])
    before, drains = s.node_requested(), raw_drain(s)
    check_sets(s, doc, sets)
    # two calls return the same bytes; the rows and ksg_drain's answer did not move
    assert raw(s, sets) == raw(s, sets)
    assert s.node_requested() == before and raw_drain(s) == drains


# ------------------------------------------------------------------ 10: refusals
def refused(doc, match, **kw):
    s = Scheduler(doc["profile"], **kw)
    s.load_cluster(doc)
    out = (_DrainSet * 2)()
    s.L.ksg_drain_sets.argtypes = [ctypes.c_void_p, U32P, U32P, ctypes.c_uint32, ctypes.POINTER(_DrainSet)]
    assert s.L.ksg_drain_sets(s.h, (ctypes.c_uint32 * 2)(0, 1), (ctypes.c_uint32 * 2)(0, 2), 1, out) == E_INVALID
    for call in (lambda: s.drain_sets([[0, 1]]), lambda: s.drain_prefixes([0, 1]), lambda: s.drain_set_plan([0, 1])):
        with pytest.raises(KsgError, match=match):
            call()
    return s


def test_profiles_outside_the_closed_form():
    cfg4 = g.generate(4, n_nodes=40, n_existing=60, n_pods=8, n_zones=4)
    s = refused(cfg4, "PodTopologySpread")
    s.schedule()  # a queue run still works after the refusal
    assert len(s.results()) == 8
    nofit = dict(dm.comp_doc())
    nofit["profile"] = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2)], 7)
    refused(nofit, "NodeResourcesFit")
    refused(bf.cfg2_doc(), "sharded", shard_rank=0, shard_count=2)
