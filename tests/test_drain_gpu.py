"""Drain simulation (ksg_drain / ksg_drain_plan; Scheduler.drain / drain_plan): a
node's bound pods re-placed one after another on the device, first fit in node
order, each counted on its destination before the next is judged.

No expected value comes from the calls under test.  The references are those of
test_drain_model -- hand-written literals, a few lines of Python over the
eviction fit's model, and the ORACLE as an experiment, pinned against each other
there on the CPU -- and, on the GPU, the engine's existing routes: per subject
removePod, ksg_cycle(commit=0), ksg_filter_codes, addPod on the destination; and
ksg_bound_fit, which does not run the new kernel.

Kernel constants: one block of 256 threads per candidate walks the nodes in tiles
of T = kSqTile = 1024 (csrc/snapshot_query.hip; 4 nodes per thread) and ends a
subject's walk at the first tile with a hit; KSG_DRAIN_MAX = 512 subjects.
"""
import copy
import ctypes

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import KsgError, _Drain, _DrainMove
import test_bound_fit_model as bf
import test_drain_model as m

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE, E_NOBUF = -1, -4, -5
PASSED = bf.PASSED
T = m.TILE


def load(doc):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    return s


def full_name(pod):
    return (pod["metadata"].get("namespace") or "default") + "/" + pod["metadata"]["name"]


def check_all(s, doc, model=None, n_subjects=None, cap=m.DRAIN_MAX):
    """One ksg_drain over every node and every node's plan equal the model."""
    model = m.simulate_all(doc, cap, n_subjects) if model is None else model
    got = s.drain()
    assert len(got) == len(model) == s.n_nodes
    for x, (d, plan) in enumerate(model):
        assert tuple(got[x]) == tuple(d), (x, got[x], d)
        assert got[x].drainable == m.drainable(d)
        if d.pods or x % 16 == 0:
            assert s.drain_plan(x) == plan, x
    return got


# ------------------------------------------------------------------ 1: the competition cluster
def test_competition_cluster():
    doc = m.comp_doc()
    s = load(doc)
    got = s.drain()
    assert [tuple(d) for d in got] == [tuple(d) for d in m.COMP]
    assert [s.drain_plan(x) for x in range(len(doc["nodes"]))] == m.COMP_PLANS
    assert [d.drainable for d in got] == [False, True, True, False, True, False, True, False, False, False, False]
    # judged alone every pod of node 0 has somewhere to go; the drain leaves one of the two competitors behind
    assert s.node_evictability()[0] == (4, 0, 0) and got[0].unplaced == 1 and got[0].first_unplaced == 3
    assert s.drain(4, 3) == got[4:7] and s.drain(10, 1) == got[10:] and s.drain(0, 0) == []
    check_all(s, doc)


def test_equivalence_with_the_event_and_cycle_route():
    """Per subject: removePod, a cycle of the pod without spec.nodeName (commit = 0), ksg_filter_codes, the
    lowest passed node other than the candidate, addPod there (an unplaced pod returns to its node): the moves
    equal the plan taken before.  Node 0 (the competitors, two pods left in place), 4 (a destination filled
    exactly), 6 (pod room through the overlay alone), 7 (the gpu), 10 (a rejected subject)."""
    doc = m.comp_doc()
    s = load(doc)
    by_name = {full_name(p): p for p in doc["pods"]}
    for x in (0, 4, 6, 7, 10):
        names = s.bound_pods()
        before = [(names[b][0], d) for b, d in s.drain_plan(x)]
        assert before and all(names[b][1] == x for b, _ in s.drain_plan(x))
        route = []
        for name, _ in before:
            pod = by_name[name]
            s.apply_events([{"op": "removePod", "name": pod["metadata"]["name"], "namespace": "default"}])
            q, _r = s.cycle(bf.unbound(pod), commit=False)
            codes = s.filter_codes(q)
            dest = next((n for n, c in enumerate(codes) if c == PASSED and n != x), -1)
            back = copy.deepcopy(pod)
            back["spec"]["nodeName"] = doc["nodes"][dest if dest >= 0 else x]["metadata"]["name"]
            s.apply_events([{"op": "addPod", "pod": back}])
            route.append((name, dest))
        assert route == before, (x, route, before)


# ------------------------------------------------------------------ 2: tile edges
@pytest.mark.parametrize("n_nodes", [T - 1, T, T + 1, 2 * T + 52])
def test_node_tile_edges(n_nodes):
    """T = 1024 nodes a tile: one short, exact, one node into a second tile, two tiles and a ragged third.  The
    only admitting destination on node 0, the last node, the last node of tile 0 and the first of tile 1;
    candidates node 0, the last node and the destination's neighbours; a drain whose overlay entries lie in
    two (three) tiles.  The destinations are test_drain_model.edge_cases' literals, checked there against
    the model and the oracle."""
    for rooms, cands, want in m.edge_cases(n_nodes):
        doc = m.edge_doc(n_nodes, rooms, cands)
        s = load(doc)
        got = s.drain()
        assert len(got) == n_nodes
        b0 = 0
        for x in sorted(cands):
            plan = s.drain_plan(x)
            assert plan == list(zip(range(b0, b0 + cands[x]), want[x])), (rooms, x, plan)
            b0 += cands[x]
            gone = [d for d in want[x] if d >= 0]
            assert tuple(got[x]) == (cands[x], 0, len(gone), cands[x] - len(gone), 0,
                                     plan[len(gone)][0] if len(gone) < cands[x] else -1, len(set(gone))), (rooms, x)
        assert all(tuple(got[x]) == tuple(m.EMPTY) for x in range(n_nodes) if x not in cands)
        s.close()


def test_first_hit_rotation():
    """One block, eight subjects of four sizes over three tiles: hits in tile 0, 2, none, 1, 1, 0, 2, none, so
    the rotation of the three first-hit words passes every residue with a hit and without one.  The plan is
    test_drain_model's literal, checked there against the model and the oracle."""
    s = load(m.rotation_doc())
    assert s.drain_plan(m.ROTATION_X) == m.ROTATION_PLAN
    got = s.drain(m.ROTATION_X, 1)[0]
    assert tuple(got) == tuple(m.ROTATION_DRAIN) and not got.drainable
    s.close()


# ------------------------------------------------------------------ 3: the cap
def test_cap(monkeypatch):
    """KSG_DRAIN_MAX=4 at ksg_create: of six subjects four are simulated, two skipped."""
    base = m.comp_doc()
    names = [n["metadata"]["name"] for n in base["nodes"]]
    extra = [g.pod_obj(f"e{j}", [g.req(100, 64 * g.Mi)], node=names[6]) for j in range(2)]
    doc = dict(base, pods=base["pods"] + extra)
    want, plan = m.simulate(doc, 6, cap=4)
    assert want.skipped == 2 and want.placed + want.unplaced == 4 and [d for _, d in plan[4:]] == [-2, -2]
    monkeypatch.setenv("KSG_DRAIN_MAX", "4")
    s = load(doc)
    monkeypatch.delenv("KSG_DRAIN_MAX")
    got = s.drain(6, 1)[0]
    assert tuple(got) == tuple(want) and not got.drainable
    assert s.drain_plan(6) == plan
    check_all(s, doc, cap=4)
    assert tuple(load(doc).drain(6, 1)[0]) == tuple(m.simulate(doc, 6)[0])  # without the override: all six


# ------------------------------------------------------------------ 4: families
def bound_fit_cross_check(s, got):
    """Against ksg_bound_fit (no code of the drain): the first subject's destination is its first_other;
    a subject with no other node is unplaced."""
    fits = s.bound_fit()
    n_first = 0
    for x, d in enumerate(got):
        if d.pods == d.daemon:
            continue
        plan = s.drain_plan(x)
        assert plan[0][1] == fits[plan[0][0]].first_other, x
        assert all(dest == -1 for b, dest in plan if fits[b].other_nodes == 0), x
        assert all(fits[b].node == x for b, _ in plan)
        n_first += 1
    return n_first


@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_families(family):
    doc = m.cfg2_doc() if family == "cfg2" else m.cfg3_doc()
    s = load(doc)
    got = check_all(s, doc, m.family_model(family))
    assert any(d.unplaced for d in got) and any(d.drainable and d.placed >= 2 for d in got) and any(d.daemon for d in got)
    assert bound_fit_cross_check(s, got) >= len(doc["nodes"]) // 2


# ------------------------------------------------------------------ 5: the live snapshot
def raw(s):
    n = s.n_nodes
    arr = (_Drain * n)()
    assert s.L.ksg_drain(s.h, 0, n, arr) == 0
    out = bytes(arr)
    for x in range(n):
        mv, cnt = (_DrainMove * 64)(), ctypes.c_uint32()
        assert s.L.ksg_drain_plan(s.h, x, mv, 64, ctypes.byref(cnt)) == 0
        out += bytes(mv)[:8 * cnt.value]
    return out


def test_live_snapshot():
    base = m.comp_doc()
    doc = {"profile": base["profile"], "nodes": copy.deepcopy(base["nodes"]), "pods": list(base["pods"]),
           "queue": list(base["queue"])}
    subjects, load_only = list(doc["pods"]), []
    s = load(doc)
    s.drain()
    # a queue run: the placed queue pods are load on their nodes, not subjects
    by_name = {full_name(p): p for p in doc["queue"]}
    s.schedule()
    for q, r in enumerate(s.results()):
        assert r.status == 0
        p = copy.deepcopy(by_name[s.queue_pod(q)])
        p["spec"]["nodeName"] = doc["nodes"][r.selected]["metadata"]["name"]
        load_only.append(p)
    doc["pods"] = subjects + load_only
    before = s.node_requested()
    got = check_all(s, doc, n_subjects=len(subjects))
    assert sum(d.pods for d in got) == len(subjects)
    bound_fit_cross_check(s, got)
    assert s.node_requested() == before
    # an event batch cordons node 4's first destination: the plan moves on
    dest = s.drain_plan(4)[0][1]
    assert dest >= 0
    upd = copy.deepcopy(doc["nodes"][dest])
    upd["spec"]["unschedulable"] = True
    s.apply_events([{"op": "updateNode", "node": upd}])
    doc["nodes"][dest] = upd
    before = s.node_requested()
    check_all(s, doc, n_subjects=len(subjects))
    assert all(d != dest for x in range(s.n_nodes) for _, d in s.drain_plan(x))
    # two calls return the same bytes; the rows did not move
    assert raw(s) == raw(s)
    assert s.node_requested() == before


def test_no_side_effects_on_a_queue_run():
    doc = m.cfg2_doc()
    a, b = load(doc), load(doc)
    a.schedule()
    n = len(doc["queue"])
    for q in range(n):  # drain calls between the pods of b's run
        b.drain((17 * q) % 150, 40)
        b.drain_plan((29 * q) % 200)
        b.schedule(q, 1)
    assert a.results() == b.results()
    assert a.node_requested() == b.node_requested()
    assert a.drain() == b.drain()


# ------------------------------------------------------------------ 6: refusals
def test_errors_leave_the_context_usable():
    doc = m.comp_doc()
    s = load(doc)
    s.drain()  # (binds the argument types)
    s.drain_plan(0)
    before = raw(s)
    out = (_Drain * 12)()
    mv = (_DrainMove * 8)()
    n = ctypes.c_uint32(9)
    assert s.n_nodes == 11
    assert s.L.ksg_drain(s.h, 0, 3, None) == E_RANGE
    assert s.L.ksg_drain(s.h, 9, 3, out) == E_RANGE
    assert s.L.ksg_drain(s.h, 12, 0, out) == E_RANGE
    assert s.L.ksg_drain(s.h, 0xFFFFFFFF, 2, out) == E_RANGE
    assert s.L.ksg_drain_plan(s.h, 11, mv, 8, ctypes.byref(n)) == E_RANGE and n.value == 0
    assert s.L.ksg_drain_plan(s.h, 0, None, 8, ctypes.byref(n)) == E_RANGE
    assert s.L.ksg_drain_plan(s.h, 0, mv, 8, None) == E_RANGE
    out[0].pods = 77
    assert s.L.ksg_drain(s.h, 11, 0, out) == 0 and s.L.ksg_drain(s.h, 0, 0, out) == 0
    assert out[0].pods == 77  # count == 0 writes nothing
    mv[0].bound = 55
    assert s.L.ksg_drain_plan(s.h, 6, mv, 3, ctypes.byref(n)) == E_NOBUF and n.value == 4  # a short buffer
    assert mv[0].bound == 55
    assert s.L.ksg_drain_plan(s.h, 6, mv, 4, ctypes.byref(n)) == 0 and n.value == 4
    assert [(mv[i].bound, mv[i].dest) for i in range(4)] == m.COMP_PLANS[6]
    assert s.L.ksg_drain_plan(s.h, 1, mv, 0, ctypes.byref(n)) == 0 and n.value == 0  # no subjects: nothing to hold
    assert raw(s) == before
    s.schedule()  # the context goes on working
    assert [r.status for r in s.results()] == [0, 0]


def refused(doc, match, **kw):
    s = Scheduler(doc["profile"], **kw)
    s.load_cluster(doc)
    out = (_Drain * 1)()
    s.L.ksg_drain.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_Drain)]
    assert s.L.ksg_drain(s.h, 0, 1, out) == E_INVALID
    for call in (lambda: s.drain(0, 1), lambda: s.drain_plan(0)):
        with pytest.raises(KsgError, match=match):
            call()
    return s


def test_profiles_outside_the_closed_form():
    cfg4 = g.generate(4, n_nodes=40, n_existing=60, n_pods=8, n_zones=4)
    s = refused(cfg4, "PodTopologySpread")
    s.schedule()  # a queue run still works after the refusal
    assert len(s.results()) == 8
    nofit = dict(m.comp_doc())
    nofit["profile"] = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2)], 7)
    refused(nofit, "NodeResourcesFit")
    refused(bf.cfg2_doc(), "sharded", shard_rank=0, shard_count=2)
