"""Scale-up simulation (ksg_scale_up / ksg_scale_up_plan; Scheduler.scale_up /
scale_up_plan): a list of queue pods packed onto fresh nodes shaped like a
template node, first fit in bin order, one block per template on the device.

No expected value comes from the calls under test.  The references are those of
test_scale_up_model -- hand-written literals, a few lines of Python first fit,
and the ORACLE as an experiment, pinned against each other there on the CPU --
closed-form literals at the bin edges, and, on the GPU, the engine's existing
route: a second context loaded with clones of the template, then per pod
ksg_cycle(commit=0), ksg_filter_codes and ksg_reserve on the lowest passed clone.

Kernel constants: one block of 256 threads per template; bin j lives in thread
j % 256, slot j / 256 (4 slots: KSG_SCALE_MAX = 1024 bins); a wave holds 64 bins
of a slot.
"""
import copy
import ctypes

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import KsgError, _ScaleUp
import test_bound_fit_model as bf
import test_scale_up_model as m

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -4
PASSED, NOT_EVALUATED = bf.PASSED, bf.NOT_EVALUATED
U32P = ctypes.POINTER(ctypes.c_uint32)


def load(doc):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    return s


def full_name(pod):
    return (pod["metadata"].get("namespace") or "default") + "/" + pod["metadata"]["name"]


def queue_index(s, doc):
    """Position in doc["queue"] -> the engine's queue index (the engine keeps the queue in scheduling order)."""
    at = {s.queue_pod(q): q for q in range(s.queue_len)}
    return [at[full_name(p)] for p in doc["queue"]]


def check(s, doc, pods, templates, max_nodes=m.SCALE_MAX, plans=True):
    """One ksg_scale_up over `templates` and (plans) every template's plan equal the model."""
    qi = queue_index(s, doc)
    lst = [qi[q] for q in pods]
    got = s.scale_up(lst, templates, max_nodes)
    assert len(got) == len(templates)
    for i, t in enumerate(templates):
        want, plan = m.pack(doc, pods, t, max_nodes)
        assert tuple(got[i]) == tuple(want), (t, got[i], want)
        assert got[i].satisfied == m.satisfied(want, len(pods))
        if plans:
            assert s.scale_up_plan(lst, t, max_nodes) == plan, t
    return got


# ------------------------------------------------------------------ 1: the hand cluster
def test_hand_cluster():
    doc = m.hand_doc()
    s = load(doc)
    qi = queue_index(s, doc)
    lst = [qi[q] for q in m.LIST]
    got = s.scale_up(lst, range(6))
    assert [tuple(x) for x in got] == [tuple(x) for x in m.HAND]
    assert [s.scale_up_plan(lst, t) for t in range(6)] == m.HAND_PLANS
    assert not any(x.satisfied for x in got)
    check(s, doc, m.LIST, list(range(6)))
    # sub-lists of templates equal slices, in any order; a template listed twice gives equal structs
    assert s.scale_up(lst, [2, 3, 4]) == got[2:5] and s.scale_up(lst, [5]) == got[5:] and s.scale_up(lst, []) == []
    assert s.scale_up(lst, [4, 0, 4, 4, 1]) == [got[4], got[0], got[4], got[4], got[1]]
    # other lists: one the plain template satisfies, the empty list, another order
    five = s.scale_up([qi[q] for q in (1, 2, 3, 4, 5)], [m.PLAIN])[0]
    assert tuple(five) == (2, 5, 0, 0, 0, -1, 0) and five.satisfied
    assert s.scale_up_plan([qi[q] for q in (1, 2, 3, 4, 5)], m.PLAIN) == [0, 0, 1, 1, 0]
    assert [tuple(x) for x in s.scale_up([], [m.BASE, m.PLAIN])] == [(0, 0, 0, 0, 0, -1, 2), (0, 0, 0, 0, 0, -1, 0)]
    assert s.scale_up_plan([], m.BASE) == []
    assert s.scale_up_plan([qi[q] for q in (0, 12, 11, 5)], m.BASE) == [0, 1, 1, 0]
    assert s.scale_up_plan([qi[q] for q in (12, 11, 5, 0)], m.LIMIT2) == [0, 0, 1, 1]


# ------------------------------------------------------------------ 2: the engine's existing route
@pytest.mark.parametrize("t", [m.GPUS, m.LIMIT2, m.BASE])
def test_equivalence_with_the_clone_and_cycle_route(t):
    """A second context holds 6 clones of the template (more than it opens), each with the base pods.  Per list
    entry: ksg_cycle(commit=0), ksg_filter_codes, ksg_reserve on the lowest passed clone.  Without a passed
    clone the pod is closed when the failing Filter is not NodeResourcesFit (or no clone was evaluated), else
    too big (an empty clone was among them)."""
    doc = m.hand_doc()
    s = load(doc)
    qi = queue_index(s, doc)
    before = s.scale_up_plan([qi[q] for q in m.LIST], t, 6)
    c = load(m.clone_doc(doc, t, 6))
    fit_pos = doc["profile"]["plugins"].index(bf.FIT)
    route = []
    for i, q in enumerate(m.LIST):
        q2, _r = c.cycle(m.replica(doc, q, i), commit=False)
        codes = c.filter_codes(q2)
        dest = next((n for n, code in enumerate(codes) if code == PASSED), -1)
        if dest >= 0:
            c.reserve(q2, dest)
            route.append(dest)
        else:
            assert len(set(codes)) == 1 or all(code >> 24 == fit_pos for code in codes)
            route.append(m.CLOSED if codes[5] == NOT_EVALUATED or codes[5] >> 24 != fit_pos else m.TOO_BIG)
    assert max(route) < 5  # (clone 5 stayed empty: what it refused is too big)
    assert route == before == m.HAND_PLANS[t], (t, route, before)


# ------------------------------------------------------------------ 3: bin edges
def test_bin_edges_every_pod_opens_a_bin():
    """A pod limit of 1: pod i opens bin i.  63 / 64 / 65 cross a wave, 255 / 256 / 257 a slot, 1023 / 1024 the
    last bin; the 1025th pod meets the cap."""
    doc = m.limit1_doc(1025)
    s = load(doc)
    qi = queue_index(s, doc)
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        lst = [qi[q] for q in range(n)]
        got = s.scale_up(lst, [0], 1024)[0]
        k = min(n, 1024)
        assert got.nodes == k
        assert tuple(got) == (k, k, 0, 0, n - k, 1024 if n > 1024 else -1, 0), n
        assert s.scale_up_plan(lst, 0, 1024) == list(range(k)) + [m.OVER_CAP] * (n - k), n
    assert got.over_cap == 1 and got.first_unpacked == 1024
    assert tuple(s.scale_up(lst, [0])[0]) == tuple(got)  # (the default cap is KSG_SCALE_MAX)


def test_back_fill_across_the_boundaries():
    """300 pods of 900m on a 1000m template open bins 0..299 and leave room for one pod of 100m each; 300 such
    pods then land in bins 0..299 in order (every wave and two slots are hit in turn); the next opens bin 300."""
    doc = m.backfill_doc(300, 301)
    s = load(doc)
    qi = queue_index(s, doc)
    lst = [qi[q] for q in range(601)]
    assert tuple(s.scale_up(lst, [0])[0]) == (301, 601, 0, 0, 0, -1, 0)
    assert s.scale_up_plan(lst, 0) == list(range(300)) + list(range(300)) + [300]
    # under a cap of 300 the last pod finds every bin full
    assert tuple(s.scale_up(lst, [0], 300)[0]) == (300, 600, 0, 0, 1, 600, 0)
    assert s.scale_up_plan(lst, 0, 300)[-2:] == [299, m.OVER_CAP]


# ------------------------------------------------------------------ 4: caps
def test_caps(monkeypatch):
    doc = m.hand_doc()
    s = load(doc)
    qi = queue_index(s, doc)
    lst = [qi[q] for q in m.LIST]
    # max_nodes as an argument
    assert (tuple(s.scale_up(lst, [m.PLAIN], 2)[0]), s.scale_up_plan(lst, m.PLAIN, 2)) == (tuple(m.CAP2), m.CAP2_PLAN)
    assert s.scale_up_plan(lst, m.PLAIN, 3) == [0, 1, 1, 0, 2, 0, -2, -1, -2, -2, 2, 2, 2, -3]
    check(s, doc, m.LIST, list(range(6)), max_nodes=3)
    check(s, doc, m.LIST, list(range(6)), max_nodes=1)
    # KSG_SCALE_MAX=4 at ksg_create lowers the upper bound of max_nodes
    edge = m.limit1_doc(6)
    monkeypatch.setenv("KSG_SCALE_MAX", "4")
    low = load(edge)
    monkeypatch.delenv("KSG_SCALE_MAX")
    six = [queue_index(low, edge)[q] for q in range(6)]
    with pytest.raises(KsgError) as e:
        low.scale_up(six, [0], 8)
    assert e.value.args and low.L.ksg_scale_up(low.h, (ctypes.c_uint32 * 6)(*six), 6, (ctypes.c_uint32 * 1)(0), 1, 8,
                                               (_ScaleUp * 1)()) == E_RANGE
    with pytest.raises(KsgError):
        low.scale_up(six, [0])  # (the default, 1024, is above the lowered bound too)
    assert tuple(low.scale_up(six, [0], 4)[0]) == (4, 4, 0, 0, 2, 4, 0)
    assert low.scale_up_plan(six, 0, 4) == [0, 1, 2, 3, -3, -3]
    # without the override the same list packs fully at 8
    full = load(edge)
    six = [queue_index(full, edge)[q] for q in range(6)]
    assert tuple(full.scale_up(six, [0], 8)[0]) == (6, 6, 0, 0, 0, -1, 0) and full.scale_up(six, [0], 8)[0].satisfied


# ------------------------------------------------------------------ 5: many templates in one launch
def test_many_templates():
    doc, pods, model = m.many_doc(), m.many_list(), m.many_model()
    ss = [x for x, _ in model]
    assert len(doc["nodes"]) == 300 and len(pods) == 64
    assert any(x.closed for x in ss) and any(x.too_big for x in ss) and any(x.base_pods for x in ss)
    assert any(m.satisfied(x, 64) and x.nodes >= 2 for x in ss)
    s = load(doc)
    qi = queue_index(s, doc)
    lst = [qi[q] for q in pods]
    got = s.scale_up(lst, range(300))
    assert [tuple(x) for x in got] == [tuple(x) for x in ss]
    for t in range(0, 300, 16):
        assert s.scale_up_plan(lst, t) == model[t][1], t


# ------------------------------------------------------------------ 6: the live snapshot
def raw(s, lst, templates):
    p, t = (ctypes.c_uint32 * len(lst))(*lst), (ctypes.c_uint32 * len(templates))(*templates)
    arr = (_ScaleUp * len(templates))()
    assert s.L.ksg_scale_up(s.h, p, len(lst), t, len(templates), 1024, arr) == 0
    out = bytes(arr)
    for x in templates:
        bins = (ctypes.c_int32 * len(lst))()
        assert s.L.ksg_scale_up_plan(s.h, p, len(lst), x, 1024, bins) == 0
        out += bytes(bins)
    return out


def test_live_snapshot():
    base = m.hand_doc()
    doc = {"profile": base["profile"], "nodes": copy.deepcopy(base["nodes"]), "pods": list(base["pods"]),
           "queue": list(base["queue"])}
    s = load(doc)
    all6 = list(range(6))
    first = check(s, doc, m.LIST, all6)
    # a queue run: what it places on a template is load there, not part of a fresh node
    s.schedule()
    assert sum(r.status == 0 and r.selected >= 0 for r in s.results()) >= 8
    before = s.node_requested()
    assert check(s, doc, m.LIST, all6) == first and [tuple(x) for x in first] == [tuple(x) for x in m.HAND]
    # updateNode in place: the plain template gains the taint (only `tol` stays open) ...
    upd = copy.deepcopy(doc["nodes"][m.PLAIN])
    upd["spec"]["taints"] = [dict(bf.GPU_TAINT)]
    s.apply_events([{"op": "updateNode", "node": upd}])
    doc["nodes"][m.PLAIN] = upd
    got = check(s, doc, m.LIST, all6)
    assert tuple(got[m.PLAIN]) == tuple(m.HAND[m.TAINTED]) and got[1:] == first[1:]
    # ... and the limit-2 template loses half its cpu: big and a medium pod no longer share a bin, small-a joins big
    upd = copy.deepcopy(doc["nodes"][m.LIMIT2])
    for k in ("allocatable", "capacity"):
        upd["status"][k]["cpu"] = "4"
    s.apply_events([{"op": "updateNode", "node": upd}])
    doc["nodes"][m.LIMIT2] = upd
    got = check(s, doc, m.LIST, all6)
    assert s.scale_up_plan([queue_index(s, doc)[q] for q in m.LIST], m.LIMIT2)[:4] == [0, 1, 1, 0]
    assert m.HAND_PLANS[m.LIMIT2][:4] == [0, 0, 1, 1] and got[m.LIMIT2].nodes == 5  # (the bins moved, their number not)
    # the rows did not move; two calls return the same bytes
    assert s.node_requested() == before
    lst = [queue_index(s, doc)[q] for q in m.LIST]
    assert raw(s, lst, all6) == raw(s, lst, all6)
    assert s.node_requested() == before


def test_no_side_effects_on_a_queue_run():
    doc = m.dm.cfg2_doc()
    a, b = load(doc), load(doc)
    n = len(doc["queue"])
    lst = list(range(n)) + [0, n - 1]
    a.schedule()
    for q in range(n):  # scale-up calls between the pods of b's run
        b.scale_up(lst, range((17 * q) % 150, (17 * q) % 150 + 40))
        b.scale_up_plan(lst, (29 * q) % 200)
        b.schedule(q, 1)
    assert a.results() == b.results()
    assert a.node_requested() == b.node_requested()
    assert a.scale_up(lst, range(200)) == b.scale_up(lst, range(200))


# ------------------------------------------------------------------ 7: errors and refusals
def bind(s):
    s.L.ksg_scale_up.argtypes = [ctypes.c_void_p, U32P, ctypes.c_uint32, U32P, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.POINTER(_ScaleUp)]
    s.L.ksg_scale_up_plan.argtypes = [ctypes.c_void_p, U32P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.POINTER(ctypes.c_int32)]


def test_errors_leave_the_context_usable():
    doc = m.hand_doc()
    s = load(doc)
    bind(s)
    qi = queue_index(s, doc)
    lst = [qi[q] for q in m.LIST]
    before = raw(s, lst, list(range(6)))
    assert s.n_nodes == 6 and s.queue_len == 13
    pods, bad_pod = (ctypes.c_uint32 * 3)(0, 1, 2), (ctypes.c_uint32 * 3)(0, 13, 2)
    tmpl, bad_tmpl = (ctypes.c_uint32 * 2)(0, 3), (ctypes.c_uint32 * 2)(0, 6)
    out, bins = (_ScaleUp * 2)(), (ctypes.c_int32 * 3)(7, 7, 7)
    out[0].nodes = out[1].nodes = 77
    up, plan = s.L.ksg_scale_up, s.L.ksg_scale_up_plan
    assert up(s.h, pods, 3, tmpl, 2, 4, None) == E_RANGE
    assert up(s.h, None, 3, tmpl, 2, 4, out) == E_RANGE
    assert up(s.h, pods, 3, None, 2, 4, out) == E_RANGE
    assert up(s.h, bad_pod, 3, tmpl, 2, 4, out) == E_RANGE
    assert up(s.h, (ctypes.c_uint32 * 1)(0xFFFFFFFF), 1, tmpl, 2, 4, out) == E_RANGE
    assert up(s.h, pods, 3, bad_tmpl, 2, 4, out) == E_RANGE
    assert up(s.h, pods, 3, tmpl, 2, 0, out) == E_RANGE
    assert up(s.h, pods, 3, tmpl, 2, 1025, out) == E_RANGE
    assert up(s.h, pods, 3, tmpl, 0, 1025, out) == E_RANGE and up(s.h, bad_pod, 3, tmpl, 0, 4, out) == E_RANGE
    assert plan(s.h, pods, 3, 0, 4, None) == E_RANGE
    assert plan(s.h, None, 3, 0, 4, bins) == E_RANGE
    assert plan(s.h, bad_pod, 3, 0, 4, bins) == E_RANGE
    assert plan(s.h, pods, 3, 6, 4, bins) == E_RANGE
    assert plan(s.h, pods, 3, 0, 0, bins) == E_RANGE and plan(s.h, pods, 3, 0, 2048, bins) == E_RANGE
    # zero counts: KSG_OK; no template, nothing written; no pod, nothing for a plan to write
    assert up(s.h, pods, 3, tmpl, 0, 4, out) == 0 and up(s.h, pods, 3, None, 0, 4, None) == 0
    assert plan(s.h, pods, 0, 0, 4, bins) == 0 and plan(s.h, None, 0, 0, 4, None) == 0
    assert [out[0].nodes, out[1].nodes] == [77, 77] and list(bins) == [7, 7, 7]  # untouched throughout
    assert up(s.h, None, 0, tmpl, 2, 4, out) == 0
    assert [(o.nodes, o.packed, o.first_unpacked, o.base_pods, o.reserved) for o in out] == [(0, 0, -1, 0, 0)] * 2
    assert raw(s, lst, list(range(6))) == before
    s.schedule()  # the context goes on working
    assert len(s.results()) == 13 and sum(r.status == 0 and r.selected >= 0 for r in s.results()) >= 8


def refused(doc, match, **kw):
    s = Scheduler(doc["profile"], **kw)
    s.load_cluster(doc)
    bind(s)
    out = (_ScaleUp * 1)()
    out[0].nodes = 77
    one = (ctypes.c_uint32 * 1)(0)
    assert s.L.ksg_scale_up(s.h, one, 1, one, 1, 4, out) == E_INVALID and out[0].nodes == 77
    assert s.L.ksg_scale_up(s.h, one, 1, one, 1, 4, None) == E_INVALID  # (the refusal comes before the arguments)
    for call in (lambda: s.scale_up([0], [0]), lambda: s.scale_up_plan([0], 0)):
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
    refused(nofit, "NodeResourcesFit")
    refused(bf.cfg2_doc(), "sharded", shard_rank=0, shard_count=2)
