"""GPU parity of the persistent window loop with two replay blocks.

KSG_WIN_REPLAY2=1 lets blocks 0 and 1 of k_window_run replay the even and the
odd windows in turn; the replay of W then waits for the other block's publish of
W-1 before it reads P_{W-1}.  Every case compares (selected, feasible, status)
of every pod with the CPU oracle, with one and with two replay blocks, and (but
for the forced fallback) checks that the persistent loop really ran.
"""
import json

import pytest

from _oracle import Oracle
from ksg import Scheduler, generator as g

# KSG_WIN_REPLAY2 is the loop's only switch: the environment of a case is its r2
# value.  The mb / pfix / one-counter parts of the ids name merge-block, prior-step
# and one-counter arms that are retired (nothing reads them); they select nothing,
# so the six ids of one r2 value run the same loop as r2=*-mb=0-pfix=1.
IDS = [f"r2={r2}-mb={mb}-pfix={pf}" for r2 in "01" for mb, pf in ("00", "10", "01", "11")]
IDS += [f"r2={r2}-mb={mb}-pfix=0-one-counter" for r2 in "01" for mb in "01"]
ENVS = [{"KSG_WIN_REPLAY2": i[3]} for i in IDS]
STATIC_PROFILE = [("TaintToleration", 3), ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                  ("NodeResourcesBalancedAllocation", 1)]

_docs = {}


def _case(key, make, record=0):
    """The document and its oracle pass, computed once per module and left unchanged."""
    if key not in _docs:
        doc = make()
        o = Oracle(doc)
        o.schedule(record=record)
        _docs[key] = (doc, o)
    return _docs[key]


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _results(s):
    return [(r.selected, r.feasible, r.status) for r in s.results()]


def _check(s, o):
    got = _results(s)
    want = [o.result(q) for q in range(len(got))]
    bad = [q for q in range(len(got)) if got[q] != want[q]]
    assert not bad, f"{len(bad)} pods differ, first {[(q, got[q], want[q]) for q in bad[:5]]}"
    return want


def _run(doc, o, keep=False, expect_run=True):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    assert s.batch_path
    if keep:
        s.keep_outputs(0, s.queue_len)
    before = s.window_runs()
    s.schedule()
    want = _check(s, o)
    assert (s.window_runs() > before) == expect_run
    return s, want


def _tight_cfg2(n_nodes=60, n_pods=300, seed=7):
    """cfg2's nodes and pods on nodes that hold 3..7 pods: the cluster fills up, a
    window's pods crowd onto the few nodes left and the replay iterates."""
    doc = g.generate(2, n_nodes=n_nodes, n_pods=n_pods)
    r = g.Rng(seed)
    for n in doc["nodes"]:
        cap = str(3 + r.below(5))
        n["status"]["allocatable"]["pods"] = cap
        n["status"]["capacity"]["pods"] = cap
    return doc


def _fallback_doc(kind):
    """Pod 0 is pinned (required NodeAffinity) on node 17, which then holds no more
    pods; node 17 is the only node at the later pods' static max (the only node
    with an untolerated PreferNoSchedule taint, or the only node their preference
    matches), so their NormalizeScore max drops: the exact re-evaluation, in
    windows 0, 1 and 2 (70 pods) — on both replay blocks."""
    nodes = []
    for i in range(40):
        labels = {"slot": f"s{i}"}
        taints = None
        pods = 8
        if i == 17:
            pods = 1
            labels["special"] = "yes"
            if kind == "taint":
                taints = [{"key": "t", "value": "v", "effect": "PreferNoSchedule"}]
        nodes.append(g.node_obj(f"node-{i:03d}", 4000, 8 * g.Gi, pods=pods, labels=labels, taints=taints))
    pin = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {
        "nodeSelectorTerms": [{"matchExpressions": [{"key": "special", "operator": "In", "values": ["yes"]}]}]}}}
    pref = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": 50, "preference": {"matchExpressions": [{"key": "special", "operator": "Exists"}]}}]}}
    queue = [g.pod_obj("pod-000", [g.req(100, 128 * g.Mi)], affinity=pin)]
    for j in range(1, 70):
        extra = {"affinity": pref} if kind == "na" else {}
        queue.append(g.pod_obj(f"pod-{j:03d}", [g.req(100 + 10 * (j % 7), 128 * g.Mi)], **extra))
    return {"profile": g.make_profile(STATIC_PROFILE, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=IDS)
@pytest.mark.parametrize("n_pods", [32, 64, 96, 133])
def test_cfg2_one_tile(monkeypatch, env, n_pods):
    """300 nodes (one tile per pod).  32 pods: one window, block 1 idle; 64: each
    block replays once; 96: an odd window count; 133: five windows, the short last
    one on block 0."""
    _setenv(monkeypatch, env)
    doc, o = _case(("cfg2", 300, n_pods), lambda: g.generate(2, n_nodes=300, n_pods=n_pods))
    _run(doc, o)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_cfg2_two_tiles_kept_outputs(monkeypatch, env):
    """1,500 nodes (two tiles), 160 pods, every pod's outputs kept: the kept patches
    of window W are written while W+1 replays.  Annotations of every 7th pod."""
    _setenv(monkeypatch, env)
    doc, o = _case(("cfg2", 1500, 160), lambda: g.generate(2, n_nodes=1500, n_pods=160), record=3)
    s, _ = _run(doc, o, keep=True)
    for q in range(0, s.queue_len, 7):
        a, b = s.annotations(q), o.annotations(q)
        for k in b:
            assert a.get(k) == b[k], f"pod {q} annotation {k}:\n gpu    {a.get(k)[:300]}\n oracle {b[k][:300]}"


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_cfg2_saturating_cluster(monkeypatch, env):
    """60 nodes of 3..7 pods each, 300 pods: full P lists, nodes picked several times
    in a window, several Jacobi iterations, replays of varying length (the two
    blocks drift against each other).  The oracle leaves 76 pods unschedulable."""
    _setenv(monkeypatch, env)
    doc, o = _case("tight-cfg2", _tight_cfg2)
    _, want = _run(doc, o)
    assert sum(1 for w in want if w[2] == 1) > 20, "the cluster should saturate"


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_two_passes_on_one_context(monkeypatch, env):
    """reset() and schedule() again: the loop's counters are zeroed per launch."""
    _setenv(monkeypatch, env)
    doc, o = _case(("cfg2", 300, 133), lambda: g.generate(2, n_nodes=300, n_pods=133))
    s, _ = _run(doc, o)
    before = s.window_runs()
    s.reset()
    s.schedule()
    _check(s, o)
    assert s.window_runs() > before


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_cfg3_small_and_normaliser_fallback(monkeypatch, env):
    """Taint / NodeAffinity profiles: a small cfg3 queue (three windows), and the
    normaliser fallback (win_exact_select / win_exact_write) in windows of both
    parities, with the annotations of the pods whose normaliser dropped."""
    _setenv(monkeypatch, env)
    doc, o = _case(("cfg3", 400, 96), lambda: g.generate(3, n_nodes=400, n_pods=96))
    _run(doc, o)
    for kind in ("taint", "na"):
        doc, o = _case(("fallback", kind), lambda: _fallback_doc(kind), record=3)
        s, _ = _run(doc, o, keep=True)
        assert o.result(0)[0] == 17
        plugin = "TaintToleration" if kind == "taint" else "NodeAffinity"
        for q in (1, 33, 40, 69):  # (windows 0, 1, 1 and 2)
            a, b = s.annotations(q), o.annotations(q)
            for k in b:
                assert a.get(k) == b[k], f"{kind} pod {q} annotation {k}"
            fin = json.loads(a["kube-scheduler-simulator.sigs.k8s.io/finalscore-result"])
            # with node 17 full, every feasible node has the same raw score: the exact max is 0
            assert len({v[plugin] for v in fin.values()}) == 1


@pytest.mark.gpu
def test_forced_fallback_to_launch_per_window(monkeypatch):
    """A grid that is never all resident (KSG_RUN_NORES=1): the loop leaves at the
    handshake before any state changes and the launch-per-window loop runs."""
    monkeypatch.setenv("KSG_WIN_REPLAY2", "1")
    monkeypatch.setenv("KSG_RUN_NORES", "1")
    doc, o = _case(("cfg2", 300, 133), lambda: g.generate(2, n_nodes=300, n_pods=133))
    _run(doc, o, expect_run=False)
