"""GPU parity of the window replay's core: the starting guess, the per-pick row
table and the paired phase B of win_fixup.

Every case is one tile, built so that the CPU oracle's own pass shows the
property it is about (asserted from the oracle's results where they show it),
and runs three arms: the persistent loop with one and with two replay blocks,
and the launch-per-window loop.  (selected, feasible, status) of every pod
equal the oracle's; where outputs are kept, so do the annotations.
"""
import json

import pytest

from _oracle import Oracle
from ksg import Scheduler, generator as g

ARMS = {"r2=0": {"KSG_WIN_REPLAY2": "0"}, "r2=1": {"KSG_WIN_REPLAY2": "1"}, "per-window": {"KSG_WIN_RUN": "0"}}
FIT_BA = [("NodeResourcesFit", 1), ("NodeResourcesBalancedAllocation", 1)]
STATIC_PROFILE = [("TaintToleration", 3), ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                  ("NodeResourcesBalancedAllocation", 1)]
FINAL = "kube-scheduler-simulator.sigs.k8s.io/finalscore-result"
WINDOW = 32

_docs = {}


def _case(key, make, record=0):
    """The document and its oracle pass, computed once per module and left unchanged."""
    if key not in _docs:
        doc = make()
        o = Oracle(doc)
        o.schedule(record=record)
        _docs[key] = (doc, o, [o.result(q) for q in range(len(doc["queue"]))])
    return _docs[key]


def _check(s, want):
    got = [(r.selected, r.feasible, r.status) for r in s.results()]
    bad = [q for q in range(len(want)) if got[q] != want[q]]
    assert not bad, f"{len(bad)} pods differ, first {[(q, got[q], want[q]) for q in bad[:5]]}"


def _run(monkeypatch, arm, doc, want, keep=False):
    for k, v in ARMS[arm].items():
        monkeypatch.setenv(k, v)
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    assert s.batch_path
    if keep:
        s.keep_outputs(0, s.queue_len)
    before = s.window_runs()
    s.schedule()
    _check(s, want)
    if arm != "per-window":
        assert s.window_runs() > before
    return s


def _same_annotations(s, o, pods):
    for q in pods:
        a, b = s.annotations(q), o.annotations(q)
        for k in b:
            assert a.get(k) == b[k], f"pod {q} annotation {k}:\n gpu    {a.get(k)[:300]}\n oracle {b[k][:300]}"


def _window_picks(want):
    """Per window: node -> how many of the window's pods the oracle placed on it."""
    out = []
    for w0 in range(0, len(want), WINDOW):
        c = {}
        for sel, _, _ in want[w0:w0 + WINDOW]:
            if sel >= 0:
                c[sel] = c.get(sel, 0) + 1
        out.append(c)
    return out


def _ordered_doc(n_pods):
    """38 nodes of 125n millicores and 256n MiB each, identical pods of 1000m / 2 GiB:
    both resources are used in the same proportion on every node (BalancedAllocation
    is 100 everywhere) and n is chosen so that NodeResourcesFit's score of an empty
    node is another integer for every node.  No two nodes tie, so all pods of the
    first window rank the nodes alike: each round of the guess they all propose the
    same node, one pod keeps it and the rest move on, the longest chain there is."""
    ns = []
    for t in range(50, 3, -1):
        n = -(-800 // t)
        if -(-800 // n) == t and n not in ns:
            ns.append(n)
    nodes = [g.node_obj(f"node-{i:03d}", 125 * n, n * 256 * g.Mi, pods=8) for i, n in enumerate(ns)]
    queue = [g.pod_obj(f"pod-{j:03d}", [g.req(1000, 2 * g.Gi)]) for j in range(n_pods)]
    return {"profile": g.make_profile(FIT_BA, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("n_pods", [33, 63, 64])
def test_maximal_guess_depth(monkeypatch, arm, n_pods):
    """One full window, then a window of 1, of 31 or of 32 pods."""
    doc, o, want = _case(("ordered", n_pods), lambda: _ordered_doc(n_pods), record=3)
    fin = json.loads(o.annotations(0)[FINAL])
    totals = [sum(int(x) for x in v.values()) for v in fin.values()]
    assert len(totals) == len(doc["nodes"]) >= WINDOW and len(set(totals)) == len(totals), "the first window's scores tie"
    _run(monkeypatch, arm, doc, want)


def _crowded_doc():
    """Five large nodes of 8 pods each among 60 nodes too small for any pod: the 32
    pods of the first window share five nodes."""
    nodes = [g.node_obj(f"node-{i:03d}", 50, 64 * g.Mi, pods=8) for i in range(60)]
    for i in (3, 17, 29, 41, 58):
        nodes[i] = g.node_obj(f"node-{i:03d}", 16000 + 1000 * (i % 7), (32 + i % 5) * g.Gi, pods=8)
    queue = [g.pod_obj(f"pod-{j:03d}", [g.req(100 + 10 * (j % 7), (128 + 64 * (j % 3)) * g.Mi)]) for j in range(45)]
    return {"profile": g.make_profile(FIT_BA, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_node_picked_several_times_in_a_window(monkeypatch, arm):
    doc, o, want = _case("crowded", _crowded_doc)
    assert max(max(c.values()) for c in _window_picks(want) if c) >= 3, "no node is picked three times in a window"
    _run(monkeypatch, arm, doc, want)


def _tight_cfg2(n_nodes=60, n_pods=300, seed=7):
    """cfg2's nodes and pods on nodes that hold 3..7 pods: the cluster fills up, a
    window's pods crowd onto the few nodes left (candidates of deep ranks, nodes of
    the previous window's list) and the replay iterates."""
    doc = g.generate(2, n_nodes=n_nodes, n_pods=n_pods)
    r = g.Rng(seed)
    for n in doc["nodes"]:
        cap = str(3 + r.below(5))
        n["status"]["allocatable"]["pods"] = cap
        n["status"]["capacity"]["pods"] = cap
    return doc


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_deep_ranks_and_previous_window_nodes(monkeypatch, arm):
    """Ten windows; with two replay blocks every pod's outputs are kept.  That a pick
    comes from a candidate rank >= KSG_STAGE cannot be read from the oracle's results
    (it keeps no ranking): the crowding onto few nodes gives such picks by
    construction only; what the oracle does show, picks on the previous window's
    nodes, is asserted."""
    doc, o, want = _case("tight-cfg2", _tight_cfg2, record=3)
    assert len(want) >= 5 * WINDOW
    # nodes picked again in the window after the one that modified them
    picks = _window_picks(want)
    assert any(set(picks[w]) & set(picks[w + 1]) for w in range(len(picks) - 1))
    keep = arm == "r2=1"
    s = _run(monkeypatch, arm, doc, want, keep=keep)
    if keep:
        _same_annotations(s, o, range(0, s.queue_len, 7))


def _saturating_doc():
    """10 nodes of 5 pods each, 100 pods: the 50 slots run out at pod 50, inside the
    second window."""
    nodes = [g.node_obj(f"node-{i:03d}", 8000 + 500 * i, (16 + i) * g.Gi, pods=5) for i in range(10)]
    queue = [g.pod_obj(f"pod-{j:03d}", [g.req(100 + 10 * (j % 5), 128 * g.Mi)]) for j in range(100)]
    return {"profile": g.make_profile(FIT_BA, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_saturation_inside_a_window(monkeypatch, arm):
    doc, o, want = _case("saturating", _saturating_doc)
    first = next(q for q, w in enumerate(want) if w[0] < 0)
    assert first % WINDOW != 0 and first + WINDOW < len(want)
    assert all(w[0] >= 0 and w[2] == 0 for w in want[:first])
    assert all(w == (-1, 0, 1) for w in want[first:])
    _run(monkeypatch, arm, doc, want)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_two_passes_on_one_context(monkeypatch, arm):
    doc, o, want = _case(("ordered", 63), lambda: _ordered_doc(63), record=3)
    s = _run(monkeypatch, arm, doc, want)
    before = s.window_runs()
    s.reset()
    s.schedule()
    _check(s, want)
    if arm != "per-window":
        assert s.window_runs() > before


def _static_fallback_doc():
    """Pod 0 is pinned (required NodeAffinity) on node 17, which then holds no more
    pods; node 17 is the only node with an untolerated PreferNoSchedule taint, so the
    later pods' NormalizeScore max drops: the exact re-evaluation, whose picks come
    from the node rows, in windows 0, 1 and 2 (70 pods)."""
    nodes = []
    for i in range(40):
        labels = {"slot": f"s{i}"}
        taints = None
        pods = 8
        if i == 17:
            pods = 1
            labels["special"] = "yes"
            taints = [{"key": "t", "value": "v", "effect": "PreferNoSchedule"}]
        nodes.append(g.node_obj(f"node-{i:03d}", 4000, 8 * g.Gi, pods=pods, labels=labels, taints=taints))
    pin = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {
        "nodeSelectorTerms": [{"matchExpressions": [{"key": "special", "operator": "In", "values": ["yes"]}]}]}}}
    queue = [g.pod_obj("pod-000", [g.req(100, 128 * g.Mi)], affinity=pin)]
    for j in range(1, 70):
        queue.append(g.pod_obj(f"pod-{j:03d}", [g.req(100 + 10 * (j % 7), 128 * g.Mi)]))
    return {"profile": g.make_profile(STATIC_PROFILE, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_static_profile_fallback_picks(monkeypatch, arm):
    doc, o, want = _case("static-fallback", _static_fallback_doc, record=3)
    assert want[0][0] == 17
    # identical nodes: a window's pods come back to the nodes its earlier pods picked
    assert max(max(c.values()) for c in _window_picks(want)) >= 2
    s = _run(monkeypatch, arm, doc, want, keep=True)
    _same_annotations(s, o, (1, 33, 40, 69))
    for q in (1, 33, 69):  # with node 17 full every feasible node has the same raw score: the exact max is 0
        fin = json.loads(s.annotations(q)[FINAL])
        assert len({v["TaintToleration"] for v in fin.values()}) == 1
