"""GPU parity of the persistent window loop's hand-over of P_W from the replay to
the evaluation.

The replay of k_window_run stores P_W one 64-bit word per thread, with node -1 in
the entries it does not use, and the eval blocks read the whole of P_{E-2} (nodes
and after rows) into LDS beside their first row load, without its count; a node of
the list is evaluated on its row from LDS.  Every case
compares (selected, feasible, status) of every pod with the CPU oracle, with one
and with two replay blocks, and (but for the forced fallback) checks that the
persistent loop really ran; where outputs are kept, the annotations as well.
"""
import pytest

from _oracle import Oracle
from ksg import Scheduler, generator as g

R2 = ["0", "1"]
FIT_BA = [("NodeResourcesFit", 1), ("NodeResourcesBalancedAllocation", 1)]
STATIC_PROFILE = [("TaintToleration", 3), ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                  ("NodeResourcesBalancedAllocation", 1)]
WINDOW = 32
STAGE = 4  # KSG_STAGE: the candidate ranks whose rows the record carries
ONE_TILE, TWO_TILES = 300, 1027  # (1,024 nodes per tile: the second tile holds 3 < STAGE nodes)

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


def _run(monkeypatch, r2, doc, want, keep=False, expect_run=True):
    monkeypatch.setenv("KSG_WIN_REPLAY2", r2)
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    assert s.batch_path
    if keep:
        s.keep_outputs(0, s.queue_len)
    before = s.window_runs()
    s.schedule()
    _check(s, want)
    assert (s.window_runs() > before) == expect_run
    return s


def _same_annotations(s, o, pods):
    for q in pods:
        a, b = s.annotations(q), o.annotations(q)
        for k in b:
            assert a.get(k) == b[k], f"pod {q} annotation {k}:\n gpu    {a.get(k)[:300]}\n oracle {b[k][:300]}"


def _window_picks(want):
    out = []
    for w0 in range(0, len(want), WINDOW):
        out.append({sel for sel, _, _ in want[w0:w0 + WINDOW] if sel >= 0})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("r2", R2)
@pytest.mark.parametrize("n_pods", [1, 33, 70, 160])
@pytest.mark.parametrize("n_nodes", [ONE_TILE, TWO_TILES])
def test_tiles_and_short_windows(monkeypatch, r2, n_nodes, n_pods):
    """One tile and two tiles (the second nearly empty: fewer nodes than
    KSG_STAGE); queues whose last window is short in either parity (1, 33, 70
    pods), so a P list of fewer than 32 entries, filled up with -1, lands in both
    slots, and five whole windows (160).  Two tiles, 70 pods: outputs kept."""
    doc, o, want = _case(("cfg2", n_nodes, n_pods), lambda: g.generate(2, n_nodes=n_nodes, n_pods=n_pods), record=3)
    keep = n_nodes == TWO_TILES and n_pods == 70
    s = _run(monkeypatch, r2, doc, want, keep=keep)
    if keep:
        _same_annotations(s, o, range(0, s.queue_len, 9))


def _few_feasible_doc():
    """1,027 nodes too small for any pod but three of 20 pods each, one of them in the
    second tile: every pod has at most 3 < KSG_STAGE feasible nodes (empty candidate
    ranks, zero rows in the record), pods 10 and 40 fit nowhere, and the 60 slots
    run out inside the last window of 70 pods."""
    nodes = [g.node_obj(f"node-{i:04d}", 50, 64 * g.Mi, pods=8) for i in range(TWO_TILES)]
    for i in (5, 700, 1025):
        nodes[i] = g.node_obj(f"node-{i:04d}", 64000 + 1000 * (i % 7), (128 + i % 5) * g.Gi, pods=20)
    queue = []
    for j in range(70):
        cpu = 10 ** 6 if j in (10, 40) else 100 + 10 * (j % 7)
        queue.append(g.pod_obj(f"pod-{j:03d}", [g.req(cpu, (128 + 64 * (j % 3)) * g.Mi)]))
    return {"profile": g.make_profile(FIT_BA, 5), "nodes": nodes, "pods": [], "queue": queue}


@pytest.mark.gpu
@pytest.mark.parametrize("r2", R2)
def test_fewer_feasible_nodes_than_staged_ranks(monkeypatch, r2):
    doc, o, want = _case("few-feasible", _few_feasible_doc, record=3)
    assert all(0 <= w[1] < STAGE for w in want)
    assert want[10] == (-1, 0, 1) and want[40] == (-1, 0, 1)
    assert want[0][1] == 3 and want[69] == (-1, 0, 1)
    assert {w[0] for w in want if w[0] >= 0} == {5, 700, 1025}
    s = _run(monkeypatch, r2, doc, want, keep=True)
    _same_annotations(s, o, (0, 9, 10, 11, 33, 40, 64, 69))


def _tight_cfg2(n_nodes=48, n_pods=224, seed=11):
    """cfg2's nodes and pods on nodes that hold 3..7 pods: the cluster fills up, and
    the nodes a window modified are among the best of the window after the next."""
    doc = g.generate(2, n_nodes=n_nodes, n_pods=n_pods)
    r = g.Rng(seed)
    for n in doc["nodes"]:
        cap = str(3 + r.below(5))
        n["status"]["allocatable"]["pods"] = cap
        n["status"]["capacity"]["pods"] = cap
    return doc


@pytest.mark.gpu
@pytest.mark.parametrize("r2", R2)
def test_saturating_cluster_rows_from_the_list(monkeypatch, r2):
    """48 nodes: nearly every node is in P_{E-2}, so the rows the tiles evaluate on
    are the list's after rows from LDS; the oracle shows nodes picked again two
    windows after a window modified them, and the cluster running full."""
    doc, o, want = _case("tight-cfg2", _tight_cfg2)
    picks = _window_picks(want)
    assert sum(1 for w in range(len(picks) - 2) if picks[w] & picks[w + 2]) >= 3
    assert sum(1 for w in want if w[2] == 1) > 10, "the cluster should saturate"
    _run(monkeypatch, r2, doc, want)


@pytest.mark.gpu
@pytest.mark.parametrize("r2", R2)
def test_two_passes_on_one_context(monkeypatch, r2):
    """reset() and schedule() again: the second pass meets the first one's P lists
    (a short list's stale entries behind it)."""
    for key, make in (("few-feasible", _few_feasible_doc),
                      (("cfg2", TWO_TILES, 70), lambda: g.generate(2, n_nodes=TWO_TILES, n_pods=70))):
        doc, o, want = _case(key, make, record=3)
        s = _run(monkeypatch, r2, doc, want)
        before = s.window_runs()
        s.reset()
        s.schedule()
        _check(s, want)
        assert s.window_runs() > before


def _fallback_doc():
    """Pod 0 is pinned (required NodeAffinity) on node 17, which then holds no more
    pods; node 17 is the only node with an untolerated PreferNoSchedule taint, so the
    later pods' NormalizeScore max drops: the exact re-evaluation, in windows 0, 1
    and 2 (70 pods)."""
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
@pytest.mark.parametrize("r2", R2)
def test_cfg3_small_and_normaliser_fallback(monkeypatch, r2):
    """The static variant of the loop: a small cfg3 queue over two tiles (three
    windows), and the normaliser fallback with kept outputs."""
    doc, o, want = _case(("cfg3", 1100, 96), lambda: g.generate(3, n_nodes=1100, n_pods=96))
    _run(monkeypatch, r2, doc, want)
    doc, o, want = _case("fallback", _fallback_doc, record=3)
    assert want[0][0] == 17
    s = _run(monkeypatch, r2, doc, want, keep=True)
    _same_annotations(s, o, (1, 33, 40, 69))


@pytest.mark.gpu
@pytest.mark.parametrize("r2", R2)
def test_two_nodes_per_thread(monkeypatch, r2):
    """7,200 nodes: 32 pods x 8 tiles of 1,024 nodes and a replay block exceed the
    256 compute units, so a thread holds two nodes (four tiles per pod): the second
    node's lookup in the list and its row from LDS, beside the next row's load."""
    doc, o, want = _case(("cfg2", 7200, 70), lambda: g.generate(2, n_nodes=7200, n_pods=70))
    _run(monkeypatch, r2, doc, want)


@pytest.mark.gpu
def test_forced_fallback_to_launch_per_window(monkeypatch):
    """A grid that is never all resident (KSG_RUN_NORES=1): the loop leaves at the
    handshake and the launch-per-window loop, which goes by the lists' counts and not
    by the -1 entries the host wrote for the loop, computes the same."""
    monkeypatch.setenv("KSG_RUN_NORES", "1")
    doc, o, want = _case(("cfg2", TWO_TILES, 70), lambda: g.generate(2, n_nodes=TWO_TILES, n_pods=70), record=3)
    _run(monkeypatch, "1", doc, want, expect_run=False)
