"""Ranked candidates (ksg_ranked_nodes / Scheduler.ranked_nodes): the K best
feasible nodes of a kept pod's cycle, selected on the device, in the engine's own
selection order.

The expected list never comes from the call under test.  It comes from a host
model in this file: the pod's filter codes and, per scoring position, its
normalized scores x the framework weight, summed; the selection key
(total << 40 | (0xFFFFF - h20) << 20 | node, h20 the seeded
splitmix64 tie-break hash) restated here; the feasible nodes' keys sorted
descending.  The model is pinned first, for every pod of every case, by its own
top entry being the pod's (selected, total), which the parity tests check against
the oracle: a cluster that breaks that self-check is a wrong input, not a finding.
"""
import copy
import ctypes
import functools

import pytest

from ksg import Scheduler, generator as g
from ksg.engine import FILTER_PASSED, _RankedNode
from test_plugin_api_gpu import CASES, SCORERS

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
E_STATE, E_RANGE = -3, -4
C_SUCCESS = 0


def splitmix64(x):
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pack_key(total, seed, qidx, node):
    h20 = splitmix64((seed ^ ((qidx * GOLDEN) & M64) ^ node) & M64) >> 44
    return (total << 40) | ((0xFFFFF - h20) << 20) | node


@functools.lru_cache(maxsize=None)
def _doc(c, sizes):
    return g.generate(c, **dict(sizes))


def family(name):
    _, c, sizes = next(x for x in CASES if x[0] == name)
    return _doc(c, tuple(sorted(sizes.items())))


def model(s, q, doc, r):
    """[(node, total)] of every feasible node of kept pod q, best first; r its result.
    Pinned by its own top entry: (r.selected, r.total) of a scheduled pod."""
    if r.status == 2:  # the cycle ended in an error: nothing is ranked
        return []
    feas = [i for i, c in enumerate(s.filter_codes(q)) if c == FILTER_PASSED]
    assert len(feas) == r.feasible, (q, len(feas), r)
    total = dict.fromkeys(feas, 0)
    if len(feas) > 1:  # (a single feasible node: upstream runs no scoring)
        for pos, pl in enumerate(doc["profile"]["plugins"]):
            if pl in SCORERS and s.prescore_status(q, pos)[0] == C_SUCCESS or pl == "ImageLocality":
                norm, w = s.normalized_scores(q, pos), s.plugin_weights(pos)[0]
                for i in feas:
                    total[i] += norm[i] * w
    keys = sorted((pack_key(total[i], doc["profile"]["seed"], q, i) for i in feas), reverse=True)
    assert len(set(keys)) == len(keys)
    ranked = [(k & 0xFFFFF, k >> 40) for k in keys]
    if r.status == 0:
        assert ranked and ranked[0] == (r.selected, r.total), ("model self-check", q, ranked[:2], r)
    else:
        assert not ranked, ("model self-check", q, r)
    return ranked


def check(s, q, doc, r, ks):
    want = model(s, q, doc, r)
    for k in ks:
        got = s.ranked_nodes(q, k)
        assert len(got) == min(k, max(r.feasible, 0) if r.status != 2 else 0), (q, k, got, r)
        assert got == want[:k], (q, k, got, want[:k])
    return want


def queue_run(doc, keep=None):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(0, len(doc["queue"]) if keep is None else keep)
    s.schedule()
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_families_queue_mode(name):
    """cfg1..cfg4 at the plugin-API sizes, queue mode, every pod's outputs kept:
    k = 1, 3 and KSG_RANK_MAX against the model, for every pod."""
    doc = family(name)
    s = queue_run(doc)
    res = s.results()
    assert len(res) == len(doc["queue"])
    many = 0
    for q, r in enumerate(res):
        want = check(s, q, doc, r, (1, 3, 64))
        many += len(want) > 3
    assert many >= len(res) // 2  # the case ranks: most pods have more than three candidates


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,tile,n_pods", [(127, "128", 8), (128, "128", 8), (129, "128", 8), (1000, "128", 8),
                                                 (5000, None, 1)])
def test_tile_edges_and_merge_levels(monkeypatch, n_nodes, tile, n_pods):
    """KSG_RANK_TILE=128: one tile short by a node, one full tile, one node into a
    second tile, and 1000 nodes = 8 tiles, three merge levels; then 5,000 nodes at
    the default tile (three tiles, one merge)."""
    if tile is None:
        monkeypatch.delenv("KSG_RANK_TILE", raising=False)
    else:
        monkeypatch.setenv("KSG_RANK_TILE", tile)
    doc = _doc(2, (("n_nodes", n_nodes), ("n_pods", n_pods)))
    s = queue_run(doc)
    for q, r in enumerate(s.results()):
        want = check(s, q, doc, r, (64,))
        assert len(want) > 64  # more candidates than the call returns: the select chooses


def tied_doc(n_nodes=300, n_pods=6):
    """cfg2 with every node a copy of node 0 (and of its filler pod) under its own name."""
    base = _doc(2, (("n_nodes", n_nodes), ("n_pods", n_pods)))
    doc = dict(base, nodes=[], pods=[])
    n0 = base["nodes"][0]
    fill = [p for p in base["pods"] if p["spec"].get("nodeName") == n0["metadata"]["name"]]
    for i in range(n_nodes):
        n = copy.deepcopy(n0)
        name = f"node-{i:07d}"
        n["metadata"]["name"] = name
        n["metadata"]["labels"][g.HOSTNAME] = name
        doc["nodes"].append(n)
        for p in fill:
            p = copy.deepcopy(p)
            p["metadata"]["name"] = f"fill-{i:07d}"
            p["spec"]["nodeName"] = name
            doc["pods"].append(p)
    return doc


@pytest.mark.gpu
def test_all_ties(monkeypatch):
    """300 identical nodes, three tiles of 128: the first pod's totals all tie, so
    its order is the hash order alone; later pods mix ties and non-ties."""
    monkeypatch.setenv("KSG_RANK_TILE", "128")
    doc = tied_doc()
    s = queue_run(doc)
    res = s.results()
    first = model(s, 0, doc, res[0])
    assert len(first) == 300 and len({t for _, t in first}) == 1
    mixed = 0
    for q, r in enumerate(res):
        want = check(s, q, doc, r, (3, 64))
        mixed += len({t for _, t in want}) > 1
    assert mixed >= 1


@pytest.mark.gpu
def test_fewer_feasible_than_k():
    """Pods that fit 5 nodes, then 1 node (upstream's single-feasible shortcut: no
    scoring, the total from the summary), then none (unschedulable)."""
    base = _doc(2, (("n_nodes", 40), ("n_pods", 3)))
    doc = dict(base, nodes=copy.deepcopy(base["nodes"]), pods=[], queue=[])
    for i, n in enumerate(doc["nodes"]):  # allocatable by hand: 1 cpu, but 4 on four nodes and 16 on one
        cpu = "16" if i == 17 else "4" if i in (3, 11, 26, 38) else "1"
        for k in ("allocatable", "capacity"):
            n["status"][k]["cpu"] = cpu
            n["status"][k]["memory"] = "32Gi"
    for j, cpu in enumerate((2000, 10000, 64000)):
        doc["queue"].append(g.pod_obj(f"pod-{j:07d}", [g.req(cpu, 64 * g.Mi)]))
    s = queue_run(doc)
    res = s.results()
    assert [(r.feasible, r.status) for r in res] == [(5, 0), (1, 0), (0, 1)]
    assert sorted(n for n, _ in check(s, 0, doc, res[0], (1, 3, 5, 64))) == [3, 11, 17, 26, 38]
    assert check(s, 1, doc, res[1], (1, 64)) == [(17, res[1].total)]
    assert res[1].selected == 17
    assert check(s, 2, doc, res[2], (1, 64)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("commit", [False, True], ids=["plugin", "harness"])
@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_cycle_mode(name, commit):
    """ksg_cycle with either commit value (cfg2: the cycle's k_eval writes the view
    itself; cfg4: k_view): the list against the model, and unchanged by the Reserve
    that follows a commit = 0 cycle."""
    doc = family(name)
    s = Scheduler(doc["profile"])
    s.load_cluster(dict(doc, queue=[]))
    ranked = 0
    for pod in doc["queue"][:20]:
        q, r = s.cycle(pod, commit=commit)
        want = check(s, q, doc, r, (3, 64))
        ranked += len(want) > 1
        if not commit and r.selected >= 0:
            s.reserve(q, r.selected)
            assert s.ranked_nodes(q, 64) == want[:64], q
            assert s.ranked_nodes(q, 3) == want[:3], q
    assert ranked >= 10


def _raw(s, q, k, cap=64):
    out = (_RankedNode * cap)()
    n = ctypes.c_uint32(99)
    return s.L.ksg_ranked_nodes(s.h, q, k, out, ctypes.byref(n)), n.value


@pytest.mark.gpu
def test_errors_leave_the_context_usable():
    doc = _doc(2, (("n_nodes", 60), ("n_pods", 4)))
    s = queue_run(doc, keep=2)
    res = s.results()
    good = s.ranked_nodes(0, 3)
    assert good == model(s, 0, doc, res[0])[:3]
    assert _raw(s, 0, 0) == (E_RANGE, 0)
    assert _raw(s, 0, 65, cap=65) == (E_RANGE, 0)
    assert _raw(s, s.queue_len, 3) == (E_RANGE, 0)
    out = (_RankedNode * 4)()
    assert s.L.ksg_ranked_nodes(s.h, 0, 3, None, ctypes.byref(ctypes.c_uint32())) == E_RANGE
    assert s.L.ksg_ranked_nodes(s.h, 0, 3, out, None) == E_RANGE
    # a pod whose outputs were not kept: what ksg_normalized_scores answers for it
    arr = (ctypes.c_int64 * s.n_nodes)()
    norm_rc = s.L.ksg_normalized_scores(s.h, 3, 0, arr, s.n_nodes)
    assert norm_rc == E_STATE
    assert _raw(s, 3, 3) == (norm_rc, 0)
    assert b"not kept" in s.L.ksg_last_error(s.h)
    # the context is still usable, and the answer is the same
    assert s.ranked_nodes(0, 3) == good
    assert s.ranked_nodes(1, 64) == model(s, 1, doc, res[1])[:64]


@pytest.mark.gpu
def test_no_side_effects():
    """cfg4 scheduled cycle by cycle, once plainly and once with ranked_nodes after
    every cycle: the same results and node rows; two calls on a pod, the same list."""
    doc = family("cfg4")
    runs = []
    for ask in (False, True):
        s = Scheduler(doc["profile"])
        s.load_cluster(dict(doc, queue=[]))
        for pod in doc["queue"]:
            q, r = s.cycle(pod, commit=True)
            if ask:
                a = s.ranked_nodes(q, 64)
                assert s.ranked_nodes(q, 64) == a
                assert s.ranked_nodes(q, 5) == a[:5]
                assert (a[0] if a else None) == ((r.selected, r.total) if r.status == 0 else None), (q, a[:1], r)
        runs.append((s.results(), s.node_requested()))
    assert runs[0] == runs[1]
