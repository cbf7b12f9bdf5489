"""Unschedulable diagnosis (ksg_filter_histogram / ksg_fit_error;
Scheduler.filter_histogram / fit_error): the per-reason node counts of a kept
pod's cycle, counted on the device, and upstream's FitError sentence from them.

No expected value comes from the calls under test.  The expected histogram is a
Counter over the pod's filter codes (ksg_filter_codes) zipped with the cycle
view's fail_pos / fail_code (a not-evaluated node, fail_pos -1, has status -1:
what ksg_filter_status answers there).  The expected sentence is built by
test_diagnosis_model.fit_error from the ORACLE's annotations (filter-result,
prefilter-result-status, prefilter-result) under the rules restated in that
module, which pins its builder by hand-written literals.

Tile constant: the counting kernel gives one block 512 nodes (kDiagTile,
csrc/diagnosis.hip), two per thread; a block's LDS table holds 64 keys
(kDiagLds) and the device table KSG_DIAG_MAX = 1024 (KSG_DIAG_SLOTS shrinks it).
"""
import copy
import ctypes
import functools
from collections import Counter

import pytest

from _oracle import Oracle
from ksg import Scheduler, edge, generator as g
from ksg.engine import DIAG_MAX, FILTER_NOT_EVALUATED, FILTER_PASSED, KsgError, _FilterBucket
from test_diagnosis_model import fit_error
from test_plugin_api_gpu import CASES

E_INVALID, E_STATE, E_RANGE, E_NOBUF = -1, -3, -4, -5
EDGE = ("na", "pts", "ipa", "preempt", "volumes")
TILE = 512


def want_histogram(s, q):
    """[(code, pos, status, count)] ascending, from ksg_filter_codes and the cycle view."""
    v = s.cycle_view(q)
    try:
        codes = s.filter_codes(q)
        assert len(codes) == v.N
        c = Counter()
        for i, code in enumerate(codes):
            fp = v._v.fail_pos[i]
            c[(code, fp, v._v.fail_code[i] if fp >= 0 else -1)] += 1
        return [k + (n,) for k, n in sorted(c.items(), key=lambda kv: (kv[0][0], kv[0][2]))]
    finally:
        v.release()


def check(s, q, sentence):
    """Both calls on kept pod q; returns (histogram, sentence)."""
    want = want_histogram(s, q)
    got = s.filter_histogram(q)
    assert got == want, (q, got, want)
    assert sum(b[3] for b in got) == s.n_nodes
    for code, pos, status, _ in got:  # the bucket's own fields agree
        if code == FILTER_PASSED:
            assert status == 0
        elif code == FILTER_NOT_EVALUATED:
            assert (pos, status) == (-1, -1)
        else:
            assert status in (2, 3) and pos >= 0
    text = s.fit_error(q)
    assert text == sentence, (q, text, sentence)
    return got, text


def oracle_sentences(doc):
    """(result, sentence) of every queue pod, from the oracle alone."""
    o = Oracle(doc)
    o.schedule(record=3)
    n, plugins = len(doc["nodes"]), doc["profile"]["plugins"]
    return [(o.result(q), fit_error(o.annotations(q), o.result(q)[2], n, plugins)) for q in range(o.n_queue)]


def queue_run(doc, keep=None):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(0, s.queue_len if keep is None else keep)
    s.schedule()
    return s


def oversized(name="pod-oversized"):
    return g.pod_obj(name, [g.req(10_000_000, g.Mi)])


# ------------------------------------------------------------------ 1: the hand-built cluster
GPU_TAINT = {"key": "dedicated", "value": "gpu", "effect": "NoSchedule"}
FLAKY_TAINT = {"key": "flaky", "value": "yes", "effect": "NoSchedule"}
HAND_SENTENCE = ("0/40 nodes are available: 12 node(s) had untolerated taint {dedicated: gpu}, 15 Insufficient cpu, "
                 "3 node(s) had untolerated taint {flaky: yes}, 4 Too many pods, "
                 "5 node(s) didn't match Pod's node affinity/selector, 6 Insufficient memory.")
# (profile position, Fit detail bits or None, framework code, nodes): pod-a's buckets in
# (code, status) order.  Fit's detail: bit 0 too many pods, bit 1 cpu, bit 2 memory; its code is
# Unschedulable (2), or UnschedulableAndUnresolvable (3) where a short request exceeds allocatable
HAND_BUCKETS = [(0, None, 3, 12), (0, None, 3, 3), (1, None, 3, 5),
                (2, 1, 2, 3), (2, 2, 2, 4), (2, 2, 3, 6), (2, 3, 3, 1), (2, 4, 3, 2), (2, 6, 3, 4)]


@functools.lru_cache(maxsize=None)
def hand_doc():
    """40 nodes under TaintToleration, NodeAffinity, Fit, BalancedAllocation.  pod-a (8 cpu,
    16Gi, selector disk=ssd, no toleration) fits nowhere:
      0-11  taint dedicated=gpu                     12-14  taint flaky=yes
      15-19 no disk label                           20-25  4 cpu allocatable (cpu short, unresolvable)
      26-29 16 cpu, 12 in use (cpu short)           30-31  8Gi (memory short)
      32-35 4 cpu and 8Gi (both: two reasons)       36-38  pod limit 1, in use
      39    pod limit 1 in use and 4 cpu (two reasons)
    pod-b (selector only=b) fits node 26 alone; pod-c (no selector) fits the 21 untainted nodes
    with pod room, 15-35."""
    big, ssd = 64 * g.Gi, {"disk": "ssd"}
    nodes, pods = [], []

    def add(cpu, mem, labels=None, taints=None, limit=110, used=None):
        name = f"node-{len(nodes):07d}"
        nodes.append(g.node_obj(name, cpu, mem, pods=limit, labels=labels, taints=taints))
        if used:
            pods.append(g.filler_pod(f"fill-{len(nodes) - 1:07d}", name, *used))

    for _ in range(12):
        add(16000, big, ssd, [GPU_TAINT])
    for _ in range(3):
        add(16000, big, ssd, [FLAKY_TAINT])
    for _ in range(5):
        add(16000, big)
    for _ in range(6):
        add(4000, big, ssd)
    for i in range(4):
        add(16000, big, dict(ssd, only="b") if i == 0 else ssd, used=(12000, g.Gi))
    for _ in range(2):
        add(16000, 8 * g.Gi, ssd)
    for _ in range(4):
        add(4000, 8 * g.Gi, ssd)
    for _ in range(3):
        add(16000, big, ssd, limit=1, used=(100, 64 * g.Mi))
    add(4000, big, ssd, limit=1, used=(100, 64 * g.Mi))
    assert len(nodes) == 40
    queue = [g.pod_obj("pod-a", [g.req(8000, 16 * g.Gi)], nodeSelector=ssd),
             g.pod_obj("pod-b", [g.req(1000, g.Gi)], nodeSelector={"only": "b"}),
             g.pod_obj("pod-c", [g.req(1000, g.Gi)])]
    prof = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                           ("NodeResourcesBalancedAllocation", 1)], 7)
    return {"profile": prof, "nodes": nodes, "pods": pods, "queue": queue}


def hand_answers(s):
    return [(s.filter_histogram(q), s.fit_error(q)) for q in range(3)]


@pytest.mark.gpu
def test_hand_built_cluster_literals():
    doc = hand_doc()
    ora = oracle_sentences(doc)  # the literal pins the test's own builder as well as the engine
    assert [r[1:] for r, _ in ora] == [(0, 1), (1, 0), (21, 0)]
    assert [t for _, t in ora] == [HAND_SENTENCE, "", ""]
    s = queue_run(doc)
    res = s.results()
    assert [(r.feasible, r.status) for r in res] == [(0, 1), (1, 0), (21, 0)] and res[1].selected == 26
    hist, _ = check(s, 0, HAND_SENTENCE)
    assert [(pos, status, n) for _, pos, status, n in hist] == [(p, st, n) for p, _, st, n in HAND_BUCKETS]
    for (code, pos, _, _), (_, detail, _, _) in zip(hist, HAND_BUCKETS):
        if detail is not None:
            assert code & 0xFFFFFF == detail and code >> 24 == pos
    hist_b, _ = check(s, 1, "")  # one feasible node: no sentence, the histogram still exact
    assert [(c, n) for c, _, _, n in hist_b if c == FILTER_PASSED] == [(FILTER_PASSED, 1)]
    assert sorted(n for c, _, _, n in hist_b if c != FILTER_PASSED) == [3, 12, 24]
    hist_c, _ = check(s, 2, "")
    assert [(c, n) for c, _, _, n in hist_c if c == FILTER_PASSED] == [(FILTER_PASSED, 21)]
    assert s.diag_routes() == (6, 0)


# ------------------------------------------------------------------ 2: families
@functools.lru_cache(maxsize=None)
def family(name):
    if name in EDGE:
        return edge.generate_edge(name)
    _, c, sizes = next(x for x in CASES if x[0] == name)
    return g.generate(c, **sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES] + list(EDGE))
def test_families_queue_mode(name):
    """cfg1..cfg4 at the plugin-API sizes and the edge variants at their default sizes, queue
    mode, every pod kept: histogram and sentence of every pod.  The edge variants must keep
    yielding unschedulable pods (checked with the oracle on the CPU when the sizes were fixed:
    na 100 pods, up to 6 reasons; pts 5; ipa 9; preempt 73, up to 5; volumes 52, up to 3, 19 of
    them rejected by a PreFilter, 2 by an empty PreFilterResult intersection)."""
    doc = family(name)
    ora = oracle_sentences(doc)
    s = queue_run(doc)
    res = s.results()
    assert len(res) == len(ora)
    unsched = prefilter = merge = 0
    for q, (r, (want_r, text)) in enumerate(zip(res, ora)):
        assert (r.selected, r.feasible, r.status) == want_r, (name, q)
        check(s, q, text)
        if r.status == 1:
            unsched += 1
            assert text.startswith(f"0/{len(doc['nodes'])} nodes are available:")
            body = text.split(": ", 1)[1] if ": " in text else ""
            if body and not body[0].isdigit():
                prefilter += 1
                merge += "didn't satisfy plugin" in body
    if name in EDGE:
        assert unsched >= 1, name
    if name == "volumes":
        assert prefilter >= 1 and merge >= 1, (prefilter, merge)


def test_edge_variants_keep_their_unschedulable_pods():
    """The condition behind the family sizes, on the CPU: every listed edge variant yields an
    unschedulable pod, and at least three yield one with three or more distinct reasons."""
    rich = 0
    for name in EDGE:
        texts = [t for (_, _, st), t in oracle_sentences(family(name)) if st == 1]
        assert texts, name
        rich += any(t.count(", ") >= 2 and t.split(": ", 1)[1][0].isdigit() for t in texts if ": " in t)
    assert rich >= 3


# ------------------------------------------------------------------ 3: tile and table edges
@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [TILE - 1, TILE, TILE + 1, 2 * TILE + 276])
def test_tile_edges(n_nodes):
    """cfg2-shaped clusters with an oversized pod appended: one node short of a block's tile
    of 512, exactly one tile, one node past it, and 1,300 nodes: three blocks, the last ragged."""
    base = g.generate(2, n_nodes=n_nodes, n_pods=3)
    doc = dict(base, queue=base["queue"] + [oversized()])
    ora = oracle_sentences(doc)
    s = queue_run(doc)
    for q, (r, (want_r, text)) in enumerate(zip(s.results(), ora)):
        assert (r.selected, r.feasible, r.status) == want_r, q
        check(s, q, text)
    assert ora[-1][0][2] == 1 and ora[-1][1] == f"0/{n_nodes} nodes are available: {n_nodes} Insufficient cpu."
    assert s.diag_routes()[1] == 0


# ------------------------------------------------------------------ 4: many distinct reasons
def own_taint_doc(n_nodes):
    nodes = [g.node_obj(f"node-{i:07d}", 16000, 64 * g.Gi,
                        taints=[{"key": "own", "value": f"v{i}", "effect": "NoSchedule"}]) for i in range(n_nodes)]
    prof = g.make_profile([("TaintToleration", 3), ("NodeResourcesFit", 1), ("NodeResourcesBalancedAllocation", 1)], 11)
    return {"profile": prof, "nodes": nodes, "pods": [], "queue": [g.pod_obj("pod-a", [g.req(1000, g.Gi)])]}


def _raw_hist(s, q, cap, out=True, n_out=True):
    arr = (_FilterBucket * max(cap, 1))()
    n = ctypes.c_uint32(99)
    rc = s.L.ksg_filter_histogram(s.h, ctypes.c_uint32(q), arr if out else None, ctypes.c_uint32(cap),
                                  ctypes.byref(n) if n_out else None)
    return rc, n.value


@pytest.mark.gpu
def test_more_reasons_than_a_block_table():
    """300 nodes, each with its own taint value: 300 keys in one block, more than its 64 LDS
    slots, fewer than KSG_DIAG_MAX: the device table answers."""
    doc = own_taint_doc(300)
    (_, text), = oracle_sentences(doc)
    assert text.count(", ") == 299
    s = queue_run(doc)
    hist, _ = check(s, 0, text)
    assert len(hist) == 300 and all(b[3] == 1 for b in hist)
    dev, host = s.diag_routes()  # (the binding calls again with a larger buffer after KSG_E_NOBUF)
    assert dev >= 2 and host == 0


@pytest.mark.gpu
def test_more_reasons_than_the_device_table():
    """1,100 nodes: more keys than KSG_DIAG_MAX.  Both calls still succeed, by the host count."""
    doc = own_taint_doc(1100)
    (_, text), = oracle_sentences(doc)
    assert text.count(", ") == 1099
    s = queue_run(doc)
    hist, _ = check(s, 0, text)
    assert len(hist) == 1100
    dev, host = s.diag_routes()
    assert dev == 0 and host >= 2
    assert _raw_hist(s, 0, DIAG_MAX) == (E_NOBUF, 1100)
    assert _raw_hist(s, 0, 1100) == (0, 1100)
    assert _raw_hist(s, 0, 2048) == (0, 1100)


# ------------------------------------------------------------------ 5: forced overflow
@pytest.mark.gpu
def test_forced_overflow_same_bytes(monkeypatch):
    """KSG_DIAG_SLOTS=4 on the hand-built cluster: pod-a's nine keys overflow four slots; the
    host count returns the bytes the device table returns at the default size."""
    doc = hand_doc()
    monkeypatch.delenv("KSG_DIAG_SLOTS", raising=False)
    s = queue_run(doc)
    default = hand_answers(s)
    assert s.diag_routes() == (6, 0)
    monkeypatch.setenv("KSG_DIAG_SLOTS", "4")
    t = queue_run(doc)
    assert hand_answers(t) == default
    assert default[0][1] == HAND_SENTENCE
    dev, host = t.diag_routes()
    assert host >= 2 and dev + host == 6  # (both calls on pod-a at the least)
    check(t, 0, HAND_SENTENCE)


# ------------------------------------------------------------------ 6: cycle mode
@pytest.mark.gpu
@pytest.mark.parametrize("commit", [False, True], ids=["plugin", "harness"])
@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_cycle_mode(name, commit):
    """ksg_cycle with either commit value, an oversized pod after the family's first 20: the
    answers against the oracle's, unchanged by the Reserve that follows a commit = 0 cycle."""
    base = family(name)
    doc = dict(base, queue=base["queue"][:20] + [oversized()])
    ora = oracle_sentences(doc)
    s = Scheduler(doc["profile"])
    s.load_cluster(dict(doc, queue=[]))
    for i, pod in enumerate(doc["queue"]):
        q, r = s.cycle(pod, commit=commit)
        assert (r.selected, r.feasible, r.status) == ora[i][0], (name, i)
        got = check(s, q, ora[i][1])
        if not commit and r.selected >= 0:
            s.reserve(q, r.selected)
            assert (s.filter_histogram(q), s.fit_error(q)) == got, (name, i)
    assert r.status == 1 and ora[-1][1].startswith(f"0/{len(doc['nodes'])} nodes are available: ")


# ------------------------------------------------------------------ 7: side effects, errors
@pytest.mark.gpu
def test_no_side_effects():
    """cfg4 cycle by cycle, with and without the two calls after every cycle: the same results
    and node rows; two calls on one pod, the same bytes."""
    base = family("cfg4")
    doc = dict(base, queue=base["queue"] + [oversized()])
    runs = []
    for ask in (False, True):
        s = Scheduler(doc["profile"])
        s.load_cluster(dict(doc, queue=[]))
        for pod in doc["queue"]:
            q, _ = s.cycle(pod, commit=True)
            if ask:
                a = (s.filter_histogram(q), s.fit_error(q))
                assert (s.filter_histogram(q), s.fit_error(q)) == a
        runs.append((s.results(), s.node_requested()))
    assert runs[0] == runs[1]
    assert a[1].startswith("0/120 nodes are available: ")


def _raw_text(s, q, cap, length=True):
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_size_t(99)
    rc = s.L.ksg_fit_error(s.h, ctypes.c_uint32(q), buf if cap else None, ctypes.c_size_t(cap),
                           ctypes.byref(n) if length else None)
    return rc, n.value, buf.raw[:n.value] if rc == 0 else b""


@pytest.mark.gpu
def test_errors_leave_the_context_usable():
    doc = hand_doc()
    s = queue_run(doc, keep=2)
    good = [(s.filter_histogram(q), s.fit_error(q)) for q in range(2)]
    assert good[0][1] == HAND_SENTENCE
    n = len(HAND_SENTENCE)
    # buffers: the size query, a short buffer, an exact one
    assert _raw_text(s, 0, 0) == (E_NOBUF, n, b"")
    assert _raw_text(s, 0, n - 1) == (E_NOBUF, n, b"")
    assert _raw_text(s, 0, n) == (0, n, HAND_SENTENCE.encode())
    assert _raw_text(s, 1, 0) == (0, 0, b"")  # a scheduled pod: nothing to write
    assert _raw_hist(s, 0, 8) == (E_NOBUF, 9)
    assert _raw_hist(s, 0, 9) == (0, 9)
    # arguments and range
    assert _raw_hist(s, 0, 16, out=False) == (E_RANGE, 0)
    assert _raw_hist(s, 0, 16, n_out=False)[0] == E_RANGE
    assert _raw_hist(s, s.queue_len, 16) == (E_RANGE, 0)
    assert _raw_text(s, 0, 64, length=False)[0] == E_RANGE
    assert _raw_text(s, s.queue_len, 64)[:2] == (E_RANGE, 0)
    # a pod whose outputs were not kept: what ksg_normalized_scores answers for it
    arr = (ctypes.c_int64 * s.n_nodes)()
    norm_rc = s.L.ksg_normalized_scores(s.h, 2, 0, arr, s.n_nodes)
    assert norm_rc == E_STATE
    assert _raw_hist(s, 2, 16) == (norm_rc, 0)
    assert b"not kept" in s.L.ksg_last_error(s.h)
    assert _raw_text(s, 2, 64)[:2] == (norm_rc, 0)
    assert b"not kept" in s.L.ksg_last_error(s.h)
    with pytest.raises(KsgError):
        s.fit_error(2)
    # the context is still usable, and the answers are the same
    assert [(s.filter_histogram(q), s.fit_error(q)) for q in range(2)] == good
    check(s, 0, HAND_SENTENCE)


@pytest.mark.gpu
def test_sharded_context_is_refused():
    doc = hand_doc()
    s = Scheduler(doc["profile"], shard_rank=0, shard_count=2)
    s.load_cluster(doc)
    assert _raw_hist(s, 0, 16) == (E_INVALID, 0)
    assert _raw_text(s, 0, 64)[:2] == (E_INVALID, 0)
    assert b"sharded" in s.L.ksg_last_error(s.h)
