"""The magnitude family (ksg.edge.gen_magnitude: clusters sized at the gates of
the engine's arithmetic fast paths) through every path that scores
NodeResourcesFit / BalancedAllocation.  Unlike the sampled checks elsewhere,
every pod's (selected, feasible, status) AND every pod's annotations (the
per-node filter, score and final-score values) must equal the oracle's, so a
score that is one off on a node that does not win still fails.
tests/test_magnitude_oracle.py pins the oracle itself at these sizes;
tests/test_arith_gpu.py tests the primitives on their own."""
import functools

import pytest

from _oracle import Oracle
from ksg import Scheduler, edge
from ksg.engine import FILTER_PASSED
from test_edge_gpu import without_queue
from test_plugin_api_gpu import SCORERS, _ViewCalls, rebuild
from test_ranked_gpu import check as ranked_check
from test_whatif_gpu import STEP, _oracle_steps

PLAIN = ("div32", "div52", "zero_over")
# every kind x profile; norm20 is about the NodeAffinity normaliser and runs under the profile that has it
CASES = [(k, p) for k in PLAIN + ("wc_gate",) for p in edge.MAG_PROFILES] + [("norm20", "static")]
IDS = [f"{k}-{p}" for k, p in CASES]


@functools.lru_cache(maxsize=None)
def queue_reference(kind, profile, n_pods=96):
    doc = edge.gen_magnitude(kind, profile=profile, n_pods=n_pods)
    o = Oracle(doc)
    o.schedule(record=3)
    return doc, [o.result(q) for q in range(o.n_queue)], [o.annotations(q) for q in range(o.n_queue)]


def assert_all(s, want, ann, tag):
    res = s.results()
    bad = [(q, (r.selected, r.feasible, r.status), want[q]) for q, r in enumerate(res)
           if (r.selected, r.feasible, r.status) != want[q]]
    assert not bad and len(res) == len(want), (tag, bad[:5])
    for q in range(len(want)):
        a = s.annotations(q)
        for k, v in ann[q].items():
            assert a.get(k) == v, (tag, q, k)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("per_pod", [False, True], ids=["window", "per-pod"])
@pytest.mark.parametrize("kind,profile", CASES, ids=IDS)
def test_queue_paths_match_oracle_on_every_pod(kind, profile, per_pod):
    """schedule() on the window batch path and on the per-pod chain; then
    ranked_nodes(q, 64) of a sample of pods: in key order, out[0] the result."""
    doc, want, ann = queue_reference(kind, profile)
    s = Scheduler(doc["profile"])
    s.set_path(per_pod)
    s.load_cluster(doc)
    s.keep_outputs(0, s.queue_len)
    s.schedule()
    res = assert_all(s, want, ann, (kind, profile, per_pod))
    if not per_pod:
        for q in range(0, len(res), 8):
            ranked_check(s, q, doc, res[q], (1, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,profile", CASES, ids=IDS)
def test_cycle_and_view_match_oracle_on_every_pod(kind, profile):
    """The drop-in cycle: every pod's result, the annotations rebuilt from the
    cycle view's arrays (statuses, filter results, raw and normalized scores) and
    from the extension-point calls, both against the oracle's, and the view's raw /
    normalized rows on every feasible node against scores() / normalized_scores()."""
    doc, want, ann = queue_reference(kind, profile, 40)
    s = Scheduler(doc["profile"])
    s.load_cluster(without_queue(doc))
    names = [n["metadata"]["name"] for n in doc["nodes"]]
    plugins = doc["profile"]["plugins"]
    for i, pod in enumerate(doc["queue"]):
        q, r = s.cycle(pod, commit=True)
        assert (r.selected, r.feasible, r.status) == want[i], (kind, profile, i)
        v = s.cycle_view(q)
        for src in (_ViewCalls(s, v), s):
            for k, val in rebuild(src, q, doc["profile"], names, r.status).items():
                assert val == ann[i][k], (kind, profile, i, k, type(src).__name__)
        feas = [n for n, c in enumerate(s.filter_codes(q)) if c == FILTER_PASSED]
        assert len(feas) == r.feasible, (kind, profile, i)
        if r.feasible > 1:
            for pos, pl in enumerate(plugins):
                if pl in SCORERS and s.prescore_status(q, pos)[0] == 0:
                    raw, norm, vr, vn = s.scores(q, pos), s.normalized_scores(q, pos), v.scores(pos), v.normalized_scores(pos)
                    for n in feas:
                        assert (vr[n], vn[n]) == (raw[n], norm[n]), (kind, profile, i, pl, n)
        v.release()


WHATIF_DOCS = [(k, None) for k in PLAIN] + [("wc_gate", v) for v in edge.WC_GATE_VIOLATIONS]
ENVS = [{}, {"KSG_WHATIF_CLASSES": "0"}, {"KSG_WHATIF_REC_MB": "0"}]


@functools.lru_cache(maxsize=None)
def whatif_reference(kind, violate):
    doc = edge.gen_magnitude(kind, n_pods=2 * STEP, violate=violate)
    o = _oracle_steps(doc, 2, record=3)
    return doc, [o.result(q) for q in range(o.n_queue)], [o.annotations(q) for q in range(o.n_queue)]


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=["default", "no-classes", "recompute"])
@pytest.mark.parametrize("kind,violate", WHATIF_DOCS, ids=[k if v is None else f"{k}-{v}" for k, v in WHATIF_DOCS])
def test_whatif_steps_match_oracle_on_every_pod(monkeypatch, kind, violate, env):
    """Two what-if steps under the default Fit + BalancedAllocation profile, and the
    path they took.  The class path (k_whatif_cls1/2) holds its columns in doubles:
    run_whatif admits a step only when load_cluster found every cpu / memory column
    of every node inside (-2^45, 2^45) and every pod of THAT step requests cpu /
    memory in [0, 2^44).  So whatif_class_chunks() is the step count (2) on the
    in-gate wc_gate document, 0 when one node's memory or requested memory is 2^45,
    and 1 when one pod requests 2^44 bytes: the gate is per step, the step holding
    that pod (the first: it is queue pod 5) leaves the class path as a whole and the
    second step takes it.  (The path of the other kinds also depends on their
    ephemeral-storage requests and taints, and is not asserted.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    doc, want, ann = whatif_reference(kind, violate)
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(0, s.queue_len)
    for k in range(2):
        s.whatif(k * STEP, STEP)
    assert_all(s, want, ann, (kind, violate, env))
    if kind == "wc_gate":
        chunks = {None: 2, "pod_req": 1}.get(violate, 0) if not env else 0
        assert s.whatif_class_chunks() == chunks, (kind, violate, env)
