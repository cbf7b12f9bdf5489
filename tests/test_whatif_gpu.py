"""GPU parity of what-if steps (BASELINE.json cfg5: a step of pods scored against
one frozen snapshot, placements bound between steps) against the oracle's
ksg_oracle_whatif, single context and node-sharded (host exchange over gloo).
Profiles with PodTopologySpread / InterPodAffinity (cfg4) score every pod of a
step on frozen domain tables and bind the step in queue order."""
import json
import os
import socket
import sys

import pytest
import torch.multiprocessing as mp

from _oracle import Oracle
from ksg import Scheduler, generator as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 96


def _oracle_steps(doc, steps, record=0, keep=0):
    o = Oracle(doc)
    for _ in range(steps):
        o.whatif(STEP, record=record)
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("c,sizes", [(5, dict(n_nodes=1500, n_pods=3 * STEP)), (2, dict(n_nodes=800, n_pods=2 * STEP)),
                                     (4, dict(n_nodes=600, n_existing=2400, n_pods=3 * STEP, n_zones=6)),
                                     (1, dict(n_nodes=100, n_pods=2 * STEP))],
                         ids=["cfg5", "cfg2", "cfg4-pts-ipa", "cfg1-default-profile"])
def test_whatif_steps_match_oracle(c, sizes):
    doc = g.generate(c, **sizes)
    steps = len(doc["queue"]) // STEP
    o = _oracle_steps(doc, steps, record=3)
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(STEP, 6)  # sampled parity subset: per-pair outputs / annotations of 6 pods of step 2
    for k in range(steps):
        s.whatif(k * STEP, STEP)
    res = s.results()
    bad = [(q, (r.selected, r.feasible, r.status), o.result(q)) for q, r in enumerate(res)
           if (r.selected, r.feasible, r.status) != o.result(q)]
    assert not bad, bad[:5]
    for q in range(STEP, STEP + 6):
        a, b = s.annotations(q), o.annotations(q)
        for k in b:
            assert a.get(k) == b[k], (q, k)
    # bound placements: every scheduled pod's requests landed on its node
    _, pc = s.node_requested()
    assert sum(pc) == len(doc["pods"]) + sum(1 for r in res if r.status == 0)


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    p = sk.getsockname()[1]
    sk.close()
    return p


def _sharded_worker(rank, world, port, doc_json, out):
    sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ksg import Scheduler as S
    doc = json.loads(doc_json)
    s = S(doc["profile"], device=0, shard_rank=rank, shard_count=world)
    s.set_exchange_host(world)
    s.load_cluster(doc)
    for k in range(len(doc["queue"]) // STEP):
        s.whatif(k * STEP, STEP)
    out[rank] = [(r.selected, r.feasible, r.status) for r in s.results()]
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("c", [5, 4], ids=["cfg5", "cfg4-pts-ipa"])
def test_sharded_whatif_matches_oracle(world, c):
    doc = (g.generate(5, n_nodes=1200, n_pods=2 * STEP) if c == 5 else
           g.generate(4, n_nodes=300, n_existing=1200, n_pods=2 * STEP, n_zones=4))
    o = _oracle_steps(doc, 2)
    want = [o.result(q) for q in range(o.n_queue)]
    port = _free_port()
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_sharded_worker, args=(world, port, json.dumps(doc), out), nprocs=world, join=True)
        for r in range(world):
            assert out[r] == want, f"rank {r} differs"


@pytest.mark.gpu
def test_folded_partials_match_oracle(monkeypatch):
    """Large clusters fold the table chain's per-block partials once (k_fold) instead of
    in every block of k_final, and run the register-capped kernel twins; both forced
    here on a small cfg4 cluster, queue and what-if."""
    monkeypatch.setenv("KSG_FOLD_BLOCKS", "0")
    monkeypatch.setenv("KSG_OCC_BLOCKS", "0")
    doc = g.generate(4, n_nodes=700, n_existing=2500, n_pods=2 * STEP, n_zones=6)
    o = Oracle(doc)
    o.schedule(record=3)
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(0, 8)
    s.schedule()
    for q, r in enumerate(s.results()):
        assert (r.selected, r.feasible, r.status) == o.result(q), q
    for q in range(8):
        assert s.annotations(q) == o.annotations(q), q
    w = _oracle_steps(doc, 2)
    t = Scheduler(doc["profile"])
    t.load_cluster(doc)
    for k in range(2):
        t.whatif(k * STEP, STEP)
    assert [(r.selected, r.feasible, r.status) for r in t.results()] == [w.result(q) for q in range(w.n_queue)]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"KSG_WHATIF_REC_MB": "0"}, {"KSG_WHATIF_REC_MB": "1"}, {"KSG_WHATIF_WIDE": "1"},
                                 {}],
                         ids=["recompute", "chunked-records", "8-byte-records", "classes"])
def test_whatif_pass_records(monkeypatch, env):
    """The cfg5 profile's steps normally take the class path (no per-pair
    memory); with it off (KSG_WHATIF_CLASSES=0) pass 2 reads pass 1's 4-byte
    per-pair records — forced here to recompute every pair, to split the step
    into record chunks (1 MiB: 64 + 32 pods at 1,500 nodes) and to the 8-byte
    layout — single context and 2-rank sharded."""
    if env:
        monkeypatch.setenv("KSG_WHATIF_CLASSES", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    doc = g.generate(5, n_nodes=1500, n_pods=2 * STEP)
    o = _oracle_steps(doc, 2)
    want = [o.result(q) for q in range(o.n_queue)]
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    for k in range(2):
        s.whatif(k * STEP, STEP)
    assert [(r.selected, r.feasible, r.status) for r in s.results()] == want
    assert s.whatif_class_chunks() == (0 if env else 2)
    port = _free_port()
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_sharded_worker, args=(2, port, json.dumps(doc), out), nprocs=2, join=True)
        for r in range(2):
            assert out[r] == want, f"rank {r} differs"


@pytest.mark.gpu
def test_whatif_class_path_edge_selectors():
    """The class path's decoded pods (k_wc_decode: one flat requirement list per
    pod, failed-term masks in pass 1) on the NodeAffinity edge family: matchFields
    In / NotIn (PreFilterResult bitmaps and name requirements), field-only and
    empty terms, DoesNotExist / NotIn, Gt / Lt on non-numeric values, tolerations
    of every form, plus keys and values no node has and an empty nodeSelectorTerms
    list."""
    from ksg import edge
    doc = edge.generate_edge("na", n_pods=2 * STEP - 4)
    for p in doc["queue"]:  # (ephemeral-storage requests keep a step off the class path)
        for c in p["spec"]["containers"]:
            c.get("resources", {}).get("requests", {}).pop(edge.EPH, None)
    extra = [
        {"nodeSelector": {"no-such-key": "x"}},
        {"affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
            {"matchExpressions": [{"key": "no-such-key", "operator": "DoesNotExist"},
                                  {"key": "disk", "operator": "NotIn", "values": ["no-such-value"]}]}]}}}},
        {"affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": []}}}},
        {"affinity": {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 7, "preference": {"matchExpressions": [{"key": "no-such-key", "operator": "NotIn",
                                                               "values": ["a"]}]}},
            {"weight": 5, "preference": {"matchExpressions": [{"key": "no-such-key", "operator": "Exists"}]}},
            {"weight": 3, "preference": {}}]}}},
    ]
    for i, spec in enumerate(extra):
        doc["queue"].append(g.pod_obj(f"pod-extra-{i}", [g.req(200, 256 * 1024 * 1024)], **spec))
    o = _oracle_steps(doc, 2)
    want = [o.result(q) for q in range(o.n_queue)]
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    for k in range(2):
        s.whatif(k * STEP, STEP)
    got = [(r.selected, r.feasible, r.status) for r in s.results()]
    bad = [(q, got[q], want[q]) for q in range(len(want)) if got[q] != want[q]]
    assert not bad, bad[:5]
    assert s.whatif_class_chunks() == 2


@pytest.mark.gpu
def test_whatif_class_path_weight_bound():
    """The class key holds the weighted Fit + BalancedAllocation sum in 24 bits:
    with 100 x the profile's weights just below 2^24 a step runs the class path and
    equals the oracle's (framework.go RunScorePlugins: score x weight)."""
    doc = g.generate(5, n_nodes=1200, n_pods=2 * STEP)
    for k in ("weights", "storeWeights"):
        doc["profile"][k]["NodeResourcesFit"] = 100000
        doc["profile"][k]["NodeResourcesBalancedAllocation"] = 67000
    o = _oracle_steps(doc, 2)
    want = [o.result(q) for q in range(o.n_queue)]
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    for k in range(2):
        s.whatif(k * STEP, STEP)
    got = [(r.selected, r.feasible, r.status) for r in s.results()]
    bad = [(q, got[q], want[q]) for q in range(len(want)) if got[q] != want[q]]
    assert not bad, bad[:5]
    assert s.whatif_class_chunks() > 0
