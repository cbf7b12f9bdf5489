"""The five-resource family (ksg.edge.gen_fit5: LeastAllocated, MostAllocated and
RequestedToCapacityRatio over five resource columns, 70 nodes: two waves, the
last one partial) against the oracle on every pod's result and annotations.  A
node row holds four resources, so with a fifth column every path scores
NodeResourcesFit / BalancedAllocation on the node columns: the queue path, the
per-pod chain and the what-if step.  tests/test_five_resources_oracle.py holds
the conditions that keep the family from being vacuous."""
import pytest

from _oracle import Oracle
from ksg import Scheduler, edge
from test_five_resources_oracle import scheduled
from test_magnitude_gpu import assert_all


@pytest.mark.gpu
@pytest.mark.parametrize("per_pod", [False, True], ids=["queue", "per-pod"])
@pytest.mark.parametrize("strategy", edge.FIVE_STRATEGIES)
def test_queue_paths_match_oracle_on_every_pod(strategy, per_pod):
    doc, want, ann = scheduled(strategy)
    s = Scheduler(doc["profile"])
    s.set_path(per_pod)
    s.load_cluster(doc)
    s.keep_outputs(0, s.queue_len)
    s.schedule()
    assert_all(s, want, ann, (strategy, per_pod))


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", edge.FIVE_STRATEGIES)
def test_whatif_step_matches_oracle_on_every_pod(strategy):
    doc = edge.gen_fit5(strategy)
    o = Oracle(doc)
    o.whatif(len(doc["queue"]), record=3)
    want = [o.result(q) for q in range(o.n_queue)]
    ann = [o.annotations(q) for q in range(o.n_queue)]
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    s.keep_outputs(0, s.queue_len)
    s.whatif(0, s.queue_len)
    assert_all(s, want, ann, (strategy, "whatif"))
