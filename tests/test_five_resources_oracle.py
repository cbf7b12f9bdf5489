"""The five-resource family (ksg.edge.gen_fit5) on the CPU: the conditions that
keep tests/test_five_resources_gpu.py from being vacuous, each for each Fit
strategy, from the document and the oracle's annotations alone.  With a fifth
resource column the engine scores NodeResourcesFit / BalancedAllocation on the
node columns on every path (a node row holds four)."""
import functools
import json

import pytest

from _oracle import Oracle
from ksg import edge
from test_magnitude_oracle import quantity

P = "kube-scheduler-simulator.sigs.k8s.io/"
FIT, BA = "NodeResourcesFit", "NodeResourcesBalancedAllocation"
SCALARS = (edge.GPU, edge.FPGA)


@functools.lru_cache(maxsize=None)
def scheduled(strategy):
    """(doc, [(selected, feasible, status)], [annotations]) of the whole queue."""
    doc = edge.gen_fit5(strategy)
    o = Oracle(doc)
    o.schedule(record=3)
    return doc, [o.result(q) for q in range(o.n_queue)], [o.annotations(q) for q in range(o.n_queue)]


def requests(pod, res):
    cs = pod["spec"]["containers"] + pod["spec"].get("initContainers", [])
    return sum(quantity(c.get("resources", {}).get("requests", {}).get(res, 0)) for c in cs)


@pytest.mark.parametrize("strategy", edge.FIVE_STRATEGIES)
def test_shape(strategy):
    doc, res, _ = scheduled(strategy)
    assert len(doc["nodes"]) == 70 and len(doc["queue"]) == 12 and len(res) == 12
    names = {k for n in doc["nodes"] for k in n["status"]["allocatable"]} - {"pods"}
    assert names == {"cpu", "memory", edge.EPH, edge.GPU, edge.FPGA}  # five resource columns
    assert sum(1 for s, f, st in res if st == 0 and f >= 2) >= 8, res


@pytest.mark.parametrize("strategy", edge.FIVE_STRATEGIES)
def test_both_skips_and_distinct_scores_are_met(strategy):
    doc, _res, ann = scheduled(strategy)
    alloc = {n["metadata"]["name"]: n["status"]["allocatable"] for n in doc["nodes"]}
    pc = doc["profile"]["pluginConfig"]
    scored_res = {FIT: [r["name"] for r in pc[FIT]["scoringStrategy"]["resources"]],
                  BA: [r["name"] for r in pc[BA]["resources"]]}
    assert all(set(SCALARS) <= set(v) for v in scored_res.values())
    no_scalar = fit_distinct = ba_distinct = 0
    zero_alloc = {FIT: 0, BA: 0}
    for q, pod in enumerate(doc["queue"]):
        rows = json.loads(ann[q].get(P + "score-result", "{}"))
        neither = all(requests(pod, s) == 0 for s in SCALARS)
        no_scalar += neither and len(rows) > 0  # the pod_req == 0 skip, on a pod that is scored
        for node in rows:  # the a == 0 skip, per plugin: a scored node without a resource the scorer reaches
            for plugin, names in scored_res.items():
                for r in names:
                    reached = r not in SCALARS or requests(pod, r) > 0
                    zero_alloc[plugin] += reached and quantity(alloc[node].get(r, 0), r == "cpu") == 0
        fit_distinct += len({int(v[FIT]) for v in rows.values()}) >= 2
        ba_distinct += len({int(v[BA]) for v in rows.values()}) >= 2
    assert no_scalar >= 1 and zero_alloc[BA] >= 1, (no_scalar, zero_alloc)
    # A scored node passed the Fit filter, so it has every scalar the pod requests, and every
    # node has cpu and memory: the skip can only be reached through ephemeral-storage, which
    # RequestedToCapacityRatio's resources leave out here (as ksg.edge's fit_rtc does).
    assert (zero_alloc[FIT] >= 1) == (strategy != "rtc"), zero_alloc
    assert fit_distinct >= 1 and ba_distinct >= 1, (fit_distinct, ba_distinct)
