"""The snapshot queries on one context, interleaved (csrc/snapshot_query.hip): headroom, the
eviction fit, the drain and scale-up simulations, the diagnosis and the ranked candidates share one
pinned block and one host gate, and the first four the device buffers of their launch inputs
(sq_in) and answers (sq_out), while their own tests run each on a context of its own.

The sequence makes the pinned block and either device buffer grow, be used below capacity and grow
again (small, large, small, large; the sizes stand beside the steps), and crosses one tile boundary
on each axis: 1,025 nodes (kSqTile = 1024), 33 queue pods and 33 bound pods (kSqPods = 32).  The
scale-up of all 33 pods follows the plan of one node's drain, so its open bytes, which lie behind
its inputs and are never uploaded, land on a freshly grown sq_in.  Every answer is compared with
the same call made as the first query of a fresh context of the same cluster, whose answers the
features' own tests check against their references.
"""
import copy

import pytest

from ksg import Scheduler, generator as g

pytestmark = pytest.mark.gpu

TILE, POD_TILE = 1024, 32


def tile_doc():
    """The tile-edge family of test_headroom_gpu / test_bound_fit_gpu (cfg3-shaped: inside the closed
    form): 33 bound pods placed as test_bound_fit_model.tile_doc places them, 33 queue pods."""
    n_nodes, n = TILE + 1, POD_TILE + 1
    doc = g.generate(3, n_nodes=n_nodes, n_pods=2 * n, seed=4321 + n_nodes)
    want = [0, n_nodes - 1, TILE, n_nodes // 2]
    pods = []
    for j in range(n):
        p = copy.deepcopy(doc["queue"][j])
        p["spec"]["nodeName"] = doc["nodes"][want[j] if j < len(want) else (j * 37) % n_nodes]["metadata"]["name"]
        pods.append(p)
    return {"profile": doc["profile"], "nodes": doc["nodes"], "pods": pods, "queue": doc["queue"][n:]}


def load(doc, kept=None):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    if kept is not None:  # a kept cycle of one pod
        s.keep_outputs(kept, 1)
        s.schedule(kept, 1)
    return s


def test_interleaved_calls_equal_a_fresh_context():
    doc = tile_doc()
    q = b = POD_TILE  # the one pod of the second pod tile, on either axis
    s = load(doc)
    assert (s.n_nodes, s.queue_len, s.bound_count) == (TILE + 1, POD_TILE + 1, POD_TILE + 1)
    every = list(range(POD_TILE + 1))
    steps = [                                                # bytes of   sq_in             sq_out
        lambda x: x.headroom(0, 1),                          #            -                 64
        lambda x: x.drain_plan(0),                           # (1 pod)    28: first use     8
        lambda x: x.scale_up(every, [0, TILE], 16),          #            288 + 66: grows   64
        lambda x: x.bound_fit_nodes(b),                      #            12                4,100: grows
        lambda x: x.headroom(0, POD_TILE + 1),               #            -                 2,112
        lambda x: x.drain(0, TILE + 1),                      #            16,796: grows     32,800: grows
        lambda x: x.scale_up_plan(every, TILE, 16),          #            216 + 33          132
        lambda x: x.node_evictability(),                     #            396               16,928
        lambda x: x.bound_fit(0, POD_TILE + 1),              #            396               528
        lambda x: x.headroom_nodes(q),                       #            -                 4,100
    ]
    for i, call in enumerate(steps):
        want = call(load(doc))
        got = call(s)
        assert len(want) > 0 and got == want, i
    s.keep_outputs(q, 1)
    s.schedule(q, 1)
    kept = [lambda x: x.fit_error(q), lambda x: x.ranked_nodes(q, 64), lambda x: x.filter_histogram(q)]
    answers = []
    for i, call in enumerate(kept):
        want = call(load(doc, kept=q))
        answers.append(want)
        assert call(s) == want, i
    assert answers[0] or answers[1]  # unschedulable: the sentence; scheduled: its candidates
    assert sum(count for *_, count in answers[2]) == TILE + 1
    # and back: the block is used below its capacity again, after the placement
    assert s.headroom(0, 1) == load(doc, kept=q).headroom(0, 1)
