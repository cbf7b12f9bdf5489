"""Drain simulation (ksg_drain / ksg_drain_plan, include/ksg.h): the references the
GPU tests use, checked against each other on the CPU.

A node's subjects -- its bound pods in ascending bound index, DaemonSet-owned and
mirror pods left out -- are re-placed one after another: each on the lowest node
other than its own whose verdict is "passed", and counted there (requests and
pod count) before the next is judged.

1. The model (simulate): a few lines over test_bound_fit_model.reference, called
   subject by subject on a copy of usage(doc) that gains each placed pod on its
   destination.
2. Hand-written literals for an 11-node, 20-pod competition cluster (COMP, COMP_PLANS).
3. The ORACLE as an experiment (oracle_plan): the document with the earlier
   subjects re-bound to their destinations and the current one unbound, one oracle
   cycle (oracle_verdicts), the lowest feasible node other than the candidate.

No GPU and no engine call.  The document builders of the GPU tests live here.
"""
import copy
import functools
from collections import Counter, namedtuple

import pytest

from _oracle import Oracle
from ksg import generator as g
from test_headroom_model import pod_requests, quantity
import test_bound_fit_model as bf

Drain = namedtuple("Drain", "pods daemon placed unplaced skipped first_unplaced dest_nodes")
DRAIN_MAX = 512
MIRROR = "kubernetes.io/config.mirror"
EMPTY = Drain(0, 0, 0, 0, 0, -1, 0)


def stays(pod):
    """A drain leaves the pod in place: a DaemonSet controller owns it, or it is a mirror pod."""
    md = pod["metadata"]
    return (any(o.get("controller") and o.get("kind") == "DaemonSet" for o in md.get("ownerReferences", []))
            or MIRROR in md.get("annotations", {}))


def daemon_owned(pod, name="ds"):
    p = copy.deepcopy(pod)
    p["metadata"]["ownerReferences"] = [{"apiVersion": "apps/v1", "kind": "DaemonSet", "name": name, "uid": "u-" + name,
                                         "controller": True}]
    return p


def mirror(pod):
    p = copy.deepcopy(pod)
    p["metadata"].setdefault("annotations", {})[MIRROR] = "0123abcd"
    return p


def on_node(doc, x, n_subjects=None):
    name = doc["nodes"][x]["metadata"]["name"]
    n = len(doc["pods"]) if n_subjects is None else n_subjects
    return [b for b in range(n) if doc["pods"][b]["spec"]["nodeName"] == name]


def simulate(doc, x, cap=DRAIN_MAX, n_subjects=None, state=None):
    """(Drain, plan) of node x.  The first n_subjects of doc["pods"] are the bound pods (the rest is load the
    rows hold); state: usage(doc), shared by a caller's loop and left unchanged."""
    used, cnt = state or bf.usage(doc)
    used, cnt = Counter(used), Counter(cnt)
    here = on_node(doc, x, n_subjects)
    subjects = [b for b in here if not stays(doc["pods"][b])]
    plan = []
    for b in subjects[:cap]:
        verdicts = bf.reference(doc, b, (used, cnt))
        dest = next((n for n, v in enumerate(verdicts) if v == "passed" and n != x), -1)
        plan.append((b, dest))
        if dest >= 0:
            name = doc["nodes"][dest]["metadata"]["name"]
            cnt[name] += 1
            for k, v in pod_requests(doc["pods"][b]).items():
                used[(name, k)] += v
    plan += [(b, -2) for b in subjects[cap:]]
    gone = [d for _, d in plan if d >= 0]
    lost = [b for b, d in plan if d == -1]
    return Drain(len(here), len(here) - len(subjects), len(gone), len(lost), len(subjects[cap:]),
                 lost[0] if lost else -1, len(set(gone))), plan


def simulate_all(doc, cap=DRAIN_MAX, n_subjects=None):
    state = bf.usage(doc)
    return [simulate(doc, x, cap, n_subjects, state) for x in range(len(doc["nodes"]))]


def oracle_plan(doc, x):
    """The same plan from oracle cycles: before subject b the earlier subjects are bound to their
    destinations (an unplaced one stays on x); b, unbound, runs one cycle on the document without it."""
    d = {"profile": doc["profile"], "nodes": doc["nodes"], "pods": copy.deepcopy(doc["pods"]), "queue": doc["queue"]}
    plan = []
    for b in on_node(doc, x):
        if stays(doc["pods"][b]):
            continue
        verdicts = bf.oracle_verdicts(d, b)
        dest = next((n for n, v in enumerate(verdicts) if v == "passed" and n != x), -1)
        plan.append((b, dest))
        if dest >= 0:
            d["pods"][b]["spec"]["nodeName"] = doc["nodes"][dest]["metadata"]["name"]
    return plan


# ------------------------------------------------------------------ the competition cluster
GPU = bf.GPU


@functools.lru_cache(maxsize=None)
def comp_doc():
    """11 nodes, 20 bound pods; the profile of test_bound_fit_model's hand cluster.  What is left on each
    node (cpu milli, gpu, pod room), and who lives there (bound index: name, cpu):
      0  1000 - 1  0: ds0 100 (DaemonSet), 1: a1 3000, 2: mir0 900 (mirror), 3: a2 3000; pod limit 5
      1  8000 - 8  tainted dedicated=gpu, empty: the lowest node with room, skipped
      2  8000 - 8  cordoned, empty: skipped
      3  4000 - 2  4: f3 4000; pod limit 3.  The only node with 3000 left: a1 and a2 each fit alone
      4  2500 - 5  5: b1 2000, 6: b2 2000, 7: b3 1500.  b1 and b2 fill node 3 exactly, b3 goes on to 5
      5  2000 - 7  8: f5 6000
      6  1000 - 4  9..12: z1..z4, no requests: node 0 takes one (its room), node 3 two, node 4 the last
      7  1700 1 5  13..15: g1..g3, 100 and one gpu each; 4 gpus
      8  2000 1 7  16: g8 6000 and one of 2 gpus
      9  2000 1 7  17: f9 6000; 1 gpu
      10 1000 - 6  18: r10 500, one affinity term names nodes 8 and 9 at once: rejected; 19: p10 500"""
    big = 32 * g.Gi
    names = [f"node-{i:07d}" for i in range(11)]
    nodes = [g.node_obj(names[0], 8000, big, pods=5),
             g.node_obj(names[1], 8000, big, pods=8, taints=[dict(bf.GPU_TAINT)]),
             g.node_obj(names[2], 8000, big, pods=8, unschedulable=True),
             g.node_obj(names[3], 8000, big, pods=3),
             g.node_obj(names[4], 8000, big, pods=8),
             g.node_obj(names[5], 8000, big, pods=8),
             g.node_obj(names[6], 1000, big, pods=8),
             g.node_obj(names[7], 2000, big, pods=8, scalars={GPU: 4}),
             g.node_obj(names[8], 8000, big, pods=8, scalars={GPU: 2}),
             g.node_obj(names[9], 8000, big, pods=8, scalars={GPU: 1}),
             g.node_obj(names[10], 2000, big, pods=8)]

    def on(i, name, cpu=None, gpu=None, **kw):
        c = [{}] if cpu is None else [g.req(cpu, g.Gi, {GPU: str(gpu)} if gpu else None)]
        return g.pod_obj(name, c, node=names[i], **kw)

    pods = [daemon_owned(on(0, "ds0", 100)), on(0, "a1", 3000), mirror(on(0, "mir0", 900)), on(0, "a2", 3000),
            on(3, "f3", 4000),
            on(4, "b1", 2000), on(4, "b2", 2000), on(4, "b3", 1500),
            on(5, "f5", 6000),
            on(6, "z1"), on(6, "z2"), on(6, "z3"), on(6, "z4"),
            on(7, "g1", 100, 1), on(7, "g2", 100, 1), on(7, "g3", 100, 1),
            on(8, "g8", 6000, 1),
            on(9, "f9", 6000),
            on(10, "r10", 500, affinity=bf.named_affinity([names[8], names[9]])), on(10, "p10", 500)]
    queue = [g.pod_obj("q-small", [g.req(500, 512 * g.Mi)]), g.pod_obj("q-zero", [{}])]
    return {"profile": g.make_profile(bf.HAND_PLUGINS, 7), "nodes": nodes, "pods": pods, "queue": queue}


# per node: Drain(pods, daemon, placed, unplaced, skipped, first_unplaced, dest_nodes) and the plan
COMP = [
    Drain(4, 2, 1, 1, 0, 3, 1),    # a1 takes node 3's 4000; a2 finds 1000 there and 3000 nowhere
    EMPTY, EMPTY,
    Drain(1, 0, 0, 1, 0, 4, 0),    # f3: no node has 4000 (1 and 2 are closed)
    Drain(3, 0, 3, 0, 0, -1, 2),   # b1, b2 -> 3 (4000 - 2000 - 2000 = 0, 3 of 3 pods), b3 -> 5
    Drain(1, 0, 0, 1, 0, 8, 0),
    Drain(4, 0, 4, 0, 0, -1, 3),   # z1 -> 0 (4 + 1 of 5), z2, z3 -> 3 (1 + 2 of 3), z4 -> 4
    Drain(3, 0, 2, 1, 0, 15, 2),   # g1 -> 8, g2 -> 9: one gpu each; g3: none left
    Drain(1, 0, 0, 1, 0, 16, 0),
    Drain(1, 0, 0, 1, 0, 17, 0),
    Drain(2, 0, 1, 1, 0, 18, 1),   # r10 rejected; the simulation goes on: p10 -> 0
]
COMP_PLANS = [[(1, 3), (3, -1)], [], [], [(4, -1)], [(5, 3), (6, 3), (7, 5)], [(8, -1)],
              [(9, 0), (10, 3), (11, 3), (12, 4)], [(13, 8), (14, 9), (15, -1)], [(16, -1)], [(17, -1)],
              [(18, -1), (19, 0)]]


def drainable(d):
    return d.unplaced == 0 and d.skipped == 0


def test_competition_literals():
    doc = comp_doc()
    assert bf.columns(doc) == ["cpu", "memory", "ephemeral-storage", GPU]
    assert len(doc["nodes"]) == len(COMP) == len(COMP_PLANS) == 11 and len(doc["pods"]) == 20
    got = simulate_all(doc)
    for x, (d, plan) in enumerate(got):
        assert d == COMP[x], (x, d)
        assert plan == COMP_PLANS[x], (x, plan)
    assert [drainable(d) for d in COMP] == [False, True, True, False, True, False, True, False, False, False, False]
    # what justifies the call: judged alone, each of node 0's pods has somewhere to go (stuck == 0) ...
    state = bf.usage(doc)
    fits = [bf.summary(doc, b, bf.reference(doc, b, state)) for b in range(len(doc["pods"]))]
    assert bf.evictability(doc, fits)[0] == (4, 0, 0) and fits[1].first_other == fits[3].first_other == 3
    # ... yet the two compete for node 3's room: the drain leaves one behind
    assert COMP[0].unplaced == 1
    # the gpu is the binding column of node 7's pods, the pod room that of node 6's
    assert fits[13].other_nodes == fits[15].other_nodes == 2 and bf.evictability(doc, fits)[7][1] == 0
    # the first subject's destination is its first_other; who has nowhere to go alone is unplaced
    for x, plan in enumerate(COMP_PLANS):
        if plan:
            assert plan[0][1] == fits[plan[0][0]].first_other
        assert all(d == -1 for b, d in plan if fits[b].other_nodes == 0)


def test_cap_in_the_model():
    doc = comp_doc()
    d, plan = simulate(doc, 6, cap=2)
    assert d == Drain(4, 0, 2, 0, 2, -1, 2) and plan == [(9, 0), (10, 3), (11, -2), (12, -2)] and not drainable(d)


def test_competition_oracle_experiment():
    doc = comp_doc()
    for x in range(len(doc["nodes"])):
        assert oracle_plan(doc, x) == COMP_PLANS[x], x


# ------------------------------------------------------------------ tile edges
TILE = 1024  # kSqTile (csrc/snapshot_query.hip): the nodes one step of the drain kernel's walk covers


def edge_doc(n_nodes, rooms, cands):
    """n_nodes nodes of 100m cpu, on which no subject (500m) fits; rooms: {node: cpu milli} for the nodes
    that admit some; cands: {node: subjects}, pods of 500m bound there in ascending node order."""
    names = [f"node-{i:07d}" for i in range(n_nodes)]
    nodes = [g.node_obj(names[i], rooms.get(i, 100), 32 * g.Gi, pods=8) for i in range(n_nodes)]
    pods = [g.pod_obj(f"s{x}-{j}", [g.req(500, g.Gi)], node=names[x]) for x in sorted(cands) for j in range(cands[x])]
    return {"profile": g.make_profile(bf.HAND_PLUGINS, 7), "nodes": nodes, "pods": pods,
            "queue": [g.pod_obj("q-small", [g.req(50, 64 * g.Mi)])]}


def edge_cases(n_nodes):
    """[(rooms, cands, expected plan destinations per candidate)]: the only admitting destination on node 0,
    on the last node, on the last node of tile 0 and on the first node of tile 1, with the candidates node 0,
    the last node and the nodes directly before and after the destination (a candidate that is the
    destination itself finds nothing); then a drain whose placements lie in two tiles (three from
    2 * TILE nodes on): one pod of room on the last node of tile 0, two on the first of tile 1, one on the
    last node."""
    out = []
    for d in sorted({0, n_nodes - 1, TILE - 1, TILE}):
        if d >= n_nodes:
            continue
        cands = {x: 2 for x in (0, n_nodes - 1, d - 1, d + 1) if 0 <= x < n_nodes}
        out.append(({d: 8000}, cands, {x: [-1, -1] if x == d else [d, d] for x in cands}))
    if n_nodes > TILE:
        rooms = {TILE - 1: 600, TILE: 1000}
        want = [TILE - 1, TILE, TILE]
        if n_nodes - 1 > TILE:
            rooms[n_nodes - 1] = 500
            want.append(n_nodes - 1)
        out.append((rooms, {5: 5, TILE + 1 if TILE + 1 < n_nodes - 1 else 6: 1},
                    {5: (want + [-1, -1])[:5], TILE + 1 if TILE + 1 < n_nodes - 1 else 6: [TILE - 1]}))
    return out


# The first-hit rotation (k_drain's tile step, csrc/drain.hip; SqFirstHit in csrc/snapshot_query.hip states
# the argument): a tile step uses one of three LDS words,
# chosen by a count of the steps since the drain began.  None of edge_cases' drains goes back to a lower tile
# (its subjects are all alike, so their destinations only ascend); here they differ in size.  Three tiles; the
# only rooms are 1000m on node 7 (tile 0), 4000m on T + 5 (tile 1), 16000m on the last node (tile 2).
# A subject of 200m hits in tile 0 (one step), of 1500m in tile 1 (an empty step, a hit), of 5000m in
# tile 2 (two empty steps, a hit), of 20000m nowhere (three empty steps).
ROTATION_X = 3
ROTATION_CPU = [200, 5000, 20000, 1500, 1500, 200, 5000, 20000]
ROTATION_PLAN = [(0, 7), (1, 2 * TILE + 51), (2, -1), (3, TILE + 5), (4, TILE + 5), (5, 7), (6, 2 * TILE + 51), (7, -1)]
ROTATION_DRAIN = Drain(8, 0, 6, 2, 0, 2, 3)


def rotation_doc():
    doc = edge_doc(2 * TILE + 52, {7: 1000, TILE + 5: 4000, 2 * TILE + 51: 16000}, {})
    name = doc["nodes"][ROTATION_X]["metadata"]["name"]
    doc["pods"] = [g.pod_obj(f"r{j}", [g.req(cpu, g.Gi)], node=name) for j, cpu in enumerate(ROTATION_CPU)]
    return doc


def rotation_steps(plan, n_tiles=3):
    """[(step count % 3, found)] of the tile steps a plan's subjects take, in order: a subject walks the
    tiles from 0 up to its destination's, or all of them if it has none."""
    out = []
    for _, dest in plan:
        last = dest // TILE if dest >= 0 else n_tiles - 1
        for t in range(last + 1):
            out.append((len(out) % 3, dest >= 0 and t == last))
    return out


def test_first_hit_rotation():
    """The literal plan equals the model and the oracle; over it the step count passes every residue both
    with a hit and without, and the subjects' step counts (1, 3, 3, 2, 2, 1, 3, 3) have no period of 3."""
    doc = rotation_doc()
    assert simulate(doc, ROTATION_X) == (ROTATION_DRAIN, ROTATION_PLAN)
    assert oracle_plan(doc, ROTATION_X) == ROTATION_PLAN
    steps = rotation_steps(ROTATION_PLAN)
    assert steps[:4] == [(0, True), (1, False), (2, False), (0, True)] and len(steps) == 18
    assert set(steps) == {(r, f) for r in range(3) for f in (False, True)}


@pytest.mark.parametrize("n_nodes", [TILE - 1, TILE, TILE + 1, 2 * TILE + 52])
def test_tile_shapes(n_nodes):
    """The tile-edge builders: the literal destinations equal the model; one candidate of each against the oracle."""
    for rooms, cands, want in edge_cases(n_nodes):
        doc = edge_doc(n_nodes, rooms, cands)
        state = bf.usage(doc)
        for x in cands:
            assert [d for _, d in simulate(doc, x, state=state)[1]] == want[x], (rooms, x)
        x = max(cands, key=lambda c: (cands[c], c))
        assert [d for _, d in oracle_plan(doc, x)] == want[x], (rooms, x)


# ------------------------------------------------------------------ generated clusters
def family_doc(cfg, n_nodes, per_node=5, n_queue=24):
    """test_bound_fit_model.family_doc with more pods a node: pod limits of 5..8 before the oracle places
    per_node x n_nodes queue pods; every 6th bound pod is then DaemonSet-owned and every 17th a mirror pod;
    the same drift afterwards (taints, cordons, cpu cuts, pod limits cut, labels lost)."""
    n_bound = per_node * n_nodes
    doc = g.generate(cfg, n_nodes=n_nodes, n_pods=n_bound + n_queue)
    for i, n in enumerate(doc["nodes"]):
        for k in ("allocatable", "capacity"):
            n["status"][k]["pods"] = str(5 + i % 4)
    o = Oracle(doc)
    order = o.ordered_queue(doc)
    o.schedule(n_bound, record=0)
    placed = []
    for q in range(n_bound):
        sel, _, st = o.result(q)
        if st == 0 and sel >= 0:
            p = copy.deepcopy(order[q])
            p["spec"]["nodeName"] = doc["nodes"][sel]["metadata"]["name"]
            placed.append(p)
    pods = [daemon_owned(p) if b % 6 == 5 else mirror(p) if b % 17 == 3 else p
            for b, p in enumerate(doc["pods"] + placed)]
    doc = {"profile": doc["profile"], "nodes": copy.deepcopy(doc["nodes"]), "pods": pods, "queue": order[n_bound:]}
    for i, n in enumerate(doc["nodes"]):
        if i % 7 == 3:
            n["spec"].setdefault("taints", []).append({"key": "drift", "value": "x", "effect": "NoSchedule"})
        if i % 11 == 5:
            n["spec"]["unschedulable"] = True
        if i % 5 == 1:
            for k in ("allocatable", "capacity"):
                n["status"][k]["cpu"] = f"{quantity('cpu', n['status'][k]['cpu']) * 4 // 10}m"
        if i % 9 == 4:
            for k in ("allocatable", "capacity"):
                n["status"][k]["pods"] = "1"
        if i % 13 == 2:
            n["metadata"]["labels"] = {g.HOSTNAME: n["metadata"]["name"]}
    return doc


@functools.lru_cache(maxsize=None)
def cfg2_doc():
    return family_doc(2, 200)


@functools.lru_cache(maxsize=None)
def cfg3_doc():
    return family_doc(3, 240)


@functools.lru_cache(maxsize=None)
def family_model(family):
    return simulate_all(cfg2_doc() if family == "cfg2" else cfg3_doc())


@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_generated_families(family):
    doc = cfg2_doc() if family == "cfg2" else cfg3_doc()
    model = family_model(family)
    assert len(doc["pods"]) >= 4 * len(doc["nodes"])
    ds = [d for d, _ in model]
    # the clusters hold what the feature is about: drains that succeed, drains that do not, pods left in place,
    # a drain whose placements share a destination (the overlay decides), one that spreads over several
    assert any(d.pods and drainable(d) for d in ds) and any(d.unplaced for d in ds) and any(d.daemon for d in ds)
    assert any(d.placed > d.dest_nodes >= 1 for d in ds) and any(d.dest_nodes >= 2 for d in ds)
    # a few nodes against the oracle: the first with an unplaced subject, the first that drains with several
    # subjects, the busiest, the last with pods
    want = [next(x for x, d in enumerate(ds) if d.unplaced and d.placed),
            next(x for x, d in enumerate(ds) if drainable(d) and d.placed >= 2),
            max(range(len(ds)), key=lambda x: ds[x].placed),
            max(x for x, d in enumerate(ds) if d.pods > d.daemon)]
    for x in want:
        assert oracle_plan(doc, x) == model[x][1], x
