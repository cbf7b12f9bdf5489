"""Set drain (ksg_drain_sets / ksg_drain_prefixes / ksg_drain_set_plan, include/ksg.h):
the references the GPU tests use, checked against each other on the CPU.

A set's subjects -- its nodes in list order, within a node the drain subjects of
test_drain_model -- are re-placed one after another: each on the lowest node
outside the set whose verdict is "passed", and counted there (requests and pod
count) before the next is judged, from whichever member it came.

1. The model (simulate_set): a few lines over test_bound_fit_model.reference, as
   test_drain_model.simulate is.
2. Hand-written literals (SETS) for sets of the competition cluster of
   test_drain_model.  That cluster has two drainable nodes with pods, 4 and 6, and
   they are removable together in either order, so the pair "each drainable alone,
   not together" needs two nodes more: rival_doc() is comp_doc() with nodes 11 and
   12 appended, one pod of 3000m each; node 3 has the only 3000m.  Every literal of
   test_drain_model holds on it unchanged (asserted below).
3. The ORACLE as an experiment (oracle_set_plan), in the style of
   test_drain_model.oracle_plan.

No GPU and no engine call.  The document builders of the GPU tests live here, and
what those tests rely on is asserted here.
"""
import copy
import functools
import random
from collections import Counter, namedtuple

import pytest

from ksg import generator as g
from test_headroom_model import pod_requests
import test_bound_fit_model as bf
import test_drain_model as dm

DrainSet = namedtuple("DrainSet", "pods daemon placed unplaced skipped first_unplaced first_blocked dest_nodes")
EMPTY = DrainSet(0, 0, 0, 0, 0, -1, -1, 0)
SET_NODES = 128
TILE = dm.TILE


def simulate_set(doc, nodes, cap=dm.DRAIN_MAX, n_subjects=None, state=None):
    """(DrainSet, plan) of the set `nodes`, a list of distinct node indices, in its order."""
    used, cnt = state or bf.usage(doc)
    used, cnt = Counter(used), Counter(cnt)
    here = [(b, pos) for pos, x in enumerate(nodes) for b in dm.on_node(doc, x, n_subjects)]
    subjects = [(b, pos) for b, pos in here if not dm.stays(doc["pods"][b])]
    members = set(nodes)
    plan = []
    for b, _ in subjects[:cap]:
        verdicts = bf.reference(doc, b, (used, cnt))
        dest = next((n for n, v in enumerate(verdicts) if v == "passed" and n not in members), -1)
        plan.append((b, dest))
        if dest >= 0:
            name = doc["nodes"][dest]["metadata"]["name"]
            cnt[name] += 1
            for k, v in pod_requests(doc["pods"][b]).items():
                used[(name, k)] += v
    plan += [(b, -2) for b, _ in subjects[cap:]]
    gone = [d for _, d in plan if d >= 0]
    lost = [b for b, d in plan if d == -1]
    blocked = [pos for (_, pos), (_, d) in zip(subjects, plan) if d < 0]
    return DrainSet(len(here), len(here) - len(subjects), len(gone), len(lost), len(subjects[cap:]),
                    lost[0] if lost else -1, blocked[0] if blocked else -1, len(set(gone))), plan


def removable(d):
    return d.unplaced == 0 and d.skipped == 0


def as_set(d, blocked=None):
    """test_drain_model's Drain as the DrainSet of the one-node set: first_blocked is 0 when a subject is
    unplaced or skipped."""
    return DrainSet(d.pods, d.daemon, d.placed, d.unplaced, d.skipped, d.first_unplaced,
                    (0 if d.unplaced or d.skipped else -1) if blocked is None else blocked, d.dest_nodes)


def oracle_set_plan(doc, nodes):
    """The same plan from oracle cycles: before subject b the earlier subjects are bound to their
    destinations (an unplaced one stays where it is); b, unbound, runs one cycle on the document without it."""
    d = {"profile": doc["profile"], "nodes": doc["nodes"], "pods": copy.deepcopy(doc["pods"]), "queue": doc["queue"]}
    plan = []
    for x in nodes:
        for b in dm.on_node(doc, x):
            if dm.stays(doc["pods"][b]):
                continue
            verdicts = bf.oracle_verdicts(d, b)
            dest = next((n for n, v in enumerate(verdicts) if v == "passed" and n not in nodes), -1)
            plan.append((b, dest))
            if dest >= 0:
                d["pods"][b]["spec"]["nodeName"] = doc["nodes"][dest]["metadata"]["name"]
    return plan


# ------------------------------------------------------------------ the competition cluster
@functools.lru_cache(maxsize=None)
def rival_doc():
    """comp_doc() with two nodes more: 11 and 12, 100m left on each, holding bound pods 20 (c1) and 21 (c2)
    of 3000m.  Alone each goes to node 3, the only node with 3000m; together the second finds 1000m there."""
    base = dm.comp_doc()
    names = [f"node-{i:07d}" for i in (11, 12)]
    nodes = base["nodes"] + [g.node_obj(n, 3100, 32 * g.Gi, pods=8) for n in names]
    pods = base["pods"] + [g.pod_obj(f"c{i + 1}", [g.req(3000, g.Gi)], node=n) for i, n in enumerate(names)]
    return {"profile": base["profile"], "nodes": nodes, "pods": pods, "queue": base["queue"]}


# (nodes, DrainSet(pods, daemon, placed, unplaced, skipped, first_unplaced, first_blocked, dest_nodes), plan); on
# rival_doc(); the sets without node 11 or 12 give the same on comp_doc()
SETS = [
    # 11 and 12 are each drainable alone (c1 -> 3, c2 -> 3) and not together: they compete for node 3's room
    ([11, 12], DrainSet(2, 0, 1, 1, 0, 21, 1, 1), [(20, 3), (21, -1)]),
    ([12, 11], DrainSet(2, 0, 1, 1, 0, 20, 1, 1), [(21, 3), (20, -1)]),
    # node 4 is a destination of node 6's own drain (z4 -> 4).  6 first: z1 -> 0, z2, z3 -> 3 (3 of 3 pods), z4
    # passes 4 by and lands on 5; b1 finds 3 full and takes 5's 2000, b2 goes on to 8, b3 to 7's 1700
    ([6, 4], DrainSet(7, 0, 7, 0, 0, -1, -1, 5), [(9, 0), (10, 3), (11, 3), (12, 5), (5, 5), (6, 8), (7, 7)]),
    # 4 first: b1, b2 fill node 3 (4000, 3 of 3 pods), b3 -> 5; z1 -> 0 (5 of 5 pods), the rest pass 3 and 4 by
    ([4, 6], DrainSet(7, 0, 7, 0, 0, -1, -1, 3), [(5, 3), (6, 3), (7, 5), (9, 0), (10, 5), (11, 5), (12, 5)]),
    # node 0's a2 is unplaced as in its own drain, and its a1 has taken node 3: node 4's pods move on
    ([0, 4], DrainSet(7, 2, 4, 1, 0, 3, 0, 4), [(1, 3), (3, -1), (5, 5), (6, 8), (7, 7)]),
    # nodes 8 and 9 take g1 and g2 of node 7's own drain; with 8 in the set only 9's gpu is left
    ([7, 8], DrainSet(4, 0, 1, 3, 0, 14, 0, 1), [(13, 9), (14, -1), (15, -1), (16, -1)]),
    # two empty members (tainted, cordoned) and node 10: r10 is rejected, the simulation goes on
    ([1, 10, 2], DrainSet(2, 0, 1, 1, 0, 18, 1, 1), [(18, -1), (19, 0)]),
]
ORDERED_PAIR = (6, 4)


def test_competition_set_literals():
    doc, comp = rival_doc(), dm.comp_doc()
    assert len(doc["nodes"]) == 13 and len(doc["pods"]) == 22 and len(SETS) >= 4
    # the two nodes more leave every literal of the competition cluster as it is; alone both are drainable
    alone = dm.simulate_all(doc)
    assert [d for d, _ in alone[:11]] == dm.COMP and [p for _, p in alone[:11]] == dm.COMP_PLANS
    assert alone[11] == (dm.Drain(1, 0, 1, 0, 0, -1, 1), [(20, 3)])
    assert alone[12] == (dm.Drain(1, 0, 1, 0, 0, -1, 1), [(21, 3)])
    state = bf.usage(doc)
    for nodes, want, plan in SETS:
        assert simulate_set(doc, nodes, state=state) == (want, plan), nodes
        if max(nodes) < 11:
            assert simulate_set(comp, nodes) == (want, plan), nodes
    by_nodes = {tuple(n): (d, p) for n, d, p in SETS}
    # a pair whose members are each drainable alone and not together
    assert dm.drainable(alone[11][0]) and dm.drainable(alone[12][0]) and not removable(by_nodes[(11, 12)][0])
    # a pair where one member is the other's destination in its own drain; both orders, different plans,
    # and the later member's subjects find other nodes than in its own drain
    a, b = ORDERED_PAIR
    assert b in [d for _, d in dm.COMP_PLANS[a]]
    assert dict(by_nodes[(a, b)][1]) != dict(by_nodes[(b, a)][1])
    assert by_nodes[(a, b)][0].dest_nodes != by_nodes[(b, a)][0].dest_nodes
    assert removable(by_nodes[(a, b)][0]) and removable(by_nodes[(b, a)][0])
    # no member is a destination, neither an earlier nor a later one
    for nodes, _, plan in SETS:
        assert not {d for _, d in plan} & set(nodes)


def test_singletons_equal_the_drain_model():
    for doc in (dm.comp_doc(), rival_doc()):
        state = bf.usage(doc)
        for x in range(len(doc["nodes"])):
            d, plan = dm.simulate(doc, x, state=state)
            assert simulate_set(doc, [x], state=state) == (as_set(d), plan), x
    d, plan = dm.simulate(dm.comp_doc(), 6, cap=2)
    assert simulate_set(dm.comp_doc(), [6], cap=2) == (as_set(d), plan) and as_set(d).first_blocked == 0


def test_empty_and_cap_in_the_model():
    doc = dm.comp_doc()
    assert simulate_set(doc, []) == (EMPTY, []) and simulate_set(doc, [1, 2]) == (EMPTY, [])
    d, plan = simulate_set(doc, [4, 6], cap=4)
    assert d == DrainSet(7, 0, 4, 0, 3, -1, 1, 3) and [x for _, x in plan] == [3, 3, 5, 0, -2, -2, -2]


def test_competition_sets_oracle_experiment():
    doc = rival_doc()
    for nodes, _, plan in SETS:
        assert oracle_set_plan(doc, nodes) == plan, nodes


def prefixes(doc, nodes, cap=dm.DRAIN_MAX, n_subjects=None):
    state = bf.usage(doc)
    return [simulate_set(doc, nodes[:k + 1], cap, n_subjects, state)[0] for k in range(len(nodes))]


def test_prefixes_of_the_competition_cluster():
    """Prefix k is the set nodes[:k + 1], simulated from the start: a longer prefix excludes more
    destinations, so it does not continue the shorter one."""
    doc = rival_doc()
    nodes = [6, 4, 11, 12, 0]
    got = prefixes(doc, nodes)
    assert got[0] == as_set(dm.COMP[6]) and got[1] == SETS[2][1]
    # z2 and z3 have used node 3's pod room: c1, which goes there in its own drain, finds it full; so do c2, a1, a2
    assert got[2] == DrainSet(8, 0, 7, 1, 0, 20, 2, 5) and got[3] == DrainSet(9, 0, 7, 2, 0, 20, 2, 5)
    # with node 0 in the set z1 goes to 3 as well: z1, z2 -> 3, z3, z4, b1 -> 5, b2 -> 8, b3 -> 7
    assert got[4] == DrainSet(13, 2, 7, 4, 0, 20, 2, 4)
    # z4 goes to node 4 in prefix 0 and cannot in prefix 1
    assert simulate_set(doc, nodes[:1])[1][3] == (12, 4) and simulate_set(doc, nodes[:2])[1][3] == (12, 5)


# ------------------------------------------------------------------ tile edges
def set_edge_cases(n_nodes):
    """[(rooms, cands, nodes, plan)] on test_drain_model.edge_doc (nodes of 100m, subjects of 500m; bound
    indices ascend with the node).  T = 1024 nodes a tile.
    A: the members are nodes 0, T - 1, T and the last node (those the snapshot holds), each with 8000m: the
       lowest nodes with room in their tiles, and no destinations.  The room outside the set: one subject on
       node 1, two on T + 1, two on 2T + 3 (where the snapshot holds them): overlay entries in up to three
       tiles.  The list is given in descending node order.
    B: member T - 1 with room; the destination is T, the next tile's first node.
    C: members T and 0 with room, in this order; the destination is T - 1, the previous tile's last node."""
    T = TILE
    out = []
    members = sorted({x for x in (0, T - 1, T, n_nodes - 1) if x < n_nodes})
    rooms = {x: 8000 for x in members}
    rooms.update({d: cpu for d, cpu in ((1, 600), (T + 1, 1000), (2 * T + 3, 1000)) if d < n_nodes - 1})
    cands = {x: 2 for x in members}
    bound = {}
    for x in members:
        bound[x] = list(range(len(bound) * 2, len(bound) * 2 + 2))
    order = members[::-1]
    dests = [d for d in (1, T + 1, T + 1, 2 * T + 3, 2 * T + 3) if d < n_nodes - 1]
    subjects = [b for x in order for b in bound[x]]
    out.append((rooms, cands, order, list(zip(subjects, dests + [-1] * (len(subjects) - len(dests))))))
    if n_nodes > T:
        out.append(({T - 1: 8000, T: 600}, {T - 1: 2}, [T - 1], [(0, T), (1, -1)]))
        out.append(({0: 8000, T: 8000, T - 1: 600}, {0: 1, T: 1}, [T, 0], [(1, T - 1), (0, -1)]))
    return out


@pytest.mark.parametrize("n_nodes", [TILE - 1, TILE, TILE + 1, 2100])
def test_set_tile_shapes(n_nodes):
    cases = set_edge_cases(n_nodes)
    assert len(cases) == (3 if n_nodes > TILE else 1)
    for rooms, cands, nodes, plan in cases:
        doc = dm.edge_doc(n_nodes, rooms, cands)
        d, got = simulate_set(doc, nodes)
        assert got == plan, (rooms, nodes, got)
        # every member has room for all subjects and the lowest node with room is a member: skipped, not missed
        assert all(rooms.get(x, 0) >= 8000 for x in nodes) and min(rooms) in nodes
        assert d.placed + d.unplaced == sum(cands.values()) and d.unplaced >= 1
    rooms, cands, nodes, plan = cases[0]
    assert {0, n_nodes - 1} <= set(nodes) and nodes == sorted(nodes, reverse=True)
    if n_nodes == 2100:
        assert len({d // TILE for _, d in plan if d >= 0}) == 3 and len(nodes) == 4
        assert oracle_set_plan(dm.edge_doc(n_nodes, rooms, cands), nodes) == plan
    if n_nodes > TILE:
        for rooms, cands, nodes, plan in cases[1:]:
            assert abs(plan[0][1] - nodes[0]) == 1 and plan[0][1] // TILE != nodes[0] // TILE  # across the tile edge


# ------------------------------------------------------------------ the hash overlay
HASH_CAP = 4  # KSG_DRAIN_MAX=4 at ksg_create: 2 x 4 slots


def hash_doc(dests, n_nodes=48):
    """Members 1 and 2 with three subjects of 500m each; the nodes of `dests` have 600m, room for one."""
    return dm.edge_doc(n_nodes, {d: 600 for d in dests}, {1: 3, 2: 3})


# the destinations in node order, which is the order the subjects take them in
HASH_CASES = {
    # home slots 5, 5, 5, 7: 13 and 21 are pushed to slots 6 and 7, 31 finds 7 taken and wraps to 0
    "chain_then_wrap": [5, 13, 21, 31],
    # home slots 7, 7, 7, 0: 15 wraps to 0 and 23 to 1 at once; 40 is pushed from 0 to 2
    "wrap_then_chain": [7, 15, 23, 40],
}


def table_slots(dests, slots=2 * HASH_CAP):
    """[(home, slot)] of the keys inserted in order: open addressing, linear probing with wrap-around."""
    table, out = {}, []
    for d in dests:
        s = d % slots
        while s in table:
            s = (s + 1) % slots
        table[s] = d
        out.append((d % slots, s))
    return out


def test_hash_cases_collide():
    assert table_slots(HASH_CASES["chain_then_wrap"]) == [(5, 5), (5, 6), (5, 7), (7, 0)]
    assert table_slots(HASH_CASES["wrap_then_chain"]) == [(7, 7), (7, 0), (7, 1), (0, 2)]
    for name, dests in HASH_CASES.items():
        d, d8, d16, last = dests
        assert (d8, d16) == (d + 8, d + 16)
        doc = hash_doc(dests)
        want, plan = simulate_set(doc, [1, 2], cap=HASH_CAP)
        # each destination takes one subject: the next subject has to find every earlier entry again (at
        # probe distances 0, 1 and 2) and be refused by the lowered rows, or it would stop at the first
        assert plan == list(zip(range(6), dests + [-2, -2]))
        assert want == DrainSet(6, 0, 4, 0, 2, -1, 1, 4) and not removable(want)
        # without the cap the last two subjects are simulated and find nothing
        full, plan = simulate_set(doc, [1, 2])
        assert [x for _, x in plan] == dests + [-1, -1] and full == DrainSet(6, 0, 4, 2, 0, 4, 1, 4)
        # were an entry not found, the subject would land on a node that is full
        assert [x for _, x in simulate_set(doc, [1])[1]] == dests[:3]
    assert oracle_set_plan(hash_doc(HASH_CASES["chain_then_wrap"]), [1, 2])[:4] == list(
        zip(range(4), HASH_CASES["chain_then_wrap"]))


# ------------------------------------------------------------------ limits
def limit_doc(n_nodes=140):
    """Every node 4k + 1 below 129 holds one subject of 500m; nodes 130 to 133 take eight each (their pod limit)."""
    return dm.edge_doc(n_nodes, {130 + i: 4100 for i in range(4)}, {x: 1 for x in range(1, 129, 4)})


def test_limit_shape():
    doc = limit_doc()
    d, plan = simulate_set(doc, list(range(SET_NODES)))
    assert d == DrainSet(32, 0, 32, 0, 0, -1, -1, 4) and [x for _, x in plan] == [130 + b // 8 for b in range(32)]
    d, plan = simulate_set(doc, list(range(SET_NODES))[::-1])
    assert d.placed == 32 and [b for b, _ in plan] == list(range(32))[::-1]


# ------------------------------------------------------------------ generated clusters
def family_sets(family, n_sets=24, seed=20):
    """Seeded sets of 1 to 12 distinct nodes, in drawn order: the odd ones from the nodes that hold pods
    and are drainable alone (test_drain_model.family_model), the even ones from every node."""
    doc = dm.cfg2_doc() if family == "cfg2" else dm.cfg3_doc()
    model = dm.family_model(family)
    rng = random.Random(seed + (2 if family == "cfg2" else 3))
    alone = [x for x, (d, _) in enumerate(model) if d.pods > d.daemon and dm.drainable(d)]
    every = list(range(len(doc["nodes"])))
    return [rng.sample(alone if i % 2 else every, 1 + i * 5 % 12) for i in range(n_sets)]


@functools.lru_cache(maxsize=None)
def family_set_model(family):
    doc = dm.cfg2_doc() if family == "cfg2" else dm.cfg3_doc()
    state = bf.usage(doc)
    return [simulate_set(doc, nodes, state=state) for nodes in family_sets(family)]


def rivals(family):
    """The sets that are not removable although every member is drainable alone."""
    alone = dm.family_model(family)
    return [i for i, (nodes, (d, _)) in enumerate(zip(family_sets(family), family_set_model(family)))
            if d.unplaced and all(dm.drainable(alone[x][0]) for x in nodes)]


@pytest.mark.parametrize("family", ["cfg2", "cfg3"])
def test_generated_family_sets(family):
    doc = dm.cfg2_doc() if family == "cfg2" else dm.cfg3_doc()
    sets, model = family_sets(family), family_set_model(family)
    assert len(sets) == 24 and all(1 <= len(s) <= 12 and len(set(s)) == len(s) for s in sets)
    assert {1, 12} <= {len(s) for s in sets}
    ds = [d for d, _ in model]
    # what the feature is about: sets that can go, sets that cannot, and a set of nodes that can each go alone
    # and cannot together
    assert any(removable(d) and d.placed for d in ds) and any(d.unplaced for d in ds) and any(d.daemon for d in ds)
    assert rivals(family), "no set of individually drainable nodes is blocked"
    assert any(d.dest_nodes >= 4 for d in ds)
    # the first blocked set of individually drainable nodes and the largest set against the oracle
    for i in (rivals(family)[0], max(range(len(sets)), key=lambda i: ds[i].placed)):
        assert oracle_set_plan(doc, sets[i]) == model[i][1], i


PREFIX_NODES = 24


def prefix_nodes():
    """24 nodes of cfg2_doc() in a seeded order: the candidate list of a consolidation pass."""
    return random.Random(7).sample(range(len(dm.cfg2_doc()["nodes"])), PREFIX_NODES)


@functools.lru_cache(maxsize=None)
def prefix_model():
    return prefixes(dm.cfg2_doc(), prefix_nodes())


def test_prefix_model():
    got = prefix_model()
    assert len(got) == PREFIX_NODES
    # pods and daemon accumulate; once a prefix is blocked at position p every longer one is blocked at or before p
    assert all(a.pods <= b.pods and a.daemon <= b.daemon for a, b in zip(got, got[1:]))
    assert any(removable(d) for d in got) and any(not removable(d) for d in got)
    blocked = [d.first_blocked for d in got if d.first_blocked >= 0]
    assert blocked and all(d.first_blocked <= k for k, d in enumerate(got))
