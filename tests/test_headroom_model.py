"""Headroom (ksg_headroom, include/ksg.h): the two references the GPU tests use,
checked against each other on the CPU.

1. The ORACLE as a filling experiment (oracle_fill): the queue is replaced by K
   distinctly named copies of the pod and scheduled; the scheduled copies are the
   replicas and the Counter of their nodes the per-node row.  The greedy fill ends
   with every node at its count whatever the scoring order, provided K exceeds the
   total, so every fill asserts that at least one copy stayed unschedulable.
2. A few lines of Python integers over the document (reference): allocatable, the
   bound pods' requests, the pod limits, and the static filters restated from the
   v1.Pod / v1.Node fields.  It gives bound[], open_nodes, max_node, best_node,
   which no fill shows.  It is pinned here against the fill and against
   hand-written literals.

No GPU and no engine call: these pass without a device.  The document builders
of the GPU tests live here too, so the fill condition is checked on the CPU for
every shape the GPU tests use.
"""
import copy
import functools
from collections import Counter, namedtuple

import pytest

from _oracle import Oracle
from ksg import generator as g
from ksg.generator import _expr_ok, _tolerates

Headroom = namedtuple("Headroom", "replicas nodes open_nodes max_node best_node bound")
BOUNDS = 9
BASE = ["cpu", "memory", "ephemeral-storage"]
STATIC = ("TaintToleration", "NodeAffinity", "NodeUnschedulable", "NodeName")
UNSCHED_TAINT = {"key": "node.kubernetes.io/unschedulable", "effect": "NoSchedule"}


def quantity(name, s):
    """A resource quantity in the engine's unit: cpu in milli, everything else as a number."""
    s = str(s)
    for suf, mul in (("Ki", 1 << 10), ("Mi", 1 << 20), ("Gi", 1 << 30), ("Ti", 1 << 40)):
        if s.endswith(suf):
            return int(s[:-2]) * mul
    if s.endswith("m"):
        assert name == "cpu"
        return int(s[:-1])
    return int(s) * (1000 if name == "cpu" else 1)


def pod_requests(pod):
    out = Counter()
    for c in pod["spec"]["containers"]:
        for k, v in c.get("resources", {}).get("requests", {}).items():
            out[k] += quantity(k, v)
    return out


def pending(doc):
    return doc["queue"]


def columns(doc):
    """Resource column names: cpu, memory, ephemeral-storage, then the scalars by name."""
    scal = set()
    for n in doc["nodes"]:
        scal |= set(n["status"]["allocatable"]) - set(BASE) - {"pods"}
    for p in doc["pods"] + pending(doc):
        scal |= set(pod_requests(p)) - set(BASE)
    return BASE + sorted(scal)


def static_open(pod, node, plugins):
    """Does the node pass the profile's Filters other than NodeResourcesFit (PreFilterResult included)?"""
    spec, lab = pod["spec"], node["metadata"]["labels"]
    tols = spec.get("tolerations", [])
    if "TaintToleration" in plugins:
        if any(t["effect"] in ("NoSchedule", "NoExecute") and not _tolerates(tols, t)
               for t in node["spec"].get("taints", [])):
            return False
    if "NodeAffinity" in plugins:
        if any(lab.get(k) != v for k, v in spec.get("nodeSelector", {}).items()):
            return False
        req = spec.get("affinity", {}).get("nodeAffinity", {}).get("requiredDuringSchedulingIgnoredDuringExecution")
        if req is not None:
            def term(t):
                fields = all(f["key"] == "metadata.name" and f["operator"] == "In" and
                             f["values"] == [node["metadata"]["name"]] for f in t.get("matchFields", []))
                return fields and all(_expr_ok(e, lab) for e in t.get("matchExpressions", []))
            if not any(term(t) for t in req["nodeSelectorTerms"]):
                return False
    if "NodeUnschedulable" in plugins:
        if node["spec"].get("unschedulable") and not _tolerates(tols, UNSCHED_TAINT):
            return False
    if "NodeName" in plugins:
        if spec.get("nodeName") and spec["nodeName"] != node["metadata"]["name"]:
            return False
    return True


def reference(doc, pod):
    """(Headroom, per-node row) of `pod` on the document's nodes and bound pods."""
    cols, plugins = columns(doc), doc["profile"]["plugins"]
    assert "NodeResourcesFit" in plugins
    used, cnt = Counter(), Counter()
    for p in doc["pods"]:
        cnt[p["spec"]["nodeName"]] += 1
        for k, v in pod_requests(p).items():
            used[(p["spec"]["nodeName"], k)] += v
    want = pod_requests(pod)
    row, bound, n_open = [], [0] * BOUNDS, 0
    for node in doc["nodes"]:
        name, alloc = node["metadata"]["name"], node["status"]["allocatable"]
        if not static_open(pod, node, plugins):
            row.append(0)
            continue
        n_open += 1
        limits = [max(0, quantity("pods", alloc["pods"]) - cnt[name])]
        for r, col in enumerate(cols):
            if want[col] > 0:
                free = quantity(col, alloc.get(col, 0)) - used[(name, col)]
                limits.append((0 if free < 0 else free // want[col], 1 + r))
        best, which = limits[0], 0
        for v, i in limits[1:]:
            if v < best:  # (a tie keeps the lower index)
                best, which = v, i
        bound[which] += 1
        row.append(best)
    mx = max(row, default=0)
    hr = Headroom(sum(row), sum(1 for c in row if c >= 1), n_open, mx, row.index(mx) if mx > 0 else -1, tuple(bound))
    return hr, row


def copies_doc(doc, pod, k):
    d = {key: doc[key] for key in ("profile", "nodes", "pods")}
    d["queue"] = []
    for i in range(k):
        p = copy.deepcopy(pod)
        p["metadata"]["name"] = f"copy-{i:06d}"
        d["queue"].append(p)
    return d


def oracle_fill(doc, pod, k):
    """(replicas, per-node row) from scheduling k copies of the pod with the oracle."""
    d = copies_doc(doc, pod, k)
    o = Oracle(d)
    assert o.n_queue == k
    o.schedule(record=0)
    res = [o.result(q) for q in range(k)]
    placed = Counter(sel for sel, _, st in res if st == 0 and sel >= 0)
    replicas = sum(placed.values())
    assert replicas < k, "the fill needs at least one copy left over"
    return replicas, [placed[i] for i in range(len(doc["nodes"]))]


def check_fill(doc, pod):
    """The reference equals the oracle fill for this pod; returns the reference."""
    hr, row = reference(doc, pod)
    assert max(row, default=0) <= 8, "keep the per-node counts small: K stays in the low thousands"
    replicas, orow = oracle_fill(doc, pod, hr.replicas + 3)
    assert (replicas, orow) == (hr.replicas, row)
    return hr, row


# ------------------------------------------------------------------ the hand-built cluster
GPU_TAINT = {"key": "dedicated", "value": "gpu", "effect": "NoSchedule"}
GPU = "example.com/gpu"


@functools.lru_cache(maxsize=None)
def hand_doc():
    """40 nodes under TaintToleration, NodeAffinity, NodeResourcesFit, BalancedAllocation.
    pod-a asks 2 cpu, 4Gi and disk=ssd; pod-z asks nothing (and no label); pod-g asks 1 cpu, 1Gi, 1 gpu and disk=ssd.
      0-5   taint dedicated=gpu (closed)            6-9    no disk label (closed for a and g)
      10-12 cordoned, with the taint the node controller puts on a cordoned node (closed)
      13-17 cpu-bound: 7 cpu, 64Gi -> a 3            18-21  memory-bound: 16 cpu, 10Gi -> a 2
      22-24 pod-limit-bound: limit 3, one in use -> 2 25-26  tie cpu / memory: 8 cpu, 16Gi -> a 4 (cpu wins)
      27    tie room / cpu: limit 4, 8 cpu -> a 4 (room wins)
      28-29 overcommitted: 4 cpu allocatable, 6 in use -> 0 (cpu)
      30-31 pod count above the limit: limit 1, two bound -> 0 (room)
      32-37 carry 2 gpu (16 cpu, 64Gi, limit 5) -> a 5 (room), g 2 (gpu); every other node has no gpu -> g 0
      38-39 16 cpu, 64Gi, limit 6 -> a 6 (room)"""
    big, ssd = 64 * g.Gi, {"disk": "ssd"}
    nodes, pods = [], []

    def add(cpu, mem, labels=ssd, taints=None, limit=8, used=(), scalars=None, cordon=False):
        name = f"node-{len(nodes):07d}"
        nodes.append(g.node_obj(name, cpu, mem, pods=limit, labels=labels, taints=taints, scalars=scalars,
                                unschedulable=cordon))
        for i, (c, m) in enumerate(used):
            pods.append(g.filler_pod(f"fill-{len(nodes) - 1:07d}-{i}", name, c, m))

    for _ in range(6):
        add(16000, big, taints=[GPU_TAINT])
    for _ in range(4):
        add(16000, big, labels=None)
    for _ in range(3):
        add(16000, big, taints=[dict(UNSCHED_TAINT)], cordon=True)
    for _ in range(5):
        add(7000, big)
    for _ in range(4):
        add(16000, 10 * g.Gi)
    for _ in range(3):
        add(16000, big, limit=3, used=[(100, 64 * g.Mi)])
    for _ in range(2):
        add(8000, 16 * g.Gi)
    add(8000, big, limit=4)
    for _ in range(2):
        add(4000, big, used=[(6000, g.Gi)])
    for _ in range(2):
        add(16000, big, limit=1, used=[(100, 64 * g.Mi), (100, 64 * g.Mi)])
    for _ in range(6):
        add(16000, big, limit=5, scalars={GPU: 2})
    for _ in range(2):
        add(16000, big, limit=6)
    assert len(nodes) == 40
    queue = [g.pod_obj("pod-a", [g.req(2000, 4 * g.Gi)], nodeSelector=ssd),
             g.pod_obj("pod-z", [{}]),
             g.pod_obj("pod-g", [g.req(1000, g.Gi, {GPU: "1"})], nodeSelector=ssd)]
    prof = g.make_profile([("TaintToleration", 3), ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                           ("NodeResourcesBalancedAllocation", 1)], 7)
    return {"profile": prof, "nodes": nodes, "pods": pods, "queue": queue}


def _row(*groups):
    out = []
    for n, v in groups:
        out += [v] * n
    return out


# columns: cpu, memory, ephemeral-storage, example.com/gpu -> bound index 1, 2, 3, 4
HAND_ROWS = [
    _row((6, 0), (4, 0), (3, 0), (5, 3), (4, 2), (3, 2), (2, 4), (1, 4), (2, 0), (2, 0), (6, 5), (2, 6)),
    _row((6, 0), (4, 8), (3, 0), (5, 8), (4, 8), (3, 2), (2, 8), (1, 4), (2, 7), (2, 0), (6, 5), (2, 6)),
    _row((6, 0), (4, 0), (3, 0), (5, 0), (4, 0), (3, 0), (2, 0), (1, 0), (2, 0), (2, 0), (6, 2), (2, 0)),
]
HAND = [
    # pod-a: 27 open (40 - 6 tainted - 4 unlabelled - 3 cordoned); room binds on 22-24, 27, 30-39, cpu on
    # 13-17, 25-26, 28-29, memory on 18-21
    Headroom(15 + 8 + 6 + 8 + 4 + 30 + 12, 23, 27, 6, 38, (3 + 1 + 2 + 6 + 2, 5 + 2 + 2, 4, 0, 0, 0, 0, 0, 0)),
    # pod-z: 31 open (no selector), the room alone; 28-29 hold one pod of their 8
    Headroom(32 + 40 + 32 + 6 + 16 + 4 + 14 + 30 + 12, 29, 31, 8, 6, (31, 0, 0, 0, 0, 0, 0, 0, 0)),
    # pod-g: the gpu is short on every open node without one, but room (30-31) and cpu (28-29) come first
    Headroom(12, 6, 27, 2, 32, (2, 2, 0, 0, 23, 0, 0, 0, 0)),
]


def test_hand_literals():
    doc = hand_doc()
    assert columns(doc) == BASE + [GPU]
    for q, pod in enumerate(doc["queue"]):
        hr, row = reference(doc, pod)
        assert row == HAND_ROWS[q], q
        assert hr == HAND[q], (q, hr)
        assert sum(hr.bound) == hr.open_nodes


def test_hand_oracle_fill():
    doc = hand_doc()
    for q, pod in enumerate(doc["queue"]):
        replicas, row = oracle_fill(doc, pod, HAND[q].replicas + 3)
        assert replicas == HAND[q].replicas and row == HAND_ROWS[q], q


def named_affinity(*terms):
    """Required node affinity: one term per argument, a list of node names, each name a matchFields
    requirement of its own (upstream takes exactly one value per matchFields requirement)."""
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [v]} for v in t]} for t in terms]}}}


@functools.lru_cache(maxsize=None)
def prefilter_doc():
    """The hand-built nodes under NodeUnschedulable, NodeName, TaintToleration, NodeAffinity, Fit, BA, and five
    pods of 2 cpu / 4Gi: a PreFilterResult of two nodes, spec.nodeName, a toleration of the cordon taint,
    a PreFilter rejection (one term whose two matchFields share no node), and a plain pod."""
    base = hand_doc()
    names = [n["metadata"]["name"] for n in base["nodes"]]
    cordon_tol = [{"key": UNSCHED_TAINT["key"], "operator": "Exists", "effect": "NoSchedule"}]
    doc = dict(base)
    doc["profile"] = g.make_profile([("NodeUnschedulable", 1), ("NodeName", 1), ("TaintToleration", 3),
                                     ("NodeAffinity", 2), ("NodeResourcesFit", 1),
                                     ("NodeResourcesBalancedAllocation", 1)], 7)
    c = [g.req(2000, 4 * g.Gi)]
    doc["queue"] = [g.pod_obj("two-nodes", c, affinity=named_affinity([names[13]], [names[38]])),
                    g.pod_obj("one-name", c, nodeName=names[25]),
                    g.pod_obj("cordon-ok", c, tolerations=cordon_tol),
                    g.pod_obj("rejected", c, affinity=named_affinity([names[13], names[38]])),
                    g.pod_obj("plain", c)]
    return doc


def test_prefilter_doc_fill():
    doc = prefilter_doc()
    rows = [check_fill(doc, p) for p in doc["queue"]]
    assert rows[0][1] == [3 if i == 13 else 6 if i == 38 else 0 for i in range(40)]
    assert rows[1][0][:3] == (4, 1, 1) and rows[1][0].best_node == 25
    assert rows[2][0].open_nodes == rows[4][0].open_nodes + 3 == 34
    assert rows[3][0] == Headroom(0, 0, 0, 0, -1, (0,) * 9)


# ------------------------------------------------------------------ generated clusters
def family_doc(cfg, n_nodes, n_pods, seed=None):
    """A cfg2- / cfg3-shaped generated cluster whose pod limits are 1..6 (node i: 1 + i % 6, so no
    per-node count passes 6)."""
    doc = g.generate(cfg, n_nodes=n_nodes, n_pods=n_pods, **({} if seed is None else {"seed": seed}))
    for i, n in enumerate(doc["nodes"]):
        for k in ("allocatable", "capacity"):
            n["status"][k]["pods"] = str(1 + i % 6)
    return doc


@functools.lru_cache(maxsize=None)
def cfg2_doc():
    return family_doc(2, 120, 60)


@functools.lru_cache(maxsize=None)
def cfg3_doc():
    return family_doc(3, 150, 60)


def shape_of(pod):
    """What a queue pod asks for, as far as the count's code paths see it."""
    spec = pod["spec"]
    na = spec.get("affinity", {}).get("nodeAffinity", {})
    return (tuple(sorted(k for k, v in pod_requests(pod).items() if v > 0)), len(spec["containers"]),
            bool(spec.get("tolerations")), bool(spec.get("nodeSelector")),
            "requiredDuringSchedulingIgnoredDuringExecution" in na)


def sample_pods(doc):
    """The first queue pod of every distinct shape."""
    seen, out = set(), []
    for q, p in enumerate(doc["queue"]):
        if shape_of(p) not in seen:
            seen.add(shape_of(p))
            out.append(q)
    return out


def tile_doc(n_nodes, n_pods):
    """The tile-edge clusters of the GPU test: cfg3-shaped (taints and selectors close most nodes,
    so the fills stay small) at a node count beside the kernel's node tile."""
    return family_doc(3, n_nodes, n_pods, seed=1234 + n_nodes)


def test_generated_cfg2_fill():
    doc = cfg2_doc()
    qs = sample_pods(doc)
    assert len(qs) >= 3  # BestEffort, one container, two containers
    for q in qs:
        hr, _ = check_fill(doc, doc["queue"][q])
        assert sum(hr.bound) == hr.open_nodes == len(doc["nodes"])


def test_generated_cfg3_fill():
    doc = cfg3_doc()
    for q in sample_pods(doc):
        hr, _ = check_fill(doc, doc["queue"][q])
        assert sum(hr.bound) == hr.open_nodes


@pytest.mark.parametrize("n_nodes", [1023, 1024, 1025, 2100])
def test_tile_shapes_fill(n_nodes):
    """The fill condition at the GPU tile-edge shapes, on one pod of the queue."""
    doc = tile_doc(n_nodes, 33)
    check_fill(doc, doc["queue"][0])
