"""The magnitude family (ksg.edge.gen_magnitude) on the CPU: NodeResourcesFit
(LeastAllocated, MostAllocated, RequestedToCapacityRatio) and
NodeResourcesBalancedAllocation recomputed here in Python integers and floats
from the document alone, for every (queue pod, node) the oracle scores against
the initial snapshot, and compared with the oracle's score-result annotation: the
engine is tested against the oracle (test_magnitude_gpu.py), so the two must not
share a mistake at these sizes.  Then the conditions that keep the family from
being vacuous, all computed from the document and the oracle.

A (pod, node, resource) triple is one leastRequestedScore quotient
x / a, x = (a - q) * 100, of the four-resource profile on a feasible pair with
q <= a.  div_small (csrc/engine.hip) takes its 32-bit branch when x and a are
below 2^32, its slow branch when x >= 2^52, its reciprocal estimate otherwise.
A triple sits on a quotient boundary when q and q + 1 give different floors,
i.e. x mod a < 100; only a >= 2^32 counts (below 100 every q is a boundary)."""
import functools
import json
import math

import pytest

from _oracle import Oracle
from ksg import edge

P = "kube-scheduler-simulator.sigs.k8s.io/"
FIT, BA = "NodeResourcesFit", "NodeResourcesBalancedAllocation"
FIT_PROFILES = ("default", "least4", "most", "rtc")
DOCS = [(k, None) for k in edge.MAGNITUDE_KINDS if k != "wc_gate"] + [("wc_gate", v) for v in edge.WC_GATE_VIOLATIONS]
IDS = [k if v is None else f"{k}-{v}" for k, v in DOCS]


def quantity(s, milli=False):
    s = str(s)
    for suf, mul in (("Gi", 1 << 30), ("Mi", 1 << 20), ("Ki", 1 << 10)):
        if s.endswith(suf):
            return int(s[:-2]) * mul
    if s.endswith("m"):
        assert milli
        return int(s[:-1])
    return int(s) * (1000 if milli else 1)


def pod_requests(pod):
    """(requests, non-zero cpu, non-zero memory): containers summed (the family has no
    init containers or overhead); a container without cpu / memory counts 100m / 200Mi."""
    tot, nzc, nzm = {}, 0, 0
    for c in pod["spec"]["containers"]:
        rq = {k: quantity(v, k == "cpu") for k, v in c.get("resources", {}).get("requests", {}).items()}
        for k, v in rq.items():
            tot[k] = tot.get(k, 0) + v
        nzc += rq.get("cpu", 0) or 100
        nzm += rq.get("memory", 0) or 200 << 20
    return tot, nzc, nzm


def snapshot(doc):
    nodes = {}
    for n in doc["nodes"]:
        al = {k: quantity(v, k == "cpu") for k, v in n["status"]["allocatable"].items()}
        nodes[n["metadata"]["name"]] = dict(alloc=al, req={}, nzc=0, nzm=0)
    for p in doc["pods"]:
        st = nodes[p["spec"]["nodeName"]]
        tot, nzc, nzm = pod_requests(p)
        for k, v in tot.items():
            st["req"][k] = st["req"].get(k, 0) + v
        st["nzc"] += nzc
        st["nzm"] += nzm
    return nodes


def alloc_req(st, pod, res, nonzero):
    """resource_allocation.go calculateResourceAllocatableRequest -> (allocatable, requested)."""
    tot, nzc, nzm = pod
    if res not in ("cpu", "memory", edge.EPH) and tot.get(res, 0) == 0:
        return 0, 0
    a = st["alloc"].get(res, 0)
    if res == "cpu":
        return a, (st["nzc"] + nzc) if nonzero else st["req"].get(res, 0) + tot.get(res, 0)
    if res == "memory":
        return a, (st["nzm"] + nzm) if nonzero else st["req"].get(res, 0) + tot.get(res, 0)
    return a, st["req"].get(res, 0) + tot.get(res, 0)


def go_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rtc_fn(shape, p):
    pts = [(s["utilization"], s["score"] * 10) for s in shape]
    for i, (u, sc) in enumerate(pts):
        if p <= u:
            if i == 0:
                return pts[0][1]
            return pts[i - 1][1] + go_div((sc - pts[i - 1][1]) * (p - pts[i - 1][0]), u - pts[i - 1][0])
    return pts[-1][1]


def fit_score(st, pod, args):
    ss = args["scoringStrategy"]
    ns = ws = 0
    for r in ss["resources"]:
        a, q = alloc_req(st, pod, r["name"], True)
        if a == 0:
            continue
        if ss["type"] == "LeastAllocated":
            s = 0 if q > a else (a - q) * 100 // a
        elif ss["type"] == "MostAllocated":
            s = min(q, a) * 100 // a
        else:
            shape = ss["requestedToCapacityRatio"]["shape"]
            s = rtc_fn(shape, 100) if q > a else rtc_fn(shape, q * 100 // a)
            if s <= 0:
                continue
        ns += s * r["weight"]
        ws += r["weight"]
    if ws == 0:
        return 0
    if ss["type"] == "RequestedToCapacityRatio":
        return math.floor(ns / ws + 0.5)
    return ns // ws


def ba_score(st, pod, args):
    fr = []
    for r in args["resources"]:
        a, q = alloc_req(st, pod, r["name"], False)
        if a == 0:
            continue
        f = float(q) / float(a)
        fr.append(1.0 if f > 1 else f)
    sd = 0.0
    if len(fr) == 2:
        sd = abs((fr[0] - fr[1]) / 2)
    elif len(fr) > 2:
        total = 0.0
        for f in fr:
            total = total + f
        mean = total / float(len(fr))
        s = 0.0
        for f in fr:
            s = s + (f - mean) * (f - mean)
        sd = math.sqrt(s / float(len(fr)))
    return int((1 - sd) * 100.0)


@functools.lru_cache(maxsize=None)
def first_cycle(kind, violate, profile):
    """(doc, [score-result of every queue pod against the initial snapshot])."""
    doc = edge.gen_magnitude(kind, profile=profile, violate=violate)
    o = Oracle(doc)
    o.whatif(len(doc["queue"]), record=3)
    return doc, [json.loads(o.annotations(q).get(P + "score-result", "{}")) for q in range(len(doc["queue"]))]


@pytest.mark.parametrize("profile", FIT_PROFILES)
@pytest.mark.parametrize("kind,violate", DOCS, ids=IDS)
def test_fit_and_ba_recomputed_from_the_document(kind, violate, profile):
    doc, scored = first_cycle(kind, violate, profile if kind != "norm20" or profile != "default" else None)
    snap = snapshot(doc)
    pc = doc["profile"]["pluginConfig"]
    pairs = 0
    for q, pod in enumerate(doc["queue"]):
        pr = pod_requests(pod)
        for node, row in scored[q].items():
            assert int(row[FIT]) == fit_score(snap[node], pr, pc[FIT]), (q, node, FIT)
            assert int(row[BA]) == ba_score(snap[node], pr, pc[BA]), (q, node, BA)
            pairs += 1
    assert pairs >= len(doc["queue"]) * 2


def triples(kind):
    doc, scored = first_cycle(kind, None, "least4")
    snap = snapshot(doc)
    for q, pod in enumerate(doc["queue"]):
        pr = pod_requests(pod)
        for node in scored[q]:
            for r in doc["profile"]["pluginConfig"][FIT]["scoringStrategy"]["resources"]:
                a, rq = alloc_req(snap[node], pr, r["name"], True)
                if a:
                    yield q, node, r["name"], a, rq


@pytest.mark.parametrize("kind", ["div32", "div52"])
def test_every_div_small_branch_and_quotient_boundary_is_met(kind):
    b32 = mid = slow = edge_ = 0
    for _q, _n, _r, a, rq in triples(kind):
        if rq > a:
            continue
        x = (a - rq) * 100
        if x <= 0xFFFFFFFF and a <= 0xFFFFFFFF:
            b32 += 1
        elif x >= 1 << 52:
            slow += 1
        else:
            mid += 1
        edge_ += a >= 1 << 32 and x % a < 100
    assert min(b32, mid, slow) >= 50, (b32, mid, slow)
    assert edge_ >= 20, edge_


@pytest.mark.parametrize("kind,violate", DOCS, ids=IDS)
def test_most_pods_are_scheduled_among_several_nodes(kind, violate):
    doc = edge.gen_magnitude(kind, violate=violate)
    o = Oracle(doc)
    o.schedule(record=0)
    res = [o.result(q) for q in range(o.n_queue)]
    assert sum(1 for s, f, st in res if st == 0 and f >= 2) * 2 >= len(res), res


def test_zero_over_scores_requests_above_allocatable():
    over = sum(1 for _q, _n, _r, a, rq in triples("zero_over") if rq > a)
    assert over >= 10, over
    doc = edge.gen_magnitude("zero_over")
    al = [n["status"]["allocatable"] for n in doc["nodes"]]
    assert any(a["cpu"] == "0" and a["memory"] != "0" for a in al) and any(a["memory"] == "0" != a["cpu"] for a in al)
    assert any(a["cpu"] == "0" and a["memory"] == "0" for a in al)


def test_wc_gate_documents_differ_by_one_change():
    """The in-gate document has every cpu / memory column at most 2^45 - 1 and every
    request at most 2^44 - 1, with several exactly there; each sibling moves one value."""
    top, ptop = (1 << 45) - 1, (1 << 44) - 1
    base = edge.gen_magnitude("wc_gate")
    snap = snapshot(base)
    cols = [v for st in snap.values() for v in (st["alloc"]["cpu"], st["alloc"]["memory"], st["req"].get("cpu", 0),
                                                 st["req"].get("memory", 0), st["nzc"], st["nzm"])]
    reqs = [v for p in base["queue"] for k, v in pod_requests(p)[0].items()]
    assert max(cols) == top and cols.count(top) >= 6 and max(reqs) == ptop and reqs.count(ptop) >= 6
    for v, where in (("node_alloc", "nodes"), ("pod_req", "queue"), ("node_req", "pods")):
        doc = edge.gen_magnitude("wc_gate", violate=v)
        diff = [k for k in ("nodes", "pods", "queue") if doc[k] != base[k]]
        assert diff == [where], (v, diff)
        if v == "pod_req":
            assert max(x for p in doc["queue"] for x in pod_requests(p)[0].values()) == 1 << 44
        else:
            s = snapshot(doc)
            assert max(max(st["alloc"]["memory"], st["req"].get("memory", 0)) for st in s.values()) == 1 << 45


def test_norm20_normalisers_straddle_two_to_the_twenty():
    """Each pod's largest raw NodeAffinity score over its scored nodes is its target."""
    doc, scored = first_cycle("norm20", None, None)
    seen = set()
    for q, rows in enumerate(scored):
        if rows:
            mx = max(int(r["NodeAffinity"]) for r in rows.values())
            assert mx == edge.NORM20_TARGETS[q % 3], (q, mx)
            assert len({int(r["NodeAffinity"]) for r in rows.values()}) >= 3
            seen.add(mx)
    assert seen == set(edge.NORM20_TARGETS)
