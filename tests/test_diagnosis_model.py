"""The FitError sentence, restated: the model the GPU tests of ksg_fit_error
(tests/test_diagnosis_gpu.py) compare the engine against, pinned here by literal
strings written by hand.  No engine and no GPU.

The rules are those of upstream v1.30.4 framework.FitError.Error() up to, not
including, its PostFilter clause (include/ksg.h, DESIGN.md §Unschedulable
diagnosis):

1. "0/<all nodes of the snapshot> nodes are available:"
2. a PreFilter that rejected the pod: " <its message>." and nothing from the
   nodes; for an empty PreFilterResult intersection the framework's own message,
   "node(s) didn't satisfy plugin(s) [A B] simultaneously", or, with one
   restricting plugin, "node(s) didn't satisfy plugin A"
3. otherwise every failing node's status split into its reasons (", " joins them)
4. each reason counted once per node
5. one entry "<count> <reason>" per reason
6. the entries sorted as byte strings (sort.Strings)
7. joined with ", " and closed with a full stop when there is at least one
8. nodes outside the PreFilterResult have no filter-result row: not counted
9. a scheduled pod, or a cycle that ended in an error, has no sentence
"""
import json
from collections import Counter

from _oracle import Oracle
from ksg import edge

P = "kube-scheduler-simulator.sigs.k8s.io/"
UNSCHEDULABLE = 1


def render(n_nodes, counts=None, prefilter_msg=None):
    """Rules 1, 2 and 5-7 from a {reason: nodes} map or a PreFilter message."""
    s = f"0/{n_nodes} nodes are available:"
    if prefilter_msg is not None:
        return f"{s} {prefilter_msg}."
    entries = sorted(f"{c} {r}".encode() for r, c in (counts or {}).items())
    if entries:
        s += " " + b", ".join(entries).decode() + "."
    return s


def merge_message(with_nodes):
    """RunPreFilterPlugins' status for an empty PreFilterResult intersection."""
    if len(with_nodes) == 1:
        return f"node(s) didn't satisfy plugin {with_nodes[0]}"
    return f"node(s) didn't satisfy plugin(s) [{' '.join(with_nodes)}] simultaneously"


def prefilter_rejection(ann, plugins):
    """The message of the PreFilter status that rejected the pod, or None."""
    pre = json.loads(ann[P + "prefilter-result-status"])
    for name in plugins:
        if pre.get(name) not in (None, "success", ""):
            return pre[name]
    res = json.loads(ann[P + "prefilter-result"])
    with_nodes = [p for p in plugins if p in res]
    if with_nodes:
        common = set(res[with_nodes[0]])
        for p in with_nodes[1:]:
            common &= set(res[p])
        if not common:
            return merge_message(with_nodes)
    return None


def node_reasons(ann):
    """{reason: nodes} over the filter-result rows (rules 3, 4, 8)."""
    counts = Counter()
    for row in json.loads(ann[P + "filter-result"]).values():
        reasons = set()
        for msg in row.values():
            if msg != "passed":
                reasons.update(msg.split(", "))
        counts.update(reasons)
    return counts


def fit_error(ann, status, n_nodes, plugins):
    """The sentence of a pod from its recorded annotations and its cycle's status."""
    if status != UNSCHEDULABLE:
        return ""
    rej = prefilter_rejection(ann, plugins)
    if rej is not None:
        return render(n_nodes, prefilter_msg=rej)
    return render(n_nodes, node_reasons(ann))


def _ann(pre_status=None, pre_result=None, filt=None):
    return {P + "prefilter-result-status": json.dumps(pre_status or {}),
            P + "prefilter-result": json.dumps(pre_result or {}), P + "filter-result": json.dumps(filt or {})}


TAINT = "node(s) had untolerated taint {node-role.kubernetes.io/control-plane: }"
PLUGINS = ["TaintToleration", "NodeAffinity", "NodeResourcesFit", "VolumeBinding"]


def test_upstream_shape():
    filt = {"cp": {"TaintToleration": TAINT},
            "w1": {"TaintToleration": "passed", "NodeAffinity": "passed", "NodeResourcesFit": "Insufficient cpu"},
            "w2": {"TaintToleration": "passed", "NodeAffinity": "passed", "NodeResourcesFit": "Insufficient cpu"}}
    assert fit_error(_ann({"NodeResourcesFit": "success"}, {}, filt), 1, 3, PLUGINS) == (
        "0/3 nodes are available: 1 node(s) had untolerated taint {node-role.kubernetes.io/control-plane: }, "
        "2 Insufficient cpu.")


def test_byte_order_sort_and_split():
    """Counts sort as text ("100" < "12" < "3"), and a node short of two resources
    counts under both reasons."""
    assert render(500, {"Insufficient cpu": 12, "Insufficient memory": 3, "Too many pods": 100}) == (
        "0/500 nodes are available: 100 Too many pods, 12 Insufficient cpu, 3 Insufficient memory.")
    assert render(12, {"x": 10, "y": 2}) == "0/12 nodes are available: 10 x, 2 y."
    assert render(12, {"x": 2, "y": 10}) == "0/12 nodes are available: 10 y, 2 x."
    filt = {f"n{i}": {"NodeResourcesFit": "Insufficient cpu, Insufficient memory"} for i in range(2)}
    filt["n2"] = {"NodeResourcesFit": "Too many pods, Insufficient memory"}
    filt["n3"] = {"NodeResourcesFit": "passed"}
    assert fit_error(_ann(filt=filt), 1, 4, PLUGINS) == (
        "0/4 nodes are available: 1 Too many pods, 2 Insufficient cpu, 3 Insufficient memory.")
    # upper case sorts before lower case at equal counts: bytes, not collation
    assert render(2, {"node(s) were unschedulable": 1, "Too many pods": 1}) == (
        "0/2 nodes are available: 1 Too many pods, 1 node(s) were unschedulable.")


def test_prefilter_rejection_replaces_the_nodes():
    filt = {"n0": {"NodeResourcesFit": "Insufficient cpu"}}
    ann = _ann({"NodeAffinity": "pod affinity terms conflict"}, {}, filt)
    assert fit_error(ann, 1, 7, PLUGINS) == "0/7 nodes are available: pod affinity terms conflict."
    both = _ann({"NodeAffinity": "success", "VolumeBinding": "success"},
                {"NodeAffinity": ["a", "b"], "VolumeBinding": ["c"]})
    assert fit_error(both, 1, 7, PLUGINS) == (
        "0/7 nodes are available: node(s) didn't satisfy plugin(s) [NodeAffinity VolumeBinding] simultaneously.")
    one = _ann({"VolumeBinding": "success"}, {"VolumeBinding": []})
    assert fit_error(one, 1, 7, PLUGINS) == "0/7 nodes are available: node(s) didn't satisfy plugin VolumeBinding."
    # a non-empty intersection restricts, it does not reject: the nodes speak
    meet = _ann({"NodeAffinity": "success", "VolumeBinding": "success"},
                {"NodeAffinity": ["a", "b"], "VolumeBinding": ["b"]}, {"b": {"NodeResourcesFit": "Too many pods"}})
    assert fit_error(meet, 1, 7, PLUGINS) == "0/7 nodes are available: 1 Too many pods."


def test_zero_reasons_and_no_sentence():
    assert fit_error(_ann(), 1, 5, PLUGINS) == "0/5 nodes are available:"
    assert render(0) == "0/0 nodes are available:"
    filt = {"n0": {"NodeResourcesFit": "Insufficient cpu"}}
    assert fit_error(_ann(filt=filt), 0, 5, PLUGINS) == ""  # scheduled
    assert fit_error(_ann(filt=filt), 2, 5, PLUGINS) == ""  # the cycle ended in an error


def test_from_oracle_annotations():
    """One small `na` cluster through the oracle on the CPU: every unschedulable
    pod's sentence is built from its annotations and recounted independently."""
    doc = edge.generate_edge("na", n_nodes=30, n_pods=60)
    plugins = doc["profile"]["plugins"]
    o = Oracle(doc)
    o.schedule(record=3)
    n, seen = len(doc["nodes"]), 0
    for q in range(o.n_queue):
        _, feasible, status = o.result(q)
        ann = o.annotations(q)
        s = fit_error(ann, status, n, plugins)
        if status != UNSCHEDULABLE:
            assert s == ""
            continue
        seen += 1
        assert feasible == 0
        head = f"0/{n} nodes are available:"
        assert s.startswith(head)
        if prefilter_rejection(ann, plugins) is not None:
            continue
        filt = json.loads(ann[P + "filter-result"])
        failing = [row for row in filt.values() if any(v != "passed" for v in row.values())]
        assert len(failing) == len(filt)  # no node passed every filter
        if not failing:
            assert s == head
            continue
        assert s.endswith(".")
        entries = s[len(head) + 1:-1].split(", ")
        # the reasons of this cluster hold no ", " of their own except Fit's joins, so entries
        # parse back: counted nodes >= failing nodes, each entry within the node count
        assert entries == [e.decode() for e in sorted(x.encode() for x in entries)]
        total = 0
        for e in entries:
            c, _, reason = e.partition(" ")
            assert 1 <= int(c) <= len(failing) and reason
            total += int(c)
        assert total >= len(failing)
    assert seen >= 1
