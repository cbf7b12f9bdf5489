"""CPU-side checks of the eviction-fit boundary (ksg_bound_count, ksg_bound_pod,
ksg_bound_fit, ksg_bound_fit_nodes, ksg_node_evictability): the header declares
them with their two 16-byte structs, the built library exports them, the binding
mirrors the layouts, and the ABI version did not move (pure additions within
version 4).  In C the struct is named by its tag, `struct ksg_bound_fit`, beside
the call of the same name."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")
CALLS = ("ksg_bound_count", "ksg_bound_pod", "ksg_bound_fit", "ksg_bound_fit_nodes", "ksg_node_evictability")


def fields_of(txt, tag):
    m = re.search(r"^struct\s+%s\s*\{(.*?)\};" % tag, txt, re.M | re.S)
    assert m, tag
    return re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", m.group(1), re.M)


def test_header_declares_bound_fit():
    txt = open(HDR).read()
    assert fields_of(txt, "ksg_bound_fit") == [("int32_t", "node"), ("uint32_t", "own_code"), ("int32_t", "other_nodes"),
                                               ("int32_t", "first_other")]
    assert fields_of(txt, "ksg_node_evict") == [("int32_t", "pods"), ("int32_t", "stuck"), ("int32_t", "drifted"),
                                                ("int32_t", "reserved")]
    for decl in (r"int\s+ksg_bound_count\(const\s+ksg_ctx\*\s*ctx\);",
                 r"int\s+ksg_bound_pod\(ksg_ctx\*\s*ctx,\s*uint32_t\s+b,\s*char\*\s*buf,\s*size_t\s+cap,\s*size_t\*\s*len,"
                 r"\s*int32_t\*\s*node\);",
                 r"int\s+ksg_bound_fit\(ksg_ctx\*\s*ctx,\s*uint32_t\s+first,\s*uint32_t\s+count,"
                 r"\s*struct\s+ksg_bound_fit\*\s*out\);",
                 r"int\s+ksg_bound_fit_nodes\(ksg_ctx\*\s*ctx,\s*uint32_t\s+b,\s*uint32_t\*\s*codes,\s*uint32_t\s+n\);",
                 r"int\s+ksg_node_evictability\(ksg_ctx\*\s*ctx,\s*struct\s+ksg_node_evict\*\s*out,\s*uint32_t\s+n\);"):
        assert re.search("^" + decl, txt, re.M), decl
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    for name in CALLS + ("ksg_node_evict",):
        assert name in hist, name
    # what a caller has to know stands in the header
    note = txt[txt.index("Eviction fit"):txt.index("int ksg_bound_count")]
    for phrase in ("necessary", "not subjects", "ksg_compact(ksg_queue_len())", "NodeName's Filter is not applied"):
        assert phrase in note, phrase


def test_struct_sizes_and_offsets():
    from ksg import engine
    bf, ne = engine._BoundFit, engine._NodeEvict
    assert ctypes.sizeof(bf) == 16 and ctypes.sizeof(ne) == 16
    assert [(n, getattr(bf, n).offset, getattr(bf, n).size) for n, _ in bf._fields_] == [
        ("node", 0, 4), ("own_code", 4, 4), ("other_nodes", 8, 4), ("first_other", 12, 4)]
    assert [(n, getattr(ne, n).offset, getattr(ne, n).size) for n, _ in ne._fields_] == [
        ("pods", 0, 4), ("stuck", 4, 4), ("drifted", 8, 4), ("reserved", 12, 4)]
    assert dict(bf._fields_)["own_code"] is ctypes.c_uint32 and dict(bf._fields_)["first_other"] is ctypes.c_int32
    assert engine.BoundFit._fields == ("node", "own_code", "other_nodes", "first_other")
    assert engine.NodeEvict._fields == ("pods", "stuck", "drifted")


def test_library_exports_bound_fit():
    from ksg import load_library
    L = load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.ksg_abi_version() == 4


def test_binding_offers_bound_fit():
    from ksg import Scheduler
    sig = inspect.signature(Scheduler.bound_fit)
    assert list(sig.parameters) == ["self", "first", "count"]
    assert (sig.parameters["first"].default, sig.parameters["count"].default) == (0, None)
    assert list(inspect.signature(Scheduler.bound_fit_nodes).parameters) == ["self", "b"]
    assert list(inspect.signature(Scheduler.bound_pods).parameters) == ["self"]
    assert list(inspect.signature(Scheduler.node_evictability).parameters) == ["self"]


def test_null_context_is_refused():
    """No context, no device: the entry points answer KSG_E_INVALID (the count: 0) instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    L.ksg_bound_count.argtypes = [ctypes.c_void_p]
    L.ksg_bound_pod.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
    L.ksg_bound_fit.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(engine._BoundFit)]
    L.ksg_bound_fit_nodes.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    L.ksg_node_evictability.argtypes = [ctypes.c_void_p, ctypes.POINTER(engine._NodeEvict), ctypes.c_uint32]
    n, node = ctypes.c_size_t(7), ctypes.c_int32()
    assert L.ksg_bound_count(None) == 0
    assert L.ksg_bound_pod(None, 0, ctypes.create_string_buffer(8), 8, ctypes.byref(n), ctypes.byref(node)) == -1
    assert L.ksg_bound_fit(None, 0, 2, (engine._BoundFit * 2)()) == -1
    assert L.ksg_bound_fit_nodes(None, 0, (ctypes.c_uint32 * 4)(), 4) == -1
    assert L.ksg_node_evictability(None, (engine._NodeEvict * 4)(), 4) == -1
