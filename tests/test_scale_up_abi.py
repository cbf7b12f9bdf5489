"""CPU-side checks of the scale-up simulation's boundary (ksg_scale_up,
ksg_scale_up_plan): the header declares the calls with their struct and the
constant, the built library exports them, the binding mirrors the layout (32
bytes), and the ABI version did not move (pure additions within version 4)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")
CALLS = ("ksg_scale_up", "ksg_scale_up_plan")
FIELDS = ["nodes", "packed", "closed", "too_big", "over_cap", "first_unpacked", "base_pods", "reserved"]


def test_header_declares_scale_up():
    txt = open(HDR).read()
    m = re.search(r"^struct\s+ksg_scale_up\s*\{(.*?)\};", txt, re.M | re.S)
    assert m and re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", m.group(1), re.M) == [("int32_t", f) for f in FIELDS]
    for decl in (r"int\s+ksg_scale_up\(ksg_ctx\*\s*ctx,\s*const\s+uint32_t\*\s*pods,\s*uint32_t\s+n_pods,"
                 r"\s*const\s+uint32_t\*\s*templates,\s*uint32_t\s+n_templates,\s*uint32_t\s+max_nodes,"
                 r"\s*struct\s+ksg_scale_up\*\s*out\);",
                 r"int\s+ksg_scale_up_plan\(ksg_ctx\*\s*ctx,\s*const\s+uint32_t\*\s*pods,\s*uint32_t\s+n_pods,"
                 r"\s*uint32_t\s+template_node,\s*uint32_t\s+max_nodes,\s*int32_t\*\s*bin_out[^)]*\);"):
        assert re.search("^" + decl, txt, re.M), decl
    assert re.search(r"^#define\s+KSG_SCALE_MAX\s+1024\s*$", txt, re.M)
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    for name in CALLS + ("KSG_SCALE_MAX",):
        assert name in hist, name
    # what a caller has to know stands in the header
    note = txt[txt.index("Scale-up simulation"):txt.index("#define KSG_SCALE_MAX")].lower()
    note = " ".join(re.sub(r"^\s*\*", " ", note, flags=re.M).split())  # (the comment's line breaks and leaders)
    for phrase in ("first fit", "does not sort", "packed twice", "daemonset", "mirror pods", "requested(t) does not count",
                   "prefilterresult", "spec.nodename", "kubernetes.io/hostname", "limitation", "too_big", "over_cap",
                   "ksg_scale_max", "zero-request pod", "the same bytes", "-1 closed", "ksg_e_range", "ksg_e_invalid"):
        assert phrase in note, phrase


def test_struct_size_and_offsets():
    from ksg import engine
    s = engine._ScaleUp
    assert ctypes.sizeof(s) == 32
    assert [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_] == [
        (f, 4 * i, 4) for i, f in enumerate(FIELDS)]
    assert all(t is ctypes.c_int32 for _, t in s._fields_)
    assert engine.ScaleUp._fields == tuple(FIELDS[:-1])  # (reserved is dropped)
    assert engine.ScaleUp(2, 5, 0, 0, 0, -1, 1).satisfied
    assert not engine.ScaleUp(2, 4, 1, 0, 0, 3, 0).satisfied and not engine.ScaleUp(2, 4, 0, 1, 0, 3, 0).satisfied
    assert not engine.ScaleUp(2, 4, 0, 0, 1, 4, 0).satisfied
    assert engine.SCALE_MAX == 1024


def test_library_exports_scale_up():
    from ksg import load_library
    L = load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.ksg_abi_version() == 4


def test_binding_offers_scale_up():
    from ksg import Scheduler
    sig = inspect.signature(Scheduler.scale_up)
    assert list(sig.parameters) == ["self", "pods", "templates", "max_nodes"]
    assert sig.parameters["max_nodes"].default == 1024
    assert list(inspect.signature(Scheduler.scale_up_plan).parameters) == ["self", "pods", "template", "max_nodes"]


def test_null_context_is_refused():
    """No context, no device: the entry points answer KSG_E_INVALID instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.ksg_scale_up.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, ctypes.c_uint32,
                               ctypes.POINTER(engine._ScaleUp)]
    L.ksg_scale_up_plan.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.POINTER(ctypes.c_int32)]
    pods, tmpl = (ctypes.c_uint32 * 2)(0, 1), (ctypes.c_uint32 * 1)(0)
    out, bins = (engine._ScaleUp * 1)(), (ctypes.c_int32 * 2)(7, 7)
    out[0].nodes = 77
    assert L.ksg_scale_up(None, pods, 2, tmpl, 1, 4, out) == -1 and out[0].nodes == 77
    assert L.ksg_scale_up_plan(None, pods, 2, 0, 4, bins) == -1 and list(bins) == [7, 7]
