"""CPU-side checks of the set drain's boundary (ksg_drain_sets, ksg_drain_prefixes,
ksg_drain_set_plan): the header declares the calls with their struct, the built
library exports them, the binding mirrors the 32-byte layout, and the ABI version
did not move (pure additions within version 4)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")
CALLS = ("ksg_drain_sets", "ksg_drain_prefixes", "ksg_drain_set_plan")
FIELDS = ["pods", "daemon", "placed", "unplaced", "skipped", "first_unplaced", "first_blocked", "dest_nodes"]


def test_header_declares_the_set_drain():
    txt = open(HDR).read()
    m = re.search(r"^struct\s+ksg_drain_set\s*\{(.*?)\};", txt, re.M | re.S)
    assert m and re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", m.group(1), re.M) == [("int32_t", f) for f in FIELDS]
    for decl in (r"int\s+ksg_drain_sets\(ksg_ctx\*\s*ctx,\s*const\s+uint32_t\*\s*nodes,\s*const\s+uint32_t\*\s*set_start,"
                 r"\s*uint32_t\s+n_sets,\s*struct\s+ksg_drain_set\*\s*out\);",
                 r"int\s+ksg_drain_prefixes\(ksg_ctx\*\s*ctx,\s*const\s+uint32_t\*\s*nodes,\s*uint32_t\s+n,"
                 r"\s*struct\s+ksg_drain_set\*\s*out\);",
                 r"int\s+ksg_drain_set_plan\(ksg_ctx\*\s*ctx,\s*const\s+uint32_t\*\s*nodes,\s*uint32_t\s+n,"
                 r"\s*struct\s+ksg_drain_move\*\s*out,\s*uint32_t\s+cap,\s*uint32_t\*\s*n_out\);"):
        assert re.search("^" + decl, txt, re.M), decl
    assert re.search(r"^#define\s+KSG_DRAIN_SET_NODES\s+128\b", txt, re.M)
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    for name in CALLS + ("ksg_drain_set (the struct)", "KSG_DRAIN_SET_NODES"):
        assert name in hist, name
    # the section stands behind ksg_drain_plan's declaration and before the scale-up's
    at = txt.index("Set drain")
    assert txt.index("int ksg_drain_plan(") < at < txt.index("#define KSG_DRAIN_SET_NODES") < txt.index(
        "Scale-up simulation")
    # what a caller has to know stands in the header
    note = txt[at:txt.index("#define KSG_DRAIN_SET_NODES")].lower()
    for phrase in ("first fit", "not the scheduler's choice", "daemonset", "ksg_drain_max", "mirror pods",
                   "never a destination", "ksg_e_nobuf", "does not sort", "not in the set", "listed twice",
                   "equals ksg_drain of x", "per set", "nodes[0 .. k]", "same bytes", "ksg_e_range", "ksg_e_invalid"):
        assert phrase in note, phrase


def test_struct_size_and_offsets():
    from ksg import engine
    d = engine._DrainSet
    assert ctypes.sizeof(d) == 32
    assert [(n, getattr(d, n).offset, getattr(d, n).size) for n, _ in d._fields_] == [
        (f, 4 * i, 4) for i, f in enumerate(FIELDS)]
    assert all(t is ctypes.c_int32 for _, t in d._fields_)
    assert engine.DrainSet._fields == tuple(FIELDS) and "reserved" not in engine.DrainSet._fields
    assert engine.DrainSet(3, 1, 2, 0, 0, -1, -1, 1).removable
    assert not engine.DrainSet(3, 1, 1, 1, 0, 7, 0, 1).removable
    assert not engine.DrainSet(9, 0, 4, 0, 5, -1, 2, 1).removable
    assert engine.DRAIN_SET_NODES == 128


def test_library_exports_the_set_drain():
    from ksg import load_library
    L = load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.ksg_abi_version() == 4


def test_binding_offers_the_set_drain():
    from ksg import Scheduler
    assert list(inspect.signature(Scheduler.drain_sets).parameters) == ["self", "sets"]
    assert list(inspect.signature(Scheduler.drain_prefixes).parameters) == ["self", "nodes"]
    assert list(inspect.signature(Scheduler.drain_set_plan).parameters) == ["self", "nodes"]


def test_null_context_is_refused():
    """No context, no device: the entry points answer KSG_E_INVALID instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.ksg_drain_sets.argtypes = [ctypes.c_void_p, u32p, u32p, ctypes.c_uint32, ctypes.POINTER(engine._DrainSet)]
    L.ksg_drain_prefixes.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint32, ctypes.POINTER(engine._DrainSet)]
    L.ksg_drain_set_plan.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint32, ctypes.POINTER(engine._DrainMove),
                                     ctypes.c_uint32, u32p]
    nodes, start = (ctypes.c_uint32 * 2)(0, 1), (ctypes.c_uint32 * 2)(0, 2)
    out = (engine._DrainSet * 2)()
    out[0].pods = 77
    n = ctypes.c_uint32(7)
    assert L.ksg_drain_sets(None, nodes, start, 1, out) == -1
    assert L.ksg_drain_sets(None, nodes, start, 0, out) == -1
    assert L.ksg_drain_prefixes(None, nodes, 2, out) == -1
    assert L.ksg_drain_set_plan(None, nodes, 2, (engine._DrainMove * 4)(), 4, ctypes.byref(n)) == -1 and n.value == 0
    assert out[0].pods == 77
