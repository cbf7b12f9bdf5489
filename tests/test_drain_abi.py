"""CPU-side checks of the drain simulation's boundary (ksg_drain, ksg_drain_plan):
the header declares the calls with their two structs, the built library exports
them, the binding mirrors the layouts (32 and 8 bytes), and the ABI version did
not move (pure additions within version 4)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")
CALLS = ("ksg_drain", "ksg_drain_plan")
FIELDS = ["pods", "daemon", "placed", "unplaced", "skipped", "first_unplaced", "dest_nodes", "reserved"]


def test_header_declares_drain():
    txt = open(HDR).read()
    m = re.search(r"^struct\s+ksg_drain\s*\{(.*?)\};", txt, re.M | re.S)
    assert m and re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", m.group(1), re.M) == [("int32_t", f) for f in FIELDS]
    assert re.search(r"^struct\s+ksg_drain_move\s*\{\s*int32_t\s+bound;\s*int32_t\s+dest;\s*\};", txt, re.M)
    for decl in (r"int\s+ksg_drain\(ksg_ctx\*\s*ctx,\s*uint32_t\s+first_node,\s*uint32_t\s+count,"
                 r"\s*struct\s+ksg_drain\*\s*out\);",
                 r"int\s+ksg_drain_plan\(ksg_ctx\*\s*ctx,\s*uint32_t\s+node,\s*struct\s+ksg_drain_move\*\s*out,"
                 r"\s*uint32_t\s+cap,\s*uint32_t\*\s*n_out\);"):
        assert re.search("^" + decl, txt, re.M), decl
    assert re.search(r"^#define\s+KSG_DRAIN_MAX\s+512\s*$", txt, re.M)
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    for name in CALLS + ("ksg_drain_move", "KSG_DRAIN_MAX", "the call and the struct"):
        assert name in hist, name
    # what a caller has to know stands in the header
    note = txt[txt.index("Drain simulation"):txt.index("#define KSG_DRAIN_MAX")]
    for phrase in ("first fit", "not the scheduler's choice", "daemonset", "ksg_drain_max", "mirror pods",
                   "never a destination", "ksg_e_nobuf"):
        assert phrase in note.lower(), phrase


def test_struct_sizes_and_offsets():
    from ksg import engine
    d, mv = engine._Drain, engine._DrainMove
    assert ctypes.sizeof(d) == 32 and ctypes.sizeof(mv) == 8
    assert [(n, getattr(d, n).offset, getattr(d, n).size) for n, _ in d._fields_] == [
        (f, 4 * i, 4) for i, f in enumerate(FIELDS)]
    assert [(n, getattr(mv, n).offset, getattr(mv, n).size) for n, _ in mv._fields_] == [("bound", 0, 4), ("dest", 4, 4)]
    assert all(t is ctypes.c_int32 for _, t in d._fields_ + mv._fields_)
    assert engine.Drain._fields == tuple(FIELDS[:-1])  # (reserved is dropped)
    assert engine.Drain(3, 1, 2, 0, 0, -1, 1).drainable
    assert not engine.Drain(3, 1, 1, 1, 0, 7, 1).drainable and not engine.Drain(9, 0, 4, 0, 5, -1, 1).drainable
    assert engine.DRAIN_MAX == 512


def test_library_exports_drain():
    from ksg import load_library
    L = load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.ksg_abi_version() == 4


def test_binding_offers_drain():
    from ksg import Scheduler
    sig = inspect.signature(Scheduler.drain)
    assert list(sig.parameters) == ["self", "first", "count"]
    assert (sig.parameters["first"].default, sig.parameters["count"].default) == (0, None)
    assert list(inspect.signature(Scheduler.drain_plan).parameters) == ["self", "node"]


def test_null_context_is_refused():
    """No context, no device: the entry points answer KSG_E_INVALID instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    L.ksg_drain.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(engine._Drain)]
    L.ksg_drain_plan.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(engine._DrainMove), ctypes.c_uint32,
                                 ctypes.POINTER(ctypes.c_uint32)]
    n = ctypes.c_uint32(7)
    assert L.ksg_drain(None, 0, 2, (engine._Drain * 2)()) == -1
    assert L.ksg_drain_plan(None, 0, (engine._DrainMove * 4)(), 4, ctypes.byref(n)) == -1 and n.value == 0
