"""CPU-side checks of the headroom boundary (ksg_headroom, ksg_headroom_nodes,
ksg_resource_name): the header declares them with the struct and its bound
count, the built library exports them, the binding offers them, and the ABI
version did not move (pure additions within version 4).  In C the struct is
named by its tag, `struct ksg_headroom`, beside the call of the same name."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")
CALLS = ("ksg_headroom", "ksg_headroom_nodes", "ksg_resource_name")


def test_header_declares_headroom():
    txt = open(HDR).read()
    assert re.search(r"^#define\s+KSG_HEADROOM_BOUNDS\s+9\b", txt, re.M)
    m = re.search(r"^struct\s+ksg_headroom\s*\{(.*?)\};", txt, re.M | re.S)
    assert m
    fields = re.findall(r"^\s*(int64_t|int32_t|uint32_t)\s+(\w+)(\[KSG_HEADROOM_BOUNDS\])?;", m.group(1), re.M)
    assert fields == [("int64_t", "replicas", ""), ("int32_t", "nodes", ""), ("int32_t", "open_nodes", ""),
                      ("int32_t", "max_node", ""), ("int32_t", "best_node", ""),
                      ("uint32_t", "bound", "[KSG_HEADROOM_BOUNDS]")]
    assert re.search(r"^int\s+ksg_headroom\(ksg_ctx\*\s*ctx,\s*uint32_t\s+first,\s*uint32_t\s+count,"
                     r"\s*struct\s+ksg_headroom\*\s*out\);", txt, re.M)
    assert re.search(r"^int\s+ksg_headroom_nodes\(ksg_ctx\*\s*ctx,\s*uint32_t\s+q,\s*int32_t\*\s*out,\s*uint32_t\s+n\);",
                     txt, re.M)
    assert re.search(r"^int\s+ksg_resource_name\(const\s+ksg_ctx\*\s*ctx,\s*uint32_t\s+r,\s*char\*\s*buf,\s*size_t\s+cap,"
                     r"\s*size_t\*\s*len\);", txt, re.M)
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    for name in CALLS + ("KSG_HEADROOM_BOUNDS",):
        assert name in hist, name


def test_library_exports_headroom():
    from ksg import load_library
    L = load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.ksg_abi_version() == 4


def test_binding_offers_headroom():
    from ksg import Scheduler, engine
    sig = inspect.signature(Scheduler.headroom)
    assert list(sig.parameters) == ["self", "first", "count"]
    assert (sig.parameters["first"].default, sig.parameters["count"].default) == (0, None)
    assert list(inspect.signature(Scheduler.headroom_nodes).parameters) == ["self", "q"]
    assert list(inspect.signature(Scheduler.resource_names).parameters) == ["self"]
    assert engine.Headroom._fields == ("replicas", "nodes", "open_nodes", "max_node", "best_node", "bound")
    assert engine.HEADROOM_BOUNDS == 9
    assert ctypes.sizeof(engine._Headroom) == 64 and engine._Headroom.bound.offset == 24


def test_null_context_is_refused():
    """No context, no device: the entry points answer KSG_E_INVALID instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    L.ksg_headroom.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(engine._Headroom)]
    L.ksg_headroom_nodes.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32]
    L.ksg_resource_name.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_size_t)]
    out = (engine._Headroom * 2)()
    row = (ctypes.c_int32 * 4)()
    n = ctypes.c_size_t(7)
    assert L.ksg_headroom(None, 0, 2, out) == -1
    assert L.ksg_headroom_nodes(None, 0, row, 4) == -1
    assert L.ksg_resource_name(None, 0, ctypes.create_string_buffer(8), 8, ctypes.byref(n)) == -1
