"""CPU-side checks of the ranked-candidates boundary (ksg_ranked_nodes): the
header declares it, the built library exports it, the binding offers it, and the
ABI version did not move (the call is a pure addition within version 4)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "ksg.h")


def test_header_declares_ranked_nodes():
    txt = open(HDR).read()
    assert re.search(r"^#define\s+KSG_RANK_MAX\s+64\s*$", txt, re.M)
    assert re.search(r"typedef\s+struct\s+ksg_ranked_node\s*\{[^}]*int32_t\s+node;[^}]*int32_t\s+total;[^}]*\}\s*ksg_ranked_node;",
                     txt, re.S)
    assert re.search(r"^int\s+ksg_ranked_nodes\(ksg_ctx\*\s*ctx,\s*uint32_t\s+q,\s*uint32_t\s+k,\s*ksg_ranked_node\*\s*out,"
                     r"\s*uint32_t\*\s*n_out\);", txt, re.M)
    assert re.search(r"^#define\s+KSG_ABI_VERSION\s+4\s*$", txt, re.M)
    # the ABI history says the call came within version 4
    hist = txt[txt.index("ABI history"):txt.index("#define KSG_ABI_VERSION")]
    assert "ksg_ranked_nodes" in hist


def test_library_exports_ranked_nodes():
    from ksg import load_library
    L = load_library()
    assert hasattr(L, "ksg_ranked_nodes")
    assert L.ksg_abi_version() == 4


def test_binding_offers_ranked_nodes():
    from ksg import Scheduler
    from ksg import engine
    sig = inspect.signature(Scheduler.ranked_nodes)
    assert list(sig.parameters) == ["self", "q", "k"]
    assert sig.parameters["k"].default == 3
    assert engine.RANK_MAX == 64
    assert ctypes.sizeof(engine._RankedNode) == 8


def test_null_context_is_refused():
    """No context, no device: the entry point answers KSG_E_INVALID instead of touching anything."""
    from ksg import engine
    L = engine.load_library()
    out = (engine._RankedNode * 4)()
    n = ctypes.c_uint32(7)
    assert L.ksg_ranked_nodes(None, 0, 3, out, ctypes.byref(n)) == -1
    assert n.value == 0
