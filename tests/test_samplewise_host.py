"""CPU: the sample-wise loss (losses.samplewise / scs_set_loss_samplewise) without a device: the
constructor's validation, the holder that lends the library's device buffers to torch, and the
header / Python binding / Julia binding of the new entry point, through the helpers of the
existing ABI tests."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_abi
import test_julia_binding as tjb
from conftest import ROOT, LIB

NEW = "scs_set_loss_samplewise"


def test_constructor_validation():
    from scsopt import losses
    v = lambda z, y: z  # noqa: E731
    f = losses.samplewise(v)
    assert (f.kind, f.scale, f.device, f.has_ggn) == ("samplewise", 1.0, False, False)
    assert f.value is v and f.d1 is None and f.d2 is None
    assert isinstance(f, losses.Loss)
    g = losses.samplewise(v, v, v, link=v, link_d1=v, grad_fy=v, hess_fy=v, device=True)
    assert g.has_ggn and g.device and g.d2 is v
    with pytest.raises(TypeError):
        losses.samplewise(None)
    with pytest.raises(TypeError):
        losses.samplewise(v, d1=3.0)
    for part in ({"link": v}, {"link": v, "link_d1": v, "grad_fy": v}, {"hess_fy": v}):
        with pytest.raises(ValueError, match="go together"):
            losses.samplewise(v, **part)
    with pytest.raises(TypeError):   # the GGN pieces and the mode are keywords
        losses.samplewise(v, v, v, v)


def test_binding_constants_match_the_header():
    from scsopt import _lib
    assert _lib.LOSS["samplewise"] == 7 and _lib.GGN["samplewise"] == 3
    assert (_lib.SCS_SW_VALUE, _lib.SCS_SW_D1, _lib.SCS_SW_D2, _lib.SCS_SW_GGN) == (1, 2, 4, 8)


def test_device_vector_interface():
    from scsopt import _lib
    h = _lib.DeviceVector(0x7F0000001000, 513)
    d = h.__cuda_array_interface__
    assert d["shape"] == (513,) and d["typestr"] == "<f8" and d["version"] == 2
    assert d["data"] == (0x7F0000001000, False)
    assert d.get("strides") is None and "stream" not in d
    assert _lib.is_device_array(h)
    assert _lib.parse_device_vector(d, 513) == 0x7F0000001000
    with pytest.raises(ValueError):
        _lib.parse_device_vector(d, 512)


def test_header_declares_kinds_bits_and_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "scsopt.h")).read()
    assert re.search(r"SCS_LOSS_SAMPLEWISE = 7\b", hdr) and re.search(r"SCS_GGN_SAMPLEWISE = 3\b", hdr)
    for name, bit in (("VALUE", 1), ("D1", 2), ("D2", 4), ("GGN", 8)):
        assert re.search(rf"#define SCS_SW_{name} {bit}\b", hdr), name
    assert NEW in test_abi.header_functions()
    assert "scs_samplewise_fn" not in test_abi.header_functions()      # a type, not an export
    ret, types = tjb._header_protos()[NEW]
    assert ret == "int"
    assert types == ["scs_ctx *", "scs_samplewise_fn *", "void *", "int", "int"]


def test_library_exports_and_binding_signature():
    from scsopt import _lib
    assert hasattr(ctypes.CDLL(LIB), NEW)
    assert NEW in _lib.EXPORTED
    fn = getattr(_lib.lib, NEW)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, _lib.SAMPLEWISE_FN, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    # (user, what, n, z, y, val, d1, d2, s, stream) -> int
    assert _lib.SAMPLEWISE_FN._restype_ is ctypes.c_int
    assert _lib.SAMPLEWISE_FN._argtypes_ == (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64) + (ctypes.c_void_p,) * 7
    test_abi.test_binding_covers_header()


def test_julia_binding_calls_the_entry_point():
    calls = [c for c in tjb._julia_ccalls() if c[0] == NEW]
    assert len(calls) == 1
    _, ret, args = calls[0]
    cret, ctypes_ = tjb._header_protos()[NEW]
    assert ret == "Cint" and cret == "int" and len(args) == len(ctypes_) == 5
    for a, ct in zip(args, ctypes_):
        assert tjb._compatible(a, ct), (a, ct)
    src = open(tjb.JL).read()
    assert re.search(r"^mutable struct Samplewise\b", src, flags=re.M)      # pointer_from_objref needs it
    assert "pointer_from_objref(sw)" in src
    tr = src[src.index("function samplewise_trampoline("):]
    tr = tr[:tr.index("\nend\n")]
    # the trampoline's @cfunction signature is the typedef's: 10 parameters, the pointers as Ptr
    m = re.search(r"@cfunction\(samplewise_trampoline, Cint, \((.*?)\)\)", src, flags=re.S)
    assert m and [t.strip() for t in m.group(1).split(",")] == \
        ["Ptr{Cvoid}", "Cint", "Int64"] + ["Ptr{Float64}"] * 6 + ["Ptr{Cvoid}"]
    assert "unsafe_wrap(Array, zp, n)" in tr and "sw.value(vp, zp, yp, n, stream)" in tr
    assert "CB_EXCEPTION[] = err" in tr
    tjb.test_every_ccall_matches_the_header()
    tjb.test_integration_doc_matches_module()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"ccall((:{NEW}, lib)" in doc


def test_wrong_length_and_scalar_results_in_host_mode():
    """The host-mode copy into the library's output area: a length mismatch raises, a scalar is
    broadcast (the same rule the device mode applies through copy_)."""
    from scsopt.problems import _samplewise_put_host as put
    dst = np.zeros(5)
    put(dst, 2.0 ** -8, "d2")
    assert np.all(dst == 2.0 ** -8)
    put(dst, [1, 2, 3, 4, 5], "d1")
    assert dst.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    for bad in (np.zeros(4), np.zeros(6), np.zeros((5, 1)), np.zeros(1)):
        with pytest.raises(ValueError, match="d1 returned shape"):
            put(dst, bad, "d1")
    assert dst.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
