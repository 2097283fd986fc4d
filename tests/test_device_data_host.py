"""CPU: the device-array door (scs_set_data_device / scs_set_test_data_device) as far as it can be
checked without a GPU: the header declares both functions, the library exports them, the ctypes
binding lists them, the Julia module's ccalls name them with tuples that match the header, and the
__cuda_array_interface__ parser (a pure function of the interface dict) maps layouts to strides.
"""
import ctypes
import os
import re

import pytest

from conftest import ROOT, LIB
from test_julia_binding import _compatible, _header_protos, _julia_ccalls

NEW = ("scs_set_data_device", "scs_set_test_data_device")


def test_header_declares_library_exports_binding_lists():
    protos = _header_protos()
    lib = ctypes.CDLL(LIB)
    from scsopt import _lib
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/scsopt.h"
        assert hasattr(lib, name), f"libscsopt.so does not export {name}"
        assert name in _lib.EXPORTED
        assert getattr(_lib.lib, name).argtypes is not None
    # (ctx, N, m, dA, elem_bytes, stride_n, stride_m, y, src_stream, N_global, row0)
    assert protos["scs_set_data_device"][1] == ["scs_ctx *", "int64_t", "int64_t", "const void *", "int", "int64_t",
                                                "int64_t", "const double *", "void *", "int64_t", "int64_t"]
    assert protos["scs_set_test_data_device"][1] == ["scs_ctx *", "int64_t", "const void *", "int", "int64_t",
                                                     "int64_t", "const double *", "void *", "int64_t", "int64_t"]
    from scsopt import _lib as L
    assert len(L.lib.scs_set_data_device.argtypes) == 11
    assert len(L.lib.scs_set_test_data_device.argtypes) == 10


def test_header_states_the_memory_peak_and_the_refusals():
    hdr = open(os.path.join(ROOT, "include", "scsopt.h")).read()
    doc = hdr[hdr.index("a dense A that is already on the device"):hdr.index("int scs_set_data_device(")]
    doc = " ".join(doc.replace("*", " ").split())
    assert "Peak device memory is the source plus the tiled block" in doc
    assert "hipPointerGetAttributes" in doc and "multi-device context" in doc


def test_julia_ccalls_match_the_header():
    protos = _header_protos()
    seen = {}
    for name, ret, args in _julia_ccalls():
        if name in NEW:
            cret, ctypes_ = protos[name]
            assert ret == "Cint" and cret == "int"
            assert len(args) == len(ctypes_), (name, args, ctypes_)
            for a, ct in zip(args, ctypes_):
                assert _compatible(a, ct), (name, a, ct)
            seen[name] = args
    assert set(seen) == set(NEW)
    src = open(os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd", "julia", "SCSOptAMD.jl")).read()
    assert re.search(r"function DeviceProblem\(ptr::Ptr\{Cvoid\}, N::Integer, m::Integer", src)
    assert "elem::Type=Float64" in src and "strides::Tuple{Integer,Integer}" in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ROCArray" in doc and "DeviceProblem(" in doc and "strides" in doc


def _iface(shape, typestr="<f8", strides=None, ptr=0x7F0000001000, stream="absent"):
    d = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}
    if stream != "absent":
        d["stream"] = stream
    return d


def test_parser_layouts():
    from scsopt._lib import parse_device_matrix as P
    # C order, strides given and strides = None
    for st in ((300 * 8, 8), None):
        d = P(_iface((1000, 300), "<f8", st))
        assert (d["N"], d["m"], d["elem_bytes"], d["stride_n"], d["stride_m"]) == (1000, 300, 8, 300, 1)
        assert d["ptr"] == 0x7F0000001000 and d["stream"] is None
    # F order
    d = P(_iface((1000, 300), "<f8", (8, 1000 * 8)))
    assert (d["stride_n"], d["stride_m"]) == (1, 1000)
    # a column slice T[:, 3:3+m] of a wider row-major fp32 tensor: padded leading stride, offset start
    d = P(_iface((17, 129), "<f4", (140 * 4, 4), ptr=0x7F0000001000 + 3 * 4))
    assert (d["elem_bytes"], d["stride_n"], d["stride_m"], d["ptr"] % 16) == (4, 140, 1, 12)
    # its transpose analogue
    d = P(_iface((17, 129), "<f4", (4, 40 * 4)))
    assert (d["stride_n"], d["stride_m"]) == (1, 40)
    # an extent-1 axis addresses nothing, whatever its stride says
    d = P(_iface((1, 300), "<f8", (8, 8)))
    assert (d["stride_n"], d["stride_m"]) == (300, 1)
    d = P(_iface((300, 1), "<f8", (8, 8)))
    assert (d["stride_n"], d["stride_m"]) == (1, 300)
    d = P(_iface((1, 300), "<f8", (8, 16 * 8)))
    assert (d["stride_n"], d["stride_m"]) == (1, 16)


def test_parser_types_and_refusals():
    from scsopt._lib import parse_device_matrix as P
    assert P(_iface((4, 2), "<f4"))["elem_bytes"] == 4
    assert P(_iface((4, 2), "<f8"))["elem_bytes"] == 8
    with pytest.raises(TypeError, match="<f2"):
        P(_iface((4, 2), "<f2"))
    with pytest.raises(TypeError):
        P(_iface((4, 2), "<i8"))
    with pytest.raises(ValueError, match="contiguous"):          # T[::2, ::2]
        P(_iface((4, 2), "<f8", (4 * 8 * 2, 16)))
    with pytest.raises(ValueError):
        P(_iface((4, 2, 2), "<f8"))
    with pytest.raises(ValueError, match="overlaps"):            # an expanded row: stride_n < m
        P(_iface((4, 8), "<f8", (8, 8)))


def test_parser_streams():
    from scsopt._lib import parse_device_matrix as P
    assert P(_iface((4, 2)))["stream"] is None
    assert P(_iface((4, 2), stream=None))["stream"] is None
    # 1: the legacy default stream, 2: the per-thread default stream: they pass through as src_stream,
    # and the library resolves them (include/scsopt.h)
    assert P(_iface((4, 2), stream=1))["stream"] == 1
    assert P(_iface((4, 2), stream=2))["stream"] == 2
    assert P(_iface((4, 2), stream=0x55AA00))["stream"] == 0x55AA00
    with pytest.raises(ValueError):
        P(_iface((4, 2), stream=0))


def test_parser_device_y():
    from scsopt._lib import parse_device_vector as V
    assert V({"shape": (5,), "typestr": "<f8", "data": (4096, False), "strides": None}, 5) == 4096
    with pytest.raises(TypeError):
        V({"shape": (5,), "typestr": "<f4", "data": (4096, False), "strides": None}, 5)
    with pytest.raises(ValueError):
        V({"shape": (4,), "typestr": "<f8", "data": (4096, False), "strides": None}, 5)
    with pytest.raises(ValueError):
        V({"shape": (5,), "typestr": "<f8", "data": (4096, False), "strides": (16,)}, 5)
