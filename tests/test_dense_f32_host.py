"""Host side of the fp32 storage of a dense A (scs_set_dense_f32): the C ABI declares and exports
the entry points, the ctypes binding covers them, and the Python / Julia hosts route a float32
matrix to the fp32 upload instead of widening it.  No GPU needed."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd")
HDR = os.path.join(ROOT, "include", "scsopt.h")
LIB = os.path.join(PKG, "scsopt", "libscsopt.so")
JL = os.path.join(PKG, "julia", "SCSOptAMD.jl")

NEW = ("scs_set_dense_f32", "scs_set_data_f32", "scs_set_test_data_f32", "scs_data_info")


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\bint\s+(scs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entry_points():
    protos = _protos()
    for name in NEW:
        assert name in protos, name
    assert protos["scs_set_dense_f32"] == "scs_ctx* ctx, int on"
    # the fp32 matrix is an untyped pointer (a Julia ccall passes Ptr{Cvoid}), everything else as scs_set_data
    assert protos["scs_set_data_f32"] == protos["scs_set_data"].replace("const double* A,", "const void* A32,")
    assert protos["scs_set_test_data_f32"] == protos["scs_set_test_data"].replace("const double* A,",
                                                                                  "const void* A32,")
    assert protos["scs_data_info"] == "scs_ctx* ctx, int* a_elem_bytes, int64_t* a_bytes, int64_t* ctx_bytes"


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(LIB)
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_holds_the_entry_points():
    from scsopt import _lib
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert getattr(_lib.lib, name).argtypes is not None
    # the matrix of the fp32 uploads is passed untyped, never as a double pointer
    assert _lib.lib.scs_set_data_f32.argtypes[3] is ctypes.c_void_p
    assert _lib.lib.scs_set_test_data_f32.argtypes[2] is ctypes.c_void_p


def test_python_host_surface():
    import scsopt
    assert "dense_f32" in inspect.signature(scsopt.Problem.__init__).parameters
    assert inspect.signature(scsopt.Problem.__init__).parameters["dense_f32"].default is False
    assert "dense_f32" in inspect.signature(scsopt.Problem.synthetic).parameters
    assert callable(scsopt.Problem.data_info)


def test_julia_host_has_the_float32_method():
    src = open(JL).read()
    assert re.search(r"function DeviceProblem\(A::Matrix\{Float32\}, y::AbstractVector, x0::Vector\{Float64\}", src)
    assert ":scs_set_data_f32" in src and ":scs_set_test_data_f32" in src and ":scs_data_info" in src
    assert "Atest isa Matrix{Float32}" in src
