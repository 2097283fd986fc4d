"""CPU: the sparse device door (scs_set_sparse_device / scs_set_test_sparse_device / scs_get_sparse_csc)
as far as it can be checked without a GPU: the header declares the three functions with the agreed
argument lists, the library exports them, the ctypes binding lists them, the Julia module's ccalls
name them with tuples that match the header, the interface parser (a pure function of the three
__cuda_array_interface__ dicts) maps widths, lengths and streams, and the detector tells a device CSR
from a host one.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, LIB
from test_julia_binding import _compatible, _header_protos, _julia_ccalls

NEW = ("scs_set_sparse_device", "scs_set_test_sparse_device", "scs_get_sparse_csc")
SRC = ["const void *", "int", "const void *", "int", "const void *", "int", "int", "const double *", "void *",
       "int64_t", "int64_t"]


def test_header_declares_library_exports_binding_lists():
    protos = _header_protos()
    lib = ctypes.CDLL(LIB)
    from scsopt import _lib
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/scsopt.h"
        assert hasattr(lib, name), f"libscsopt.so does not export {name}"
        assert name in _lib.EXPORTED
        assert getattr(_lib.lib, name).argtypes is not None
    # (ctx, N, m, nnz, d_rowptr, ptr_bytes, d_colidx, idx_bytes, d_val, val_bytes, val_f32, y, src_stream,
    #  N_global, row0)
    assert protos["scs_set_sparse_device"] == ("int", ["scs_ctx *", "int64_t", "int64_t", "int64_t"] + SRC)
    assert protos["scs_set_test_sparse_device"] == ("int", ["scs_ctx *", "int64_t", "int64_t"] + SRC)
    assert protos["scs_get_sparse_csc"] == ("int", ["scs_ctx *", "int64_t *", "int32_t *", "double *"])
    assert len(_lib.lib.scs_set_sparse_device.argtypes) == 15
    assert len(_lib.lib.scs_set_test_sparse_device.argtypes) == 14
    assert len(_lib.lib.scs_get_sparse_csc.argtypes) == 4


def test_header_states_the_contract_and_the_refusals():
    hdr = open(os.path.join(ROOT, "include", "scsopt.h")).read()
    doc = hdr[hdr.index("a sparse A that is already on the device"):hdr.index("int scs_set_sparse_device(")]
    doc = " ".join(doc.replace("*", " ").split())
    for words in ("bit for bit", "duplicates are kept, not summed", "hipPointerGetAttributes", "hipMemGetAddressRange",
                  "first offending row", "first offending position", "multi-device context",
                  "never reads outside the source arrays"):
        assert words in doc, words


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
    assert re.search(r"function DeviceProblem\(rowptr::Ptr\{Cvoid\}, colidx::Ptr\{Cvoid\}, val::Ptr\{Cvoid\}, "
                     r"N::Integer, m::Integer,\s+nnz::Integer", src)
    assert "ptr_type::Type=Int64" in src and "idx_type::Type=Int32" in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "scs_set_sparse_device" in doc and "ROCArray" in doc and "sparse_csr_tensor" in doc


# ---- parse_device_csr ---------------------------------------------------------------------------------
P0 = 0x7F0000001000


def _iface(n, typestr, ptr=P0, strides=None, stream="absent", shape=None):
    d = {"shape": (n,) if shape is None else shape, "typestr": typestr, "data": (ptr, False), "version": 3,
         "strides": strides}
    if stream != "absent":
        d["stream"] = stream
    return d


def _csr(N=5, m=7, nnz=11, pt="<i8", it="<i8", vt="<f8", **kw):
    from scsopt._lib import parse_device_csr
    return parse_device_csr((N, m), _iface(N + 1, pt, P0, **kw), _iface(nnz, it, P0 + 4096, **kw),
                            _iface(nnz, vt, P0 + 8192, **kw))


@pytest.mark.parametrize("pt", ["<i4", "<i8"])
@pytest.mark.parametrize("it", ["<i4", "<i8"])
@pytest.mark.parametrize("vt", ["<f4", "<f8"])
def test_parser_width_pairs(pt, it, vt):
    d = _csr(pt=pt, it=it, vt=vt)
    assert (d["ptr_bytes"], d["idx_bytes"], d["val_bytes"]) == (int(pt[2]), int(it[2]), int(vt[2]))
    assert (d["N"], d["m"], d["nnz"]) == (5, 7, 11)
    assert (d["rowptr"], d["colidx"], d["val"]) == (P0, P0 + 4096, P0 + 8192)
    assert d["stream"] is None


def test_parser_strides_none_against_explicit():
    from scsopt._lib import parse_device_csr as P
    want = _csr(pt="<i4", it="<i4", vt="<f4")
    got = P((5, 7), _iface(6, "<i4", P0, strides=(4,)), _iface(11, "<i4", P0 + 4096, strides=(4,)),
            _iface(11, "<f4", P0 + 8192, strides=(4,)))
    assert got == want
    # an array of one entry addresses nothing with its stride
    d = P((0, 7), _iface(1, "<i8", P0, strides=(64,)), _iface(0, "<i8", 0), _iface(0, "<f8", 0))
    assert (d["N"], d["nnz"]) == (0, 0)


def test_parser_empty_matrix_with_null_data_pointers():
    from scsopt._lib import parse_device_csr as P
    d = P((200, 300), _iface(201, "<i8", P0), _iface(0, "<i8", 0), _iface(0, "<f8", 0))
    assert (d["N"], d["m"], d["nnz"], d["rowptr"], d["colidx"], d["val"]) == (200, 300, 0, P0, 0, 0)
    d = P((200, 300), _iface(201, "<i8", P0), _iface(0, "<i8", None), _iface(0, "<f8", None))
    assert (d["colidx"], d["val"]) == (0, 0)


def test_parser_streams():
    assert _csr(stream=None)["stream"] is None
    assert _csr(stream=1)["stream"] == 1
    assert _csr(stream=2)["stream"] == 2
    assert _csr(stream=0x55AA00)["stream"] == 0x55AA00
    with pytest.raises(ValueError):
        _csr(stream=0)
    # the first array that names a stream decides
    from scsopt._lib import parse_device_csr as P
    d = P((5, 7), _iface(6, "<i8"), _iface(11, "<i8", stream=0x1234), _iface(11, "<f8", stream=2))
    assert d["stream"] == 0x1234


def test_parser_refusals():
    from scsopt._lib import parse_device_csr as P
    with pytest.raises(TypeError, match="<u4"):
        _csr(pt="<u4")
    with pytest.raises(TypeError, match="<i2"):
        _csr(it="<i2")
    with pytest.raises(TypeError, match="<f2"):
        _csr(vt="<f2")
    with pytest.raises(TypeError):
        _csr(vt="<i8")
    with pytest.raises(TypeError):
        _csr(it="<f8")
    with pytest.raises(ValueError, match="contiguous"):               # indices[::2]
        P((5, 7), _iface(6, "<i8"), _iface(11, "<i4", strides=(8,)), _iface(11, "<f8"))
    with pytest.raises(ValueError, match="contiguous"):
        P((5, 7), _iface(6, "<i8"), _iface(11, "<i4"), _iface(11, "<f8", strides=(16,)))
    with pytest.raises(ValueError, match="indptr"):                    # N + 1 entries are needed
        P((5, 7), _iface(5, "<i8"), _iface(11, "<i4"), _iface(11, "<f8"))
    with pytest.raises(ValueError, match="indices"):                   # as many indices as values
        P((5, 7), _iface(6, "<i8"), _iface(10, "<i4"), _iface(11, "<f8"))
    with pytest.raises(ValueError):                                    # a 2-D value array
        P((5, 7), _iface(6, "<i8"), _iface(11, "<i4"), _iface(11, "<f8", shape=(11, 1)))
    with pytest.raises(ValueError, match="two dimensions"):            # a batched CSR's shape
        P((2, 5, 7), _iface(6, "<i8"), _iface(11, "<i4"), _iface(11, "<f8"))


# ---- is_device_csr ------------------------------------------------------------------------------------
class _HostCsr:
    """the attributes of a CuPy csr_matrix, over host arrays"""

    def __init__(self):
        self.indptr, self.indices, self.data = np.zeros(3, np.int32), np.zeros(2, np.int32), np.zeros(2)
        self.shape = (2, 4)


class _DevArray:
    def __init__(self, n, typestr):
        self.__cuda_array_interface__ = _iface(n, typestr)


class _DevCsr(_HostCsr):
    def __init__(self):
        self.indptr, self.indices, self.data = _DevArray(3, "<i4"), _DevArray(2, "<i4"), _DevArray(2, "<f8")
        self.shape = (2, 4)


def test_detector():
    import scipy.sparse as sp
    from scsopt._lib import device_csr_arrays, is_device_csr
    assert not is_device_csr(None)
    assert not is_device_csr(sp.random(6, 4, 0.5, format="csr"))
    assert not is_device_csr(np.zeros((3, 2)))
    assert not is_device_csr(_HostCsr())
    assert is_device_csr(_DevCsr())
    A = _DevCsr()
    assert device_csr_arrays(A) == ((2, 4), A.indptr, A.indices, A.data)


def test_detector_torch_layouts():
    import torch
    from scsopt._lib import is_device_csr
    D = torch.tensor([[1.0, 0.0], [0.0, 2.0]], dtype=torch.float64)
    assert not is_device_csr(D)
    with pytest.raises(ValueError, match=r"to_sparse_csr\(\)"):
        is_device_csr(D.to_sparse())
    with pytest.raises(ValueError, match="CPU sparse torch tensor"):
        is_device_csr(D.to_sparse_csr())
    with pytest.raises(ValueError, match="batched CSR"):
        is_device_csr(torch.stack([D, D]).to_sparse_csr())
