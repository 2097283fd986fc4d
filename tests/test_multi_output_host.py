"""Host side of the multi-output losses (scs_set_outputs; no GPU): constructor validation, the
binding's constants and signatures against include/scsopt.h, the Julia ccalls, and the NumPy helper
the GPU tests compare against (its block-formula Hessian equals JᵀQJ of its dense pieces)."""
import ctypes
import os
import re

import numpy as np
import pytest

import multi_output_data as M
import test_abi
import test_julia_binding as tjb
from conftest import ROOT, LIB

NEW = ("scs_set_outputs", "scs_get_outputs", "scs_multi_products_eval", "scs_multi_system_eval")


def test_constructor_validation():
    from scsopt import losses
    f = losses.softmax_ce(3, 0.5)
    assert (f.kind, f.nout, f.scale) == ("softmax_ce", 3, 0.5)
    g = losses.multi_least_squares(16)
    assert (g.kind, g.nout, g.scale) == ("multi_least_squares", 16, 1.0)
    assert losses.linear_softmax_ce(3, 0.5).kind == "linear_softmax_ce" and losses.linear_softmax_ce(3).nout == 3
    assert losses.linear_multi_ls(2).kind == "linear_multi_ls"
    assert losses.ggn_kind(losses.linear_multi_ls(2)) == "linear_multi_ls"
    for make in (losses.softmax_ce, losses.multi_least_squares, losses.linear_softmax_ce, losses.linear_multi_ls):
        for bad in (0, 1, 17, -3, 2.5):
            with pytest.raises(ValueError, match="nout"):
                make(bad)
    assert "nout=3" in repr(f)
    # the single-output kinds carry no nout
    assert not hasattr(losses.least_squares(), "nout") and not hasattr(losses.linear_ls(), "nout")


def test_binding_constants_match_the_header():
    from scsopt import _lib
    hdr = open(os.path.join(ROOT, "include", "scsopt.h")).read()
    for name, key, table in (("SCS_LOSS_SOFTMAX_CE", "softmax_ce", _lib.LOSS),
                             ("SCS_LOSS_MULTI_LS", "multi_least_squares", _lib.LOSS),
                             ("SCS_GGN_LINEAR_SOFTMAX_CE", "linear_softmax_ce", _lib.GGN),
                             ("SCS_GGN_LINEAR_MULTI_LS", "linear_multi_ls", _lib.GGN)):
        m = re.search(rf"\b{name} = (\d+)\b", hdr)
        assert m and int(m.group(1)) == table[key], name
    assert (_lib.LOSS["softmax_ce"], _lib.LOSS["multi_least_squares"]) == (8, 9)
    assert (_lib.GGN["linear_softmax_ce"], _lib.GGN["linear_multi_ls"]) == (4, 5)


def test_header_declares_the_entry_points():
    protos = tjb._header_protos()
    for name in NEW:
        assert name in test_abi.header_functions()
        assert protos[name][0] == "int"
    assert protos["scs_set_outputs"][1] == ["scs_ctx *", "int"]
    assert protos["scs_get_outputs"][1] == ["scs_ctx *", "int *", "int64_t *"]
    assert protos["scs_multi_products_eval"][1] == ["scs_ctx *", "int", "const double *", "const double *", "double *",
                                                    "double *"]
    assert protos["scs_multi_system_eval"][1] == ["scs_ctx *", "const double *", "double *", "int64_t", "double *",
                                                  "double *"]


def test_library_exports_and_binding_signatures():
    from scsopt import _lib
    so = ctypes.CDLL(LIB)
    for name in NEW:
        assert hasattr(so, name) and name in _lib.EXPORTED
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    assert _lib.lib.scs_set_outputs.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert _lib.lib.scs_multi_products_eval.argtypes == [ctypes.c_void_p, ctypes.c_int] + [_lib.c_dp] * 4
    test_abi.test_binding_covers_header()


def test_julia_binding_calls_the_entry_points():
    calls = {c[0]: c for c in tjb._julia_ccalls()}
    protos = tjb._header_protos()
    for name in NEW:
        assert name in calls, name
        _, ret, args = calls[name]
        cret, ctypes_ = protos[name]
        assert ret == "Cint" and cret == "int" and len(args) == len(ctypes_)
        for a, ct in zip(args, ctypes_):
            assert tjb._compatible(a, ct), (name, a, ct)
    src = open(tjb.JL).read()
    assert ":softmax_ce => 8" in src and ":multi_least_squares => 9" in src
    assert ":linear_softmax_ce => 4" in src and ":linear_multi_ls => 5" in src
    # the multi-output method: scs_set_outputs before the data door, whose m is A's column count
    body = src[src.index("Y::AbstractMatrix, x0::Vector{Float64}"):]
    body = body[:body.index("\nend\n")]
    assert body.index("scs_set_outputs") < body.index("scs_set_data")
    assert "ctx, N, d, A, N, Ym, N, 0" in body
    tjb.test_every_ccall_matches_the_header()
    tjb.test_integration_doc_matches_module()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ccall((:scs_set_outputs, lib)" in doc


def test_device_targets_interface():
    """parse_device_targets: an N x K float64 device array, column-major with leading dimension N."""
    from scsopt import _lib
    ok = {"shape": (5, 3), "typestr": "<f8", "data": (0x7F0000001000, False), "strides": (8, 40), "version": 2}
    assert _lib.parse_device_targets(ok, 5, 3) == 0x7F0000001000
    with pytest.raises(ValueError, match="column-major"):
        _lib.parse_device_targets(dict(ok, strides=None), 5, 3)           # C-contiguous: row-major
    with pytest.raises(ValueError, match="shape"):
        _lib.parse_device_targets(ok, 5, 4)
    with pytest.raises(TypeError, match="float64"):
        _lib.parse_device_targets(dict(ok, typestr="<f4"), 5, 3)


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("soft", [False, True])
def test_helper_block_formula_equals_dense_ggn(kind, soft):
    """Pins the helper: its block-formula Hessian equals Jᵀ Q J from its dense jac_yx / hess_fy, its
    gradient equals Jᵀ grad_fy and a central difference of f, at (N, d, K) = (40, 9, 3)."""
    N, d, K = 40, 9, 3
    A, Y, x0 = M.problem(N, d, K, soft=soft)
    assert np.all(x0 != 0.0)
    if soft:
        assert np.all(np.abs(Y.sum(axis=1) - 1.0) > 1e-3)
    else:
        assert np.array_equal(Y.sum(axis=1), np.ones(N)) and set(np.unique(Y)) == {0.0, 1.0}
    c = 1.0 / N
    cl = M.closures(kind, d, K, c)
    Z = cl["out_fn"](A, x0)
    J = cl["jac_yx"](A, Y, Z, x0)
    Q = cl["hess_fy"](A, Y, Z)
    r = cl["grad_fy"](A, Y, Z).ravel(order="F")
    H = cl["hess_fx"](A, Y, x0)
    assert J.shape == (N * K, d * K) and Q.shape == (N * K, N * K)
    np.testing.assert_allclose(H, J.T @ Q @ J, rtol=0, atol=1e-15 * float(np.max(np.abs(H))) * N)
    assert np.array_equal(Q, Q.T)
    g = cl["grad_fx"](A, Y, x0)
    np.testing.assert_allclose(g, J.T @ r, rtol=0, atol=1e-15 * N)
    h = 1e-6
    for j in (0, d + 2, d * K - 1):
        e = np.zeros(d * K)
        e[j] = h
        fd = (cl["f"](A, Y, x0 + e) - cl["f"](A, Y, x0 - e)) / (2 * h)
        assert abs(fd - g[j]) <= 1e-8 * max(1.0, abs(g[j])), (j, fd, g[j])
        gd = (cl["grad_fx"](A, Y, x0 + e) - cl["grad_fx"](A, Y, x0 - e)) / (2 * h)
        np.testing.assert_allclose(gd, H[:, j], rtol=0, atol=1e-8)
    if kind == "softmax_ce":     # the k / l indices matter at this x0: the off-diagonal blocks differ
        assert not np.allclose(H[:d, d:2 * d], H[:d, 2 * d:3 * d])
