"""CPU: what minibatches of a multi-output loss (scs_set_multi_batches / multi_batches=True) promise
without a GPU -- the header prototypes, the Python and the Julia bindings of the two new entry points,
the Python-side argument checks, and the reference conditions of tests/test_gpu_multi_batches.py: the
oracle itself runs clean on every trajectory the GPU tests compare against, and each batch takes the
branch the case list states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multi_batches_data as B
import multi_output_data as M
from multi_batches_data import O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "scsopt.h")
JL = os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd", "julia", "SCSOptAMD.jl")
PKG = os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd", "scsopt")
NEW = ("scs_set_multi_batches", "scs_get_batch_data")


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int)\s+(scs_\w+)\s*\(([^)]*)\)\s*;", src):
        out[name] = (ret, [re.sub(r"\s*\w+$", "", a.strip()) for a in args.split(",")])
    return out


def test_header_declares_the_entry_points():
    protos = _protos()
    assert protos["scs_set_multi_batches"] == ("int", ["scs_ctx*", "int"])
    assert protos["scs_get_batch_data"] == ("int", ["scs_ctx*", "int64_t", "double*", "int64_t", "double*"])
    doc = open(HDR).read()
    lead = doc[doc.index("multi-output targets"):doc.index("int scs_set_outputs")]
    assert "scs_set_multi_batches" in lead           # the refusal list of scs_set_outputs points to the switch


def test_python_binding_lists_the_entry_points():
    src = open(os.path.join(PKG, "_lib.py")).read()
    assert re.search(r'"scs_set_multi_batches":\s*\(C\.c_int,\s*\[C\.c_void_p,\s*C\.c_int\]\)', src)
    assert re.search(r'"scs_get_batch_data":\s*\(C\.c_int,\s*\[C\.c_void_p,\s*C\.c_int64,\s*c_dp,\s*C\.c_int64,'
                     r'\s*c_dp\]\)', src)
    prob = open(os.path.join(PKG, "problems.py")).read()
    assert "multi_batches=False" in prob and "scs_set_multi_batches(self.ctx.h, 1)" in prob
    assert "def set_multi_batches(self, on=True)" in prob and "def get_batch_data(self, b)" in prob


def test_loaded_binding_has_the_symbols():
    from scsopt import _lib
    from conftest import LIB
    lib = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED
    fn = _lib.lib.scs_set_multi_batches
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    fn = _lib.lib.scs_get_batch_data
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int64, _lib.c_dp, C.c_int64, _lib.c_dp]


def test_julia_ccall_matches_the_header():
    src = open(JL).read()
    calls = re.findall(r"ccall\(\(:scs_set_multi_batches,\s*lib\),\s*(\w+),\s*\(([^()]*)\)", src)
    assert len(calls) >= 2                                # the constructor keyword and set_multi_batches!
    for ret, args in calls:
        assert ret == "Cint" and [a.strip() for a in args.split(",")] == ["Ptr{Cvoid}", "Cint"]
    assert "multi_batches::Bool=false" in src and "set_multi_batches!" in src
    assert "set_multi_batches!" in src[src.index("export DeviceProblem"):src.index("const lib")]
    # plumbed as multi_sample is: the switch goes before the data door
    ctor = src[src.index("multi_batches::Bool=false"):]
    assert ctor.index(":scs_set_multi_batches") < ctor.index(":scs_set_data")


def test_python_argument_checks():
    """multi_batches= is checked before any context exists (these raise on a host without a GPU too)."""
    import scsopt
    from scsopt import losses
    N, d, K = 20, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    f, of = M.device_losses(losses, "softmax_ce", K, 1.0 / N)
    with pytest.raises(TypeError, match="multi_batches must be a bool"):
        scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, multi_batches="yes")
    with pytest.raises(TypeError, match="multi_batches must be a bool"):
        scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, multi_batches=1)
    with pytest.raises(ValueError, match=r"multi_batches=True.*devices=\[\.\.\.\]"):
        scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, multi_batches=True, devices=[0, 0], device_exchange="host")


def test_case_list_states_the_oracles_branches():
    """Each case's batch sizes and the branch ggn_score_step_general takes on each batch."""
    for (N, d, K), bs, sizes, pattern in B.CASES:
        batches = O.loader_batches(N, bs, shuffle_batch=True, perm=B.perm_of(N))
        assert tuple(len(r) for r in batches) == sizes
        assert B.branches(batches, d, K) == pattern
        assert sorted(np.concatenate(batches).tolist()) == list(range(N))
    assert {c[3] for c in B.CASES} >= {"FFS", "SSS", "FF"}          # mixed, sample only, feature only
    assert [c[0] for c in B.NSCORE_CASES] == [(200, 17, 7), (520, 129, 2)]


def _clean(sol, max_epoch):
    assert np.all(np.isfinite(sol.obj)) and np.all(np.isfinite(sol.x))
    assert sol.epochs == max_epoch
    assert np.abs(sol.obj).max() < 1e3


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_oracle_runs_clean_on_the_gpu_trajectories(case, kind):
    """The runs test_gpu_multi_batches.py compares against (6 epochs, λ = 2e-3): finite, no early stop."""
    shape, bs = case[0], case[1]
    for method in ("lqn", "ggn") + (("nscore",) if case in B.NSCORE_CASES else ()):
        _clean(B.oracle_run(kind, method, shape, bs), 6)


def test_oracle_nscore_blows_up_on_rank_deficient_batches():
    """Why ProxNSCORE is compared on the n_b >= d cases only: on (40, 33, 16) / 17 with the softmax loss the
    oracle itself leaves every sensible range."""
    sol = B.oracle_run("softmax_ce", "nscore", (40, 33, 16), 17, 2e-3, 4)
    assert not np.all(np.isfinite(sol.obj)) or np.abs(sol.obj).max() > 1e20


def test_oracle_runs_clean_on_the_other_gpu_cases():
    """λ = 2e-2, the loader options and the held-out set."""
    _clean(B.oracle_run("softmax_ce", "ggn", (300, 130, 3), 137, 2e-2), 6)
    for method in ("ggn", "lqn"):
        _clean(B.oracle_run("softmax_ce", method, (200, 17, 7), None, loader=(("slice_samples", True),)), 6)
    _clean(B.oracle_run("softmax_ce", "lqn", (300, 130, 3), None, 2e-3, 6, False,
                        (("batch_size", 128), ("shuffle_batch", False))), 6)
    _clean(B.oracle_run("softmax_ce", "lqn", (300, 130, 3), None, 2e-3, 1, False,
                        (("batch_size", 128), ("shuffle_batch", False), ("local_max_iter", 2.7))), 1)
    _clean(B.oracle_run("softmax_ce", "ggn", (200, 17, 7), 200), 6)
    sol = B.oracle_run("softmax_ce", "ggn", (200, 17, 7), 50, test=True)
    _clean(sol, 6)
    assert len(sol.fvaltest) == len(sol.obj) and np.all(np.isfinite(sol.fvaltest))


def test_gather_lists_cover_the_edges():
    lists = B.gather_lists()
    assert any(r[-1] == B.GATHER_N - 1 for r in lists) and B.GATHER_N % 16 != 0
    assert any(len(set(r.tolist())) < len(r) for r in lists)
    assert all(0 <= r.min() and r.max() < B.GATHER_N for r in lists)
