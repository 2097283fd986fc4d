"""GPU: the issue order at the stage barriers of the interleaved 256 x 128 Gram kernels (SCS_GRAM_SIA =
8 + bits, gram_sia_body.h E1 / E2 / E3; 10 = the default, 12 the other arm built) changes no MFMA of
any accumulator: G's lower triangle and the fused Aᵀv are bit for bit those of the previous order
(SCS_GRAM_SIA=8), tail-balanced schedule and pair tiles included.  The switch is read once per
process: each arm runs in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
SIZES = [(512, 1000), (768, 1000), (1024, 4144)]

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import scsopt
from scsopt import losses
out = {}
for m, N in ((512, 1000), (768, 1000), (1024, 4144)):
    rng = np.random.default_rng(3000 * m + N)
    A = rng.standard_normal((N, m)); w = rng.standard_normal(N); w[::5] = 0.0; v = rng.standard_normal(N)
    p = scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
    out[f"G_{m}"] = np.tril(p.gram(w))
    out[f"nameG_{m}"] = p.ctx.kernel_names()[0]
    pairs = np.concatenate([np.array([(255, 128), (m - 1, m - 128), (5, 3), (200, 100), (m - 1, 0)]),
                            rng.integers(0, m, size=(32, 2))])
    g, atv, fused = p.gram_atv_sample(w, v, pairs)
    assert fused
    out[f"g_{m}"] = g
    out[f"atv_{m}"] = atv
    out[f"name_{m}"] = p.ctx.kernel_names()[0]
    p.ctx.close()
np.savez(sys.argv[2], **out)
"""


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run(tmp_path, sia):
    f = tmp_path / f"sia{sia}.npz"
    e = {k: v for k, v in os.environ.items() if not k.startswith("SCS_")}
    e.update(SCS_GRAM_TALL="1", SCS_GRAM_SIA=str(sia))
    subprocess.run([sys.executable, "-c", _CHILD, PKG, str(f)], env=e, check=True, timeout=300)
    return np.load(f)


@pytest.fixture(scope="module")
def previous_order(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("edges_ref"), 8)


@pytest.mark.parametrize("sia", [10, 12])
def test_barrier_edge_order_bitwise(sia, previous_order, tmp_path):
    new, old = _run(tmp_path, sia), previous_order
    for m, _ in SIZES:
        assert str(old[f"name_{m}"]) == "gram_sia_kernel<1, 4, false, true, false>"
        assert str(new[f"name_{m}"]) == f"gram_sia_kernel<{sia}, 4, false, true, false>"
        assert str(new[f"nameG_{m}"]) == f"gram_sia_kernel<{sia}, 4, false, false, false>"
        assert np.array_equal(bits(new[f"G_{m}"]), bits(old[f"G_{m}"])), m
        assert np.array_equal(bits(new[f"g_{m}"]), bits(old[f"g_{m}"])), m
        assert np.array_equal(bits(new[f"atv_{m}"]), bits(old[f"atv_{m}"])), m
