"""GPU: the staging loads of the panel-blocked interleaved Gram kernels go through buffer descriptors
on scalar bases (gram_sia_body.h SB) and load exactly what the per-lane pointers loaded: G's lower
triangle, sampled G entries and the fused Aᵀv are bit for bit those of the pointer form
(SCS_GRAM_ADDR=0, gram_sia_kernel<26, 4, ...>), of the register-staged gram_f64_kernel on 128 x 128
tiles, and, on an fp32-stored A, of the fp64 kernel on the widened values.  Sizes as in
test_gpu_gram_edges.py: pair tiles and a lone [U; D1] tile, K-split pieces (k0 > 0), a K tail (1000 is
no multiple of 16), the designated Aᵀv tiles.  The switches are read once per process: each arm runs in
a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
SIZES = [(512, 1000), (768, 1000), (1024, 4144)]

# argv: package path, output file, "m:N,m:N,...", "f32" or "-"
_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import scsopt
from scsopt import losses
out = {}
def record(tag, p, w, v, pairs):
    out[f"G_{tag}"] = np.tril(p.gram(w))
    out[f"nameG_{tag}"] = p.ctx.kernel_names()[0]
    g, atv, fused = p.gram_atv_sample(w, v, pairs)
    out[f"g_{tag}"] = g
    out[f"atv_{tag}"] = atv
    out[f"fused_{tag}"] = fused
    out[f"name_{tag}"] = p.ctx.kernel_names()[0]
for mn in sys.argv[3].split(","):
    m, N = (int(x) for x in mn.split(":"))
    rng = np.random.default_rng(3000 * m + N)
    A = rng.standard_normal((N, m)); w = rng.standard_normal(N); w[::5] = 0.0; v = rng.standard_normal(N)
    pairs = np.concatenate([np.array([(255, 128), (m - 1, m - 128), (5, 3), (200, 100), (m - 1, 0)]),
                            rng.integers(0, m, size=(32, 2))])
    p = scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
    record(f"{m}", p, w, v, pairs)
    if "SCS_GRAM_TALL" not in os.environ and os.environ.get("SCS_GRAM_SIA") != "0":
        os.environ["SCS_GRAM_FUSE"] = "2"   # read per call: the 128 x 128 kernel with the fused Aᵀv
        g, atv, fused = p.gram_atv_sample(w, v, pairs)
        assert fused
        out[f"gfuse_{m}"] = g
        out[f"namefuse_{m}"] = p.ctx.kernel_names()[0]
        del os.environ["SCS_GRAM_FUSE"]
    p.ctx.close()
    if sys.argv[4] == "f32":
        A32 = A.astype(np.float32)
        for tag, q in (("s", scsopt.Problem(A32, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0, dense_f32=True)),
                       ("d", scsopt.Problem(A32.astype(np.float64), np.zeros(N), np.zeros(m), losses.least_squares(), 1.0))):
            record(f"{tag}{m}", q, w, v, pairs)
            q.ctx.close()
np.savez(sys.argv[2], **out)
"""


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b, m, keys=("G", "g", "atv")):
    for k in keys:
        assert np.array_equal(bits(a[f"{k}_{m}"]), bits(b[f"{k}_{m}"])), (k, m)


def _run(tmp, label, sizes, f32=False, **env):
    f = tmp / f"{label}.npz"
    e = {k: v for k, v in os.environ.items() if not k.startswith("SCS_")}
    e.update(env)
    subprocess.run([sys.executable, "-c", _CHILD, PKG, str(f), ",".join(f"{m}:{N}" for m, N in sizes),
                    "f32" if f32 else "-"], env=e, check=True, timeout=300)
    return np.load(f)


@pytest.fixture(scope="module")
def tall_default(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("addr_tall"), "default", SIZES, f32=True, SCS_GRAM_TALL="1")


@pytest.fixture(scope="module")
def small_default(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("addr_small"), "default", SIZES[:1], f32=True)


def test_scalar_base_staging_against_pointer_form(tall_default, tmp_path):
    new, old = tall_default, _run(tmp_path, "addr0", SIZES, SCS_GRAM_TALL="1", SCS_GRAM_ADDR="0")
    for m, _ in SIZES:
        assert new[f"fused_{m}"] and old[f"fused_{m}"]
        assert str(new[f"name_{m}"]) == "gram_sia_kernel<10, 4, false, true, false>"
        assert str(new[f"nameG_{m}"]) == "gram_sia_kernel<10, 4, false, false, false>"
        assert str(old[f"name_{m}"]) == "gram_sia_kernel<26, 4, false, true, false>"
        assert str(old[f"nameG_{m}"]) == "gram_sia_kernel<26, 4, false, false, false>"
        same(new, old, m)


def test_128_tiles_against_register_staged_kernel(small_default, tmp_path):
    m = SIZES[0][0]
    new, old = small_default, _run(tmp_path, "sia0", SIZES[:1], SCS_GRAM_SIA="0")
    assert str(new[f"nameG_{m}"]) == "gram_sia_kernel<1, 2, false, false, false>"
    assert str(new[f"namefuse_{m}"]) == "gram_sia_kernel<1, 2, false, true, false>"
    assert str(old[f"nameG_{m}"]).startswith("gram_f64_kernel")
    same(new, old, m)
    assert np.array_equal(bits(new[f"gfuse_{m}"]), bits(old[f"g_{m}"]))


def test_f32_stored_tall_against_fp64_on_widened(tall_default):
    r = tall_default
    for m, _ in SIZES:
        assert str(r[f"name_s{m}"]) == "gram_sia_ta_kernel<float, 4, true>"
        assert str(r[f"nameG_s{m}"]) == "gram_sia_ta_kernel<float, 4, false>"
        assert str(r[f"name_d{m}"]) == "gram_sia_kernel<10, 4, false, true, false>"
        for k in ("G", "g", "atv"):
            assert np.array_equal(bits(r[f"{k}_s{m}"]), bits(r[f"{k}_d{m}"])), (k, m)


def test_f32_stored_128_tiles_against_fp64_on_widened(small_default):
    r, m = small_default, SIZES[0][0]
    assert str(r[f"nameG_s{m}"]) == "gram_sia_ta_kernel<float, 2, false>"
    assert str(r[f"nameG_d{m}"]) == "gram_sia_kernel<1, 2, false, false, false>"
    for k in ("G", "g", "atv"):
        assert np.array_equal(bits(r[f"{k}_s{m}"]), bits(r[f"{k}_d{m}"])), (k, m)
