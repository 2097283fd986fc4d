"""GPU: the main Gram's paired diagonal tiles (SCS_GRAM_DIAGPAIR, csrc/gram_tiles.h).

On 256 x 128 tiles the unpacked launches' list holds, for every two row blocks (I, I'), one pair tile
[D1(I); D1(I')] in place of the two tiles [U; D1] whose upper halves recompute a mirror block that
nothing reads.  Every stored element takes the MFMAs it took before, in the same order, so G's lower
triangle and the fused Aᵀv are compared bit for bit against SCS_GRAM_DIAGPAIR=0 wherever the K split
of the tail-balanced schedule is the same on both lists.  The switches are read once per process:
each arm runs in a child process (as test_interleaved_gram_bitwise_vs_previous_kernels does)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scsopt
from scsopt import losses

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")

# argv: package dir, output .npz, mode.  G's lower triangle is returned as one SHA-256 per 128-row
# block row (equal digests <=> equal bits; m = 4096 would otherwise move 4 x 134 MB through files).
_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import scsopt
from scsopt import losses
mode = sys.argv[3]
out = {}
def tril_digest(G):
    T = np.tril(G)
    return np.array([hashlib.sha256(T[r:r + 128].tobytes()).hexdigest() for r in range(0, T.shape[0], 128)])
def weights(rng, N):
    w = rng.standard_normal(N)      # negative weights too
    w[::7] = 0.0                    # and zeros
    return w
def sample_pairs(rng, m):
    fixed = [(255, 128), (m - 1, m - 128), (200, 130), (m - 3, m - 100),      # paired D1 blocks (1,1), (nb-1,nb-1)
             (5, 3), (127, 0), (m - 129, m - 256), (300, 257),                # D0 blocks
             (200, 100), (m - 1, m - 200), (255, 0),                          # L blocks (2I+1, 2I)
             (m - 1, 0), (300, 17), (m - 130, 140), (511, 129)]               # off-diagonal tiles
    return np.concatenate([np.array(fixed), rng.integers(0, m, size=(32, 2))])
if mode == "gram":
    for m in (512, 768, 4096):
        for N in (1000, 4144):
            rng = np.random.default_rng(1000 * m + N)
            A = rng.standard_normal((N, m)); w = weights(rng, N)
            p = scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
            out[f"G_{m}_{N}"] = tril_digest(p.gram(w))
            p.ctx.close()
    m, N = 768, 1000
    rng = np.random.default_rng(5)
    A32 = rng.standard_normal((N, m)).astype(np.float32); w = weights(rng, N)
    p = scsopt.Problem(A32, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0, dense_f32=True)
    out["G_f32"] = tril_digest(p.gram(w))
    out["name_f32"] = p.ctx.kernel_names()[0]
elif mode == "sched":
    for m in (512, 768, 1024):
        for N in (1000, 4144):
            rng = np.random.default_rng(2000 * m + N)
            A = rng.standard_normal((N, m)); w = weights(rng, N); v = rng.standard_normal(N)
            p = scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
            out[f"G_{m}_{N}"] = tril_digest(p.gram(w))
            g, atv, fused = p.gram_atv_sample(w, v, sample_pairs(rng, m))
            assert fused
            out[f"g_{m}_{N}"] = g
            out[f"atv_{m}_{N}"] = atv
            out[f"name_{m}_{N}"] = p.ctx.kernel_names()[0]
            p.ctx.close()
elif mode == "traj":
    N, m = 3001, 512
    x0 = np.random.default_rng(21).standard_normal(m) * 0.5
    p = scsopt.Problem.synthetic(N, m, x0, losses.logistic_ce(1.0 / N), 2e-3, kind=1, seed=17,
                                 out_fn=losses.sigmoid_ce(1.0 / N))
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3, x_tol=0.0,
                         f_tol=0.0, verbose=0)
    out["obj"] = np.array(sol.obj); out["x"] = sol.x; out["name"] = p.ctx.kernel_names()[0]
np.savez(sys.argv[2], **out)
"""


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _arms(tmp_path, mode, env):
    """The child under pairing on (the default: the switch unset) and SCS_GRAM_DIAGPAIR=0."""
    outs = {}
    for tag, extra in (("pair", {}), ("nopair", {"SCS_GRAM_DIAGPAIR": "0"})):
        f = tmp_path / f"{tag}.npz"
        e = {k: v for k, v in os.environ.items() if not k.startswith("SCS_")}
        e.update(env)
        e.update(extra)
        subprocess.run([sys.executable, "-c", _CHILD, PKG, str(f), mode], env=e, check=True, timeout=300)
        outs[tag] = np.load(f)
    assert sorted(outs["pair"].files) == sorted(outs["nopair"].files)
    return outs["pair"], outs["nopair"]


def test_pair_tiles_bitwise_without_k_split(tmp_path):
    """No tail schedule (SCS_GRAM_SCHED=0), forced 256 x 128 tiles: one pair (m = 512), one pair plus the
    unpaired odd row block (m = 768), eight pairs across super-blocks (m = 4096); N = 1000 (pads to
    1008) and 4144; weights with negative and zero entries; once on an fp32-stored A."""
    a, b = _arms(tmp_path, "gram", {"SCS_GRAM_SCHED": "0", "SCS_GRAM_TALL": "1"})
    keys = [k for k in a.files if k.startswith("G_")]
    assert len(keys) == 7
    for k in keys:
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0])
    assert str(a["name_f32"]) == str(b["name_f32"]) == "gram_sia_ta_kernel<float, 4, false>"


def test_pair_tiles_bitwise_default_schedule(tmp_path):
    """The tail-balanced schedule, forced 256 x 128 tiles, m = 512 / 768 / 1024: every tile is a tail
    tile and gram_schedule's split factor is 16 / 16 / 10 on both lists (5 / 11 / 18 items against
    6 / 12 / 20), so G's lower triangle and the fused Aᵀv match bit for bit -- K pieces, partial
    slots and gram_combine_kernel of pair tiles included."""
    a, b = _arms(tmp_path, "sched", {"SCS_GRAM_TALL": "1"})
    for m in (512, 768, 1024):
        for N in (1000, 4144):
            k = f"{m}_{N}"
            assert str(a["name_" + k]) == str(b["name_" + k]) == "gram_sia_kernel<10, 4, false, true, false>"
            assert np.array_equal(a["G_" + k], b["G_" + k]), (k, np.nonzero(a["G_" + k] != b["G_" + k])[0])
            assert np.array_equal(bits(a["g_" + k]), bits(b["g_" + k])), k
            assert np.array_equal(bits(a["atv_" + k]), bits(b["atv_" + k])), k


def test_pair_tiles_default_path(monkeypatch):
    """No switches, m = 12288 (nb = 96: 256 x 128 tiles by default, 24 pair tiles), N = 1024: sampled G
    entries (paired D1 blocks, D0, L and off-diagonal tiles) and Aᵀv against host fp64 dots of the
    columns read back, bench.py's bound 1e-11 · Σ|terms|."""
    for k in list(os.environ):
        if k.startswith("SCS_"):
            monkeypatch.delenv(k)
    N, m = 1024, 12288
    rng = np.random.default_rng(61)
    w = rng.random(N) + 0.5
    v = rng.standard_normal(N)
    p = scsopt.Problem.synthetic(N, m, np.zeros(m), losses.least_squares(1.0 / N), 1.0, kind=3, seed=63)
    # blocks 0, 1 (I = 0), 39 (D1 of I = 19), 50 (D0 of I = 25), 94, 95 (I = 47, the last pair's second)
    cols = np.array([3, 130, 200, 255, 5000, 5100, 6400, 6500, m - 256, m - 100, m - 1])
    pairs = [(int(i), int(j)) for a, i in enumerate(cols) for j in cols[a:]]
    g, atv, fused = p.gram_atv_sample(w, v, pairs)
    assert fused
    assert p.ctx.kernel_names()[0] == "gram_sia_kernel<10, 4, false, true, false>"   # a 256 x 128 kernel
    Ac = p.get_columns(cols)
    col = {int(c): k for k, c in enumerate(cols)}
    worst = 0.0
    for (i, j), gv in zip(pairs, g):
        x, y = Ac[:, col[i]], Ac[:, col[j]]
        worst = max(worst, abs(gv - float((x * w) @ y)) / (1e-11 * float(np.abs(x * w * y).sum()) + 1e-300))
    bound = 1e-11 * (np.abs(Ac).T @ np.abs(v))
    worst_v = float(np.max(np.abs(atv[cols] - Ac.T @ v) / (bound + 1e-300)))
    print("max err / bound: G", worst, "Aᵀv", worst_v)
    assert worst <= 1.0 and worst_v <= 1.0


def test_pair_tiles_trajectory(tmp_path):
    """Three ProxGGNSCORE epochs (logistic + l1) on forced 256 x 128 tiles, m = 512, N = 3001, pairing on
    against off: the same objectives at rtol 1e-12 and the same sign / zero pattern of x."""
    a, b = _arms(tmp_path, "traj", {"SCS_GRAM_TALL": "1"})
    assert str(a["name"]) == str(b["name"]) == "gram_sia_kernel<10, 4, false, true, false>"
    assert a["obj"].shape == b["obj"].shape
    np.testing.assert_allclose(a["obj"], b["obj"], rtol=1e-12, atol=0)
    assert np.array_equal(np.sign(a["x"]), np.sign(b["x"]))
