"""CPU: the conditions under which tests/test_gpu_exact_products.py may demand exact equality, and
the census of pipeline shapes its Gram grid reaches (tests/exact_data.py).

Precondition: for every (N, m) of the grids, Σ|terms| < 2^53 for G, A x and Aᵀ v (exact_case asserts
it while it builds the case), the entries survive a round trip through fp32, and the float64 BLAS
product -- one more summation order -- equals the int64 one.

Census: gram_sia_body.h's run() has five shapes by nk = stages of 16 rows in the item's K range
(0: nothing, 1: body(f, f), 2: body(t, f) body(f, f), 3: the first body(t, t), >= 4: steady state).
Every class must occur, over the grid, for whole-K items and K pieces on both tile heights, for pair
items and for the items an AV launch designates.  A grid change that loses a class fails here."""
import numpy as np
import pytest

import exact_data as E


def _dense_grid():
    g = {(N, m) for tall in (False, True) for m in E.GRAM_M[tall] for N in E.GRAM_N}
    g |= {(N, m) for m, N in E.CHILD_SHAPES}
    g |= {(N, m) for N in E.GEMV_T_N + E.GEMV_N_N + E.COLUMNS_N for m in E.GEMV_M}
    g |= {(m + 77, m) for m in E.SOLVE_M}
    return sorted(g)


def test_grid_meets_the_exactness_precondition():
    worst = 0
    for N, m in _dense_grid():
        c = E.exact_case(N, m, E.case_seed(N, m))        # asserts Σ|terms| < 2^53
        worst = max(worst, c.bound)
        assert np.array_equal(c.A.astype(np.float32).astype(np.float64), c.A)
        assert c.A.min() >= -8191 and c.A.max() <= 8191
        if N >= 3:
            assert (c.w == 0).any() and (c.w > 0).any() and (c.w < 0).any()
        if N * m >= 1000:
            assert 0.05 < np.mean(c.A == 0) < 0.15
    print(f"max Σ|terms| over the grid: 2^{np.log2(worst):.1f}")
    # the large streaming case: bounds from the value ranges (its A is built as int16 on the device test)
    N, m = E.BIG
    assert N * 8191 * 1000 < E.LIMIT and m * 8191 * 1000 < E.LIMIT


@pytest.mark.parametrize("N,m", [(4144, 768), (1000, 700), (300, 129), (17, 1)])
def test_float64_blas_equals_int64(N, m):
    c = E.exact_case(N, m, E.case_seed(N, m))
    G = (c.A * c.w[:, None]).T @ c.A
    assert np.array_equal(G, c.G)
    assert np.array_equal(c.A @ c.x, c.Ax) and np.array_equal(c.A.T @ c.v, c.Atv)


@pytest.mark.parametrize("N,m", E.SPARSE_SHAPES)
def test_sparse_case_structure(N, m):
    s = E.sparse_case(N, m, E.case_seed(N, m))            # asserts the bound, duplicates, the dense row
    D = s.S.toarray()
    assert np.array_equal(s.coo.toarray(), D)             # scipy sums the duplicates of the float copy exactly
    assert np.array_equal(D.astype(np.float32).astype(np.int64), D)
    for r in s.empty_rows:
        assert not D[r].any()
    for j in s.empty_cols:
        assert not D[:, j].any()
    assert np.array_equal(s.G, E._imatmul((D * s.w.astype(np.int64)[:, None]).T, D))   # dense int64 == sparse int64
    assert np.array_equal(s.G, s.G.T)


def test_tile_lists_cover_the_lower_triangle():
    """The Python restatement of the lists: every 128-block (i, j), i >= j, exactly once."""
    for nb in (1, 2, 3, 9, 17):
        tl = E.tile_list_128(nb)
        assert sorted(tl) == [(i, j) for i in range(nb) for j in range(i + 1)]
    for nb in (2, 4, 6, 10, 96):
        nbi = nb // 2
        full = sum(2 * I + 2 for I in range(nbi))
        assert len(E.tile_list_tall(nb, False)) == full
        for pair in (False, True):
            tl = E.tile_list_tall(nb, pair)
            assert len(tl) == full - (nbi // 2 if pair else 0)
            blocks = []
            for x, y in tl:
                if y < 0:
                    blocks += [(2 * x + 1, 2 * x + 1), (2 * (-1 - y) + 1, 2 * (-1 - y) + 1)]
                else:
                    blocks += [(2 * x, y), (2 * x + 1, y)]
            low = sorted(b for b in blocks if b[0] >= b[1])
            assert low == [(i, j) for i in range(nb) for j in range(i + 1)]


def test_schedule_splits_small_systems():
    """gram_schedule on the grid's sizes: every tile is a tail tile cut into S = 16 pieces (m = 1024 on
    256 x 128 tiles: 10, the figure test_gpu_gram_diagpair records), pieces of L = ceil(Npad / 16 S) 16."""
    for tall in (False, True):
        for m in E.GRAM_M[tall]:
            its = E.gram_items(m, 1000, tall, True)
            assert {it["S"] for it in its} == {16} and all(it["k"] != "whole" for it in its)
    assert E.schedule(E.tile_list_tall(8, True), 32)[0] == 10
    assert E.schedule(E.tile_list_tall(8, False), 32)[0] == 10
    assert E.piece_stages(1008, 16, 0) == (4, 4) and E.piece_stages(1008, 16, 15) == (3, 4)
    assert E.piece_stages(304, 16, 9) == (1, 2) and E.piece_stages(304, 16, 10) == (0, 2)
    assert E.piece_stages(32, 16, 2) == (0, 1)            # k0 past Npad: clamped to an empty range


def test_stage_count_census():
    t = E.census()
    missing = [(row, c) for row, classes in E.REQUIRED.items() for c in classes if not t.get((row, c))]
    assert not missing, missing
    assert not t.get(("whole 128", "0")) and not t.get(("whole 256", "0"))   # nk = 0: K pieces only
    # every item kind of the 256 x 128 lists meets every class as well
    for kind in ("pair 256", "UD1 256", "D0L 256", "off 256", "diag 128", "off 128"):
        for c in E.NK_CLASSES:
            assert t.get((kind, c)), (kind, c)
    # a short last piece with work in it (0 < nk < L / 16) occurs on both tile heights
    for sz in ("128", "256"):
        assert any(t.get((f"last piece {sz}", c)) for c in ("1", "2", "3"))
    print(E.census_markdown())
