"""Integer data on which Aᵀ diag(w) A, A·x and Aᵀ·v have one right answer in float64, and a host
census of the software-pipeline shapes (`nk`, stages of 16 rows) that the main Gram's items take.

exact_case: A in [-8191, 8191] (13 bits: a product of two entries needs 26, so an fp32 multiply or
accumulate anywhere shows), w in [-4, 4], v and x in [-1000, 1000].  Every product and every partial
sum of any summation order is an integer of magnitude <= Σ|terms| < 2^53, hence a double, and fma
rounds nothing: MFMA order, K pieces + combine, partial slots, the chunked finalize, the sparse walks
and the streaming ring must all give the int64 result bit for bit.  The entries are exact in fp32
too, so the fp32-stored arms see the same problem (fp32 storage ROUNDING is not probed by this data).

The census restates, in Python, the host code that decides how many stages an item runs:
  gram_tile_list          csrc/gram.hip 581-591   (128 x 128 tiles, super-blocks of 8)
  gram_tile_list_tall_t   csrc/gram_tiles.h 58-77 (256 x 128 tiles, unpaired / paired)
  gram_schedule           csrc/gram.hip 1132-1179 (tail tiles cut into S K pieces)
  the piece length L      csrc/gram_sia_body.h 48-52, nk at 192, run() at 194-259
  ensure_gram             csrc/scsopt.cpp 704-773  (slots per XCD: 64 / 32; which list is scheduled)
"""
import functools
from types import SimpleNamespace

import numpy as np

LIMIT = 1 << 53
GBK = 16          # rows per stage (common.h)

# ---------------------------------------------------------------------------
# the grids of tests/test_gpu_exact_products.py (the host tests check every case of them)
# ---------------------------------------------------------------------------
GRAM_M = {False: (1, 127, 128, 129, 384),          # 128 x 128 tiles (the default at these sizes)
          True: (130, 256, 512, 700, 768)}         # 256 x 128 tiles (SCS_GRAM_TALL=1)
GRAM_N = (1, 17, 40, 300, 700, 1000, 4144)
FUSED_N = (17, 40, 300, 1000)
CHILD_SHAPES = ((768, 40), (512, 700), (384, 300), (512, 1000))   # (m, N); the last: a non-empty 16th K piece
GEMV_T_N = (1, 4095, 4097, 12300, 16400)
GEMV_N_N = (1, 2, 511, 513, 4099)
GEMV_M = (1, 127, 129, 640)
BIG = (261700, 520)                                  # (N, m) of the one large streaming case
COLUMNS_N = (1, 17, 4097)
SOLVE_M = (1, 2, 127, 128, 129, 255, 256, 257, 385)
SPARSE_SHAPES = ((700, 300), (300, 4200))            # (N, m)
RING_ROWS = (16, 48, 256)                            # SCS_SPARSE_CHUNK_ROWS; 256: 16 stages, all 16 K pieces non-empty


def case_seed(N, m):
    return 1000003 * m + N


def _imatmul(a, b):
    """a @ b in int64 arithmetic (torch's integer matmul where torch is present: NumPy's runs without
    BLAS, about 40 s for the largest Gram of the grid against 0.5 s)."""
    try:
        import torch
    except ImportError:
        return a @ b
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


def _check_bound(name, terms):
    worst = int(terms.max()) if terms.size else 0
    assert worst < LIMIT, f"{name}: max Σ|terms| = {worst} >= 2^53"
    return worst


@functools.lru_cache(maxsize=None)
def exact_case(N, m, seed, zero_frac=0.1):
    """Integer A (N x m, float64, about zero_frac zeros), w (zeros and negatives), v, x and the int64
    references G = Aᵀ diag(w) A, Ax = A x, Atv = Aᵀ v.  Asserts Σ|terms| < 2^53 for all three (a
    condition of the method, not a tolerance).  Cached: the arms of a case share one reference, which
    they must not modify (the arrays are read-only)."""
    rng = np.random.default_rng(seed)
    Ai = rng.integers(-8191, 8192, size=(N, m), dtype=np.int64)
    Ai[rng.random((N, m)) < zero_frac] = 0
    wi = rng.integers(-4, 5, size=N, dtype=np.int64)
    if N >= 3:
        wi[[0, N // 2, N - 1]] = (-3, 0, 4)        # a zero and both signs at every size
    vi = rng.integers(-1000, 1001, size=N, dtype=np.int64)
    xi = rng.integers(-1000, 1001, size=m, dtype=np.int64)
    absA = np.abs(Ai)
    sg = _check_bound("G", (absA * np.abs(wi)[:, None]).sum(axis=0)[:, None] * absA.max(axis=0)[None, :])
    sx = _check_bound("A x", absA @ np.abs(xi))
    sv = _check_bound("Aᵀ v", absA.T @ np.abs(vi))
    return _Case(Ai, wi, vi, xi, max(sg, sx, sv))


class _Case:
    """One exact_case: A, w, v, x as float64 and the int64 references Ax, Atv and (formed at first use:
    the streaming cases never ask for it) G."""

    def __init__(self, Ai, wi, vi, xi, bound):
        self.N, self.m = Ai.shape
        self._Ai, self._wi, self.bound = Ai, wi, bound
        self.A, self.w, self.v, self.x = (a.astype(np.float64) for a in (Ai, wi, vi, xi))
        self.Ax, self.Atv = Ai @ xi, Ai.T @ vi
        for a in (self.A, self.w, self.v, self.x, self.Ax, self.Atv):
            a.setflags(write=False)

    @functools.cached_property
    def G(self):
        G = _imatmul((self._Ai * self._wi[:, None]).T, self._Ai)
        G.setflags(write=False)
        return G


def sparse_case(N, m, seed):
    """A user CSR in COO form with integer values: unsorted entries, duplicates (the device sums
    them), empty rows and columns, and one row dense in every column block.  Returns the COO matrix
    (float64 values), the summed matrix as int64 CSR, w, v, x and the int64 references."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    nnz = int(0.03 * N * m)
    rows = rng.integers(0, N, nnz)
    cols = rng.integers(0, m, nnz)
    dense_row = N // 3
    rows = np.concatenate([rows, np.full(m, dense_row), rows[:200]])       # the dense row; 200 duplicates
    cols = np.concatenate([cols, np.arange(m), cols[:200]])
    vals = rng.integers(-4000, 4001, rows.size, dtype=np.int64)            # a summed pair stays within 13 bits
    vals[vals == 0] = 7
    empty_rows, empty_cols = (5, N - 1), (20, m - 2)
    keep = ~np.isin(rows, empty_rows) & ~np.isin(cols, empty_cols)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    perm = rng.permutation(rows.size)
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    coo = sp.coo_matrix((vals.astype(np.float64), (rows, cols)), shape=(N, m))
    Si = sp.coo_matrix((vals, (rows, cols)), shape=(N, m)).tocsr()         # int64, duplicates summed
    Si.sum_duplicates()
    assert len(set(zip(rows.tolist(), cols.tolist()))) < rows.size          # duplicates are present
    assert Si[dense_row].nnz == m - len(empty_cols)
    wi = rng.integers(-4, 5, size=N, dtype=np.int64)
    vi = rng.integers(-1000, 1001, size=N, dtype=np.int64)
    xi = rng.integers(-1000, 1001, size=m, dtype=np.int64)
    absS = abs(Si)
    colmax = np.asarray(absS.max(axis=0).todense()).ravel().astype(np.int64)
    sg = _check_bound("G", np.asarray(absS.T @ np.abs(wi)).ravel()[:, None] * colmax[None, :])
    sx = _check_bound("A x", np.asarray(absS @ np.abs(xi)).ravel())
    sv = _check_bound("Aᵀ v", np.asarray(absS.T @ np.abs(vi)).ravel())
    G = (Si.T @ sp.diags(wi) @ Si).toarray().astype(np.int64)
    return SimpleNamespace(N=N, m=m, coo=coo, S=Si, w=wi.astype(np.float64), v=vi.astype(np.float64),
                           x=xi.astype(np.float64), G=G, Ax=np.asarray(Si @ xi).ravel(),
                           Atv=np.asarray(Si.T @ vi).ravel(), bound=max(sg, sx, sv),
                           empty_rows=empty_rows, empty_cols=empty_cols, dense_row=dense_row)


def solve_case(m, seed, indefinite=False):
    """(A, w, d, rhs, M) with M = Aᵀ diag(w) A + diag(d) formed in int64.  SPD: w, d in 1..4.
    indefinite: w of mixed sign, mostly negative, so that M has a negative eigenvalue (for m = 1:
    w < 0 and d = 1); the caller checks the eigenvalue on the host."""
    N = m + 77
    c = exact_case(N, m, seed)
    rng = np.random.default_rng(seed + 1)
    Ai = c.A.astype(np.int64)
    if indefinite:
        wi = -rng.integers(1, 5, size=N, dtype=np.int64)
        if m > 1:
            wi[rng.random(N) < 0.3] *= -1
        di = np.ones(m, dtype=np.int64)
    else:
        wi = rng.integers(1, 5, size=N, dtype=np.int64)
        di = rng.integers(1, 5, size=m, dtype=np.int64)
    rhs = rng.integers(-1000, 1001, size=m, dtype=np.int64)
    M = _imatmul((Ai * wi[:, None]).T, Ai) + np.diag(di)
    _check_bound("M", _imatmul((np.abs(Ai) * np.abs(wi)[:, None]).T, np.abs(Ai)) + np.diag(di))
    return SimpleNamespace(N=N, m=m, A=c.A, w=wi.astype(np.float64), d=di.astype(np.float64),
                           rhs=rhs.astype(np.float64), M=M)


# ---------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------
def round_up(a, b):
    return (a + b - 1) // b * b


def tile_list_128(nb):
    """gram_tile_list (gram.hip 581-591): items (i, j), i >= j, super-blocks of 8."""
    S, out = 8, []
    nsb = (nb + S - 1) // S
    for sbi in range(nsb):
        for sbj in range(sbi + 1):
            for i in range(sbi * S, min((sbi + 1) * S, nb)):
                for j in range(sbj * S, min((sbj + 1) * S, nb)):
                    if i >= j:
                        out.append((i, j))
    return out


def tile_list_tall(nb, pair):
    """gram_tile_list_tall_t (gram_tiles.h 58-77): items (I, j), or (I, -1 - I') for a pair tile."""
    nbi, SI, SJ, out = nb // 2, 4, 8, []
    for sbi in range((nbi + SI - 1) // SI):
        for sbj in range(sbi + 1):
            for I in range(sbi * SI, min((sbi + 1) * SI, nbi)):
                for j in range(sbj * SJ, min((sbj + 1) * SJ, nb)):
                    if j > 2 * I + 1:
                        continue
                    if pair and j == 2 * I + 1:
                        if I % 2 == 1:
                            continue
                        if I + 1 < nbi:
                            out.append((I, -1 - (I + 1)))
                            continue
                    out.append((I, j))
    return out


def schedule(tiles, slots):
    """gram_schedule (gram.hip 1132-1179) without the order of the whole tiles (diag_first moves
    them only): the split factor S and the work items (x, y, piece), piece = -1 for a whole tile."""
    nt = len(tiles)
    q, r = divmod(nt, 8)
    ns = [q + (1 if x < r else 0) for x in range(8)]
    tail_max = max(n % slots for n in ns)
    S = 1
    if tail_max > 0 and 4 * tail_max < 3 * slots:
        S = max(2, min(16, slots // tail_max))
    items, t0 = [], 0
    for n in ns:
        tail = n % slots if S > 1 else 0
        items += [(x, y, -1) for x, y in tiles[t0:t0 + n - tail]]
        for x, y in tiles[t0 + n - tail:t0 + n]:
            items += [(x, y, sp) for sp in range(S)]
        t0 += n
    return S, items


def piece_stages(Npad, S, piece):
    """gram_sia_body.h 48-52 and 192: the stages of K piece `piece` of S over [0, Npad)."""
    L = (Npad + S * GBK - 1) // (S * GBK) * GBK
    k0 = piece * L
    k1 = min(k0 + L, Npad)
    return max(k1 - k0, 0) // GBK, L // GBK


def gram_items(m, N, tall, sched, pair=True):
    """The items of one main-Gram launch as dicts: nk; k = 'whole' | 'piece' | 'last' (a piece shorter
    than L, the empty ones included); kind = 'pair' | 'UD1' | 'D0L' | 'off' (256 x 128) or 'diag' |
    'off' (128 x 128); av = whether an AV launch gives the item the fused Aᵀv (gram_item_designated)."""
    mpad, Npad = round_up(m, 128), max(round_up(max(N, 1), 16), 16)
    nb = mpad // 128
    assert not tall or nb % 2 == 0
    tiles = tile_list_tall(nb, pair) if tall else tile_list_128(nb)
    if sched:
        S, work = schedule(tiles, 32 if tall else 64)
    else:
        S, work = 1, [(x, y, -1) for x, y in tiles]
    out = []
    for x, y, p in work:
        if p < 0:
            nk, k = Npad // GBK, "whole"
        else:
            nk, full = piece_stages(Npad, S, p)
            k = "piece" if nk == full else "last"
        if tall:
            kind = "pair" if y < 0 else "UD1" if y == 2 * x + 1 else "D0L" if y == 2 * x else "off"
            av = y < 0 or y // 2 == x
        else:
            kind = "diag" if x == y else "off"
            av = x == y
        out.append(dict(nk=nk, k=k, kind=kind, av=av, S=S))
    return out


def nk_class(nk):
    return str(nk) if nk < 4 else ">=4"


NK_CLASSES = ("0", "1", "2", "3", ">=4")


def census():
    """{(row, nk class): sorted cases reaching it} over the Gram grid (both schedules, N of GRAM_N)
    and, for the AV rows, the fused grid (FUSED_N).  Rows: 'whole 128', 'whole 256', 'piece 128',
    'piece 256' (short last pieces included), 'last piece *', 'AV 128', 'AV 256', and per item kind
    ('pair 256', 'UD1 256' = [U; D1], 'D0L 256' = [D0; L], 'off *', 'diag 128')."""
    table = {}

    def put(row, nk, case):
        table.setdefault((row, nk_class(nk)), set()).add(case)

    for tall in (False, True):
        sz = "256" if tall else "128"
        for m in GRAM_M[tall]:
            for sched in (True, False):
                for N in sorted(set(GRAM_N) | set(FUSED_N)):
                    case = f"m={m} N={N} sched={int(sched)}"
                    for it in gram_items(m, N, tall, sched):
                        if N in GRAM_N:
                            put(("whole " if it["k"] == "whole" else "piece ") + sz, it["nk"], case)
                            if it["k"] == "last":
                                put("last piece " + sz, it["nk"], case)
                            put(f"{it['kind']} {sz}", it["nk"], case)
                        if N in FUSED_N and it["av"]:
                            put("AV " + sz, it["nk"], case)
    return {k: sorted(v) for k, v in table.items()}


REQUIRED = {"whole 128": NK_CLASSES[1:], "whole 256": NK_CLASSES[1:], "piece 128": NK_CLASSES,
            "piece 256": NK_CLASSES, "pair 256": NK_CLASSES, "AV 128": NK_CLASSES, "AV 256": NK_CLASSES}


def census_markdown():
    """The census as a Markdown table (profiles/exact_products/README.md prints it)."""
    t = census()
    rows = sorted({r for r, _ in t})
    lines = ["| items | " + " | ".join(f"nk {c}" for c in NK_CLASSES) + " |", "|---|" + "---|" * len(NK_CLASSES)]
    for r in rows:
        cells = []
        for c in NK_CLASSES:
            cases = t.get((r, c), [])
            cells.append("–" if not cases else f"{len(cases)} cases, e.g. {cases[0]}")
        lines.append(f"| {r} | " + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(census_markdown())
