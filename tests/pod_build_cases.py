"""Seeded inputs and case lists shared by tests/test_pod_build_reference_cpu.py (which checks the references and the input
conditions without a GPU) and tests/test_pod_build_exact_gpu.py (which runs the kernels of the POD build chain on them:
csrc/gramian.hip, csrc/abt_dev.h behind csrc/snapshots.hip, csrc/eigh.hip's mode selection, csrc/eigh_topk.hip).

Integer data: entries drawn from {-8..8}, stored as float64 (tests/pod_build_reference.py says why the comparison is then exact).
Errors are made visible where kernels lose them: the LAST COLUMN (the ragged end of the K loop) and the LAST ROW (the ragged end of
the last 128-row tile) hold entries of magnitude 8, and no two rows are equal wherever the shape has room for that (n_f >= 4), so a
tile or slot decoded to the wrong place cannot land on equal data.

Real data: standard normal entries, the columns scaled over six decades."""
import numpy as np

TB, KC = 128, 16                    # tile edge and K chunk of gramian.hip / abt_dev.h

# ------------------------------------------------------------------------------------------------------------- data
_INT = {}


def int_matrix(rows, cols, seed):
    """(rows x cols) integer-valued float64 matrix (cached; treat as read-only)."""
    key = (rows, cols, seed)
    if key not in _INT:
        rng = np.random.default_rng([rows, cols, seed])
        M = rng.integers(-8, 9, (rows, cols)).astype(np.float64)
        M[:, -1] = 8.0 * rng.choice([-1.0, 1.0], rows)
        M[-1, :] = 8.0 * rng.choice([-1.0, 1.0], cols)
        if cols >= 4:
            for _ in range(100):             # re-draw the interior of repeated rows
                _, first, counts = np.unique(M, axis=0, return_index=True, return_counts=True)
                if counts.max() == 1:
                    break
                dup = np.setdiff1d(np.arange(rows), first)
                if rows - 1 in dup:          # the last row keeps its magnitude 8: re-draw its earlier twins instead
                    twins = np.flatnonzero((M[:-1] == M[-1]).all(axis=1))
                    dup = np.union1d(np.setdiff1d(dup, [rows - 1]), twins)
                M[dup, :-1] = rng.integers(-8, 9, (len(dup), cols - 1))
            assert len(np.unique(M, axis=0)) == rows
        M.setflags(write=False)
        _INT[key] = M
    return _INT[key]


def real_matrix(rows, cols, seed):
    rng = np.random.default_rng([rows, cols, seed, 1])
    return rng.standard_normal((rows, cols)) * 10.0 ** rng.uniform(-3.0, 3.0, cols)


def pitched(M, ld):
    """M in a buffer of row pitch ld, the padding filled with NaN (a loader that ignores the pitch, or reads past n_f, shows)."""
    out = np.full((M.shape[0], ld), np.nan)
    out[:, :M.shape[1]] = M
    return out


# -------------------------------------------------------------------------------------------------------- Gramian
# (n_s, n_f, lds): the whole-tile path
GRAMIAN_WHOLE = [(1, 1, 1), (5, 15, 15), (127, 16, 16), (128, 17, 17), (129, 130, 137), (300, 1000, 1003)]
# the tail path: n_s = 128 ntile - 126 (a ragged last tile), 67 chunks (a part that starts at an odd chunk, a ragged last chunk)
TAIL_N_F = 1062
TAIL_PAD = 5


def tail_n_s(ntile):
    return TB * ntile - 126


def plan_model(n_s, n_f, cus):
    """The rule of srom_gramian_dev restated: (ntile, nfull, ntail, ksplit)."""
    slots = 2 * cus
    ntile = -(-n_s // TB)
    nblk = ntile * (ntile + 1) // 2
    nchunk = -(-n_f // KC)
    rem = nblk % slots
    if nblk > slots and rem > 0 and 2 * rem <= slots and nchunk >= 64:
        return ntile, nblk - rem, rem, min(8, slots // rem)
    return ntile, nblk, 0, 1


def tail_ntiles(plan):
    """Smallest ntile whose launch has a tail split 8 ways, and smallest with a tail split k ways, 1 < k < 8; plan(n_s, n_f) returns a
    dict with 'ntail' and 'ksplit'.  (None where the search to ntile = 200 finds nothing.)"""
    cap = mid = None
    for ntile in range(2, 201):
        p = plan(tail_n_s(ntile), TAIL_N_F)
        if p['ntail'] > 0 and p['ksplit'] == 8 and cap is None:
            cap = ntile
        if p['ntail'] > 0 and 1 < p['ksplit'] < 8 and mid is None:
            mid = ntile
        if cap is not None and mid is not None:
            break
    return cap, mid


# ---------------------------------------------------------------------------------------------------------- modes
# (k, n_s, n_f, lds): every k of {1, 15, 16, 17, 48, 63, 64}, n_s of {1, 63, 64, 65, 200} and n_f of {1, 63, 64, 65, 333} appears,
# each k-group boundary (16 columns per wave) with a ragged and a whole 64-row slab of S and a ragged and a whole 64-column block
MODES = [(1, 1, 1, 1), (15, 63, 63, 63), (16, 64, 64, 64), (17, 65, 65, 65), (48, 200, 333, 333), (63, 65, 333, 333),
         (64, 200, 65, 65), (64, 64, 1, 1), (1, 200, 333, 333), (17, 1, 64, 64), (63, 63, 64, 64), (16, 65, 63, 63),
         (48, 64, 65, 65), (15, 200, 1, 1), (64, 1, 63, 63),
         (17, 65, 65, 70), (64, 200, 333, 340), (1, 63, 1, 3)]                    # pitched S

# ------------------------------------------------------------------------------------------ squared distances (abt_dev.h)
# (n_s, nc, n_f, lds): n_f = 1 .. 130 -> one K part, 1062 -> 8 parts, 8200 -> the cap of 64; nc = 129 -> two tiles along N
SQDIST = [(1, 1, 1, 1), (127, 5, 15, 15), (129, 129, 17, 17), (300, 5, 130, 130), (1, 129, 130, 130), (129, 5, 1062, 1062),
          (300, 129, 1062, 1062), (127, 1, 8200, 8200), (300, 129, 8200, 8200), (300, 1, 1, 1), (127, 129, 15, 15),
          (129, 5, 1062, 1069), (300, 129, 8200, 8203), (127, 5, 17, 18)]         # pitched S
SQDIST_REAL = (300, 129, 1062, 1069)


def abt_ksplit(M, N, K, cus=256):
    """The split of abt_dev.h's Abt::run restated."""
    tiles = (-(-M // TB)) * (-(-N // TB))
    nchunk = -(-K // KC)
    return max(1, min((2 * cus + tiles - 1) // tiles, max(nchunk // 8, 1), 64))


# ------------------------------------------------------------------------------------------------- mode selection
def select_cases():
    out = []
    for n in (1, 5, 257):
        for k in sorted({1, n, min(n, 64)}):
            out.append((n, k))
    return out


def select_inputs(n, seed=0):
    """Synthetic (V, w): rows of V play the eigenvectors, w ascending and positive over eight decades."""
    rng = np.random.default_rng([n, seed, 2])
    V = rng.standard_normal((n, n))
    w = np.sort(10.0 ** rng.uniform(-4.0, 4.0, n))
    return V, w


# ------------------------------------------------------------------------------------------------------ rank edge
RANK_N, RANK, RANK_K, RANK_NF = 40, 3, 6, 90


def rank_snapshots():
    """S (40 x 90, one snapshot per row) of rank exactly 3: integer coefficients times three integer rows, so S and G = S S^T are
    exact.  The three rows are scaled 8 : 3 : 1 to separate the singular values."""
    rng = np.random.default_rng(40)
    Cf = rng.integers(-4, 5, (RANK_N, RANK)).astype(np.float64)
    B = rng.integers(-8, 9, (RANK, RANK_NF)).astype(np.float64) * np.array([[8.0], [3.0], [1.0]])
    return Cf @ B


# ------------------------------------------------------------------------------------------- leading eigenpairs, edges
# (n, k, oversample): block b = min(n, ceil16(k + oversample)), oversample -1 -> max(16, k / 2)
TOPK = [(5, 2, -1), (20, 4, -1), (40, 1, 0), (300, 16, 0), (400, 100, 28)]
TOPK_REFUSED = (400, 100, 29)


def topk_block(n, k, oversample):
    if oversample < 0:
        oversample = max(16, k // 2)
    return min(n, (k + oversample + 15) & ~15)


def topk_matrix(n, k, oversample):
    """G = Q diag(lam) Q^T, symmetric bit for bit: lam falls from 5 to 1 over the block and drops by 1e6 behind it.  The gap is set by
    the residual check, not by the eigenvalues: the solver stops when the leading eigenvalues move by less than 1e-13 w_0, which
    bounds the angle of the k-th vector by sqrt(1e-13) only, while |G v - w v| <= 1e-9 w_0 needs 1e-9; with a ratio rho behind
    the block the angle falls by rho per iteration and the eigenvalue by rho^2, so the last iteration that still moved an eigenvalue
    by 1e-13 leaves an angle of at most rho sqrt(1e-13) -- rho = 1e-6 gives 3e-13 (rho = 1e-1 would leave 3e-8)."""
    rng = np.random.default_rng([n, k, 3])
    b = topk_block(n, k, oversample)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate((np.linspace(5.0, 1.0, b), 1e-6 * rng.uniform(0.5, 1.0, n - b)))
    G = (Q * lam) @ Q.T
    return 0.5 * (G + G.T), lam


def flat_matrix():
    """n = 200, lam_i = 1 - 1e-4 i: no gap anywhere -- a block of 32 cannot settle in 30 iterations."""
    n = 200
    rng = np.random.default_rng(200)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = 1.0 - 1e-4 * np.arange(n)
    G = (Q * lam) @ Q.T
    return 0.5 * (G + G.T), lam
