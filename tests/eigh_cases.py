"""Matrices and the case table shared by tests/test_eigh_reference_cpu.py (which checks the construction, the references and the
bounds without a GPU) and tests/test_eigh_exact_gpu.py (which runs srom_eigh_dev of csrc/eigh.hip on them, path by path).

Exact-spectrum matrices.  G = Q D Q with Q = I - 2 v v^T / s a Householder reflector, v an integer vector without a zero entry
and s = v^T v.  The integer matrix

    s^2 G = s^2 D - 2 s (v v^T D + D v v^T) + 4 (v^T D v) v v^T

is built in int64.  Where s is a power of two the division by s^2 is exact: the stored doubles have exactly the spectrum D and
the eigenvectors s Q / s.  `householder_vector` starts from all ones and raises entries to 2 (adds 3 to s) or 3 (adds 8) until s is a
power of two.  No such vector exists for n = 3 (a power of two is never a sum of three non-zero squares: all three would be even,
and dividing by 4 descends to 1 or 2), nor with entries up to 3 for a few other small n; there v is all ones, s = n, and the
INTEGER matrix s^2 G itself is the case: spectrum s^2 D, the same eigenvectors.  Either way every entry is an integer multiple of
a power of two below 2^53 -- exact -- and rows and columns are permuted symmetrically with a fixed seed so that equal eigenvalues
do not sit in index order.

Structured inputs are built directly (an unsorted diagonal with ties, zero, identity, and an integer Gramian with one all-zero
snapshot and two identical ones, after pod_build_cases.rank_snapshots).  Real spectra: the graded random Gramian of
tests/test_edge_cases_gpu.py::test_device_eigh (grading 1e-3) of a snapshot matrix rounded to 2^-13, and its exact multiples by
2^100 and 2^-100.  The eigenvalues of the real spectra (the graded and the integer Gramians) by tests/eigh_reference.jacobi are
kept in tests/golden/eigh_reference_w.npz as pairs of doubles (hi, lo): `python tests/eigh_cases.py` writes the file, the CPU test
recomputes every entry, the GPU test reads it.

Nothing here imports the package."""
import os

import numpy as np

# ---------------------------------------------------------------------------------------------------- dispatch, restated
JAC_MAX, JAC_BLOCK_MIN = 128, 256          # csrc/eigh.hip: LDS kernel up to 128, scalar grid form up to 256 by default


def ne_scalar(n):
    """Padded size of the LDS and grid kernels: the next even number."""
    return (n + 1) & ~1


def ne_block(n, P):
    """(padded size, number of blocks of P / 2, number of pair problems per step) of jacobi_block_p<P>."""
    ne = (n + P - 1) // P * P
    nb = ne // (P // 2)
    return ne, nb, nb // 2


def default_solver(n):
    """Which solver the size dispatch picks with no switch set (n <= 4096)."""
    return 'lds' if n <= JAC_MAX else ('grid' if n <= JAC_BLOCK_MIN else 'block64')


# --------------------------------------------------------------------------------------------------------------- bounds
# tests/test_edge_cases_gpu.py: test_device_eigh (LDS, grid) and test_device_eigh_block_jacobi (block); relative to max |w_ref|
TIGHT = dict(eig=1e-12, defect=1e-12, resid=1e-11)
BLOCK = dict(eig=1e-11, defect=2e-11, resid=1e-10)
# asserted tolerance of a cluster's projector (and of a simple eigenvector up to sign), max entry: the CPU test shows that the
# Davis-Kahan bound at the permitted residual and defect (eigh_reference.subspace_bound) stays below it for every cluster of every case
PROJ_TOL = dict(tight=1e-6, block=1e-5)

ENV_SWITCHES = ('SRH_EIGH_ROCSOLVER', 'SRH_EIGH_BLOCK', 'SRH_EIGH_BLOCK_PAIR', 'SRH_EIGH_BLOCK_SWITCH', 'SRH_EIGH_BLOCK_ORDER',
                'SRH_EIGH_BLOCK_INNER', 'SRH_EIGH_TRACE')

FULL = ('distinct', 'clusters', 'indefinite', 'rank3', 'rank10', 'scalar', 'diagonal', 'zero', 'identity', 'gramian', 'graded',
        'graded_up', 'graded_down')
KNOWN = FULL[:9]                          # the kinds whose answer is known exactly
EDGE = ('clusters', 'indefinite')

# name -> (solver, environment, bounds, {size: kinds}).  Every solver gets FULL at a size it pads and at one it does not; the other
# sizes of the table (the boundaries of the dispatch and of the padding) get EDGE.  The scalar grid form forced above 256 (padded at 257, not at
# 300) gets every kind whose answer is known exactly; its real spectra run at 255 and 256.
PATHS = {
    'lds': ('lds', {}, TIGHT, {1: EDGE, 2: EDGE, 3: EDGE, 63: EDGE, 64: EDGE, 65: EDGE, 127: FULL, 128: FULL}),
    'grid': ('grid', {}, TIGHT, {129: EDGE, 255: FULL, 256: FULL}),
    'grid_forced': ('grid', {'SRH_EIGH_BLOCK': '0'}, TIGHT, {257: KNOWN, 300: KNOWN}),
    'block64': ('block64', {'SRH_EIGH_BLOCK': '1'}, BLOCK, {129: EDGE, 191: FULL, 192: FULL, 193: EDGE}),
    'block64_default': ('block64', {}, BLOCK, {257: EDGE}),
    'block128': ('block128', {'SRH_EIGH_BLOCK': '1', 'SRH_EIGH_BLOCK_PAIR': '128'}, BLOCK,
                 {129: EDGE, 255: FULL, 256: FULL, 257: EDGE}),
}
# the switches of the block form, on the indefinite case at 193 (ne = 256: 63 padding positions that order 1 and 2 move about)
SWITCHES = [('order0', {'SRH_EIGH_BLOCK': '1', 'SRH_EIGH_BLOCK_ORDER': '0'}), ('order1', {'SRH_EIGH_BLOCK': '1', 'SRH_EIGH_BLOCK_ORDER': '1'}),
            ('inner2', {'SRH_EIGH_BLOCK': '1', 'SRH_EIGH_BLOCK_INNER': '2'})]
SWITCH_N, SWITCH_KIND = 193, 'indefinite'
# one repeat call per solver: (path, n, kind)
REPEAT = [('lds', 127, 'graded'), ('grid', 255, 'graded'), ('block64', 191, 'graded'), ('block128', 255, 'graded'),
          ('block64', 193, 'indefinite')]


def device_cases():
    """[(path, n, kind)] of the table above, in order."""
    return [(path, n, kind) for path, (_, _, _, sizes) in PATHS.items() for n, kinds in sizes.items() for kind in kinds]


def matrix_keys():
    """The distinct (kind, n) behind device_cases() and the switch cases."""
    keys = {(kind, n) for _, n, kind in device_cases()}
    keys.add((SWITCH_KIND, SWITCH_N))
    return sorted(keys, key=lambda kn: (kn[1], kn[0]))


# -------------------------------------------------------------------------------------------------------------- spectra
def spectrum(kind, n):
    """The integer vector D of an exact-spectrum kind."""
    if kind == 'distinct':
        return np.arange(1, n + 1, dtype=np.int64)
    if kind == 'clusters':                   # multiplicities about n / 3, 3 and 2, the rest distinct; smallest gap 1
        D = ([7] * (n // 3) + [3] * 3 + [1] * 2)[:n]
        return np.array(D + list(range(10, 10 + n - len(D))), dtype=np.int64)
    if kind == 'indefinite':                 # a zero eigenvalue of multiplicity >= 3 (from n = 5) between negative and positive ones
        z = 0 if n < 3 else min(3 + n // 16, n - 2)
        k = n - z
        return np.array([0] * z + [-i for i in range(1, k // 2 + 1)] + list(range(1, k - k // 2 + 1)), dtype=np.int64)
    if kind in ('rank3', 'rank10'):          # positive semidefinite of rank 3 / about n / 10
        r = 3 if kind == 'rank3' else max(4, n // 10)
        assert r < n
        return np.array([0] * (n - r) + [3 * i for i in range(1, r + 1)], dtype=np.int64)
    if kind == 'scalar':                     # D = c I: G = c I, diagonal
        return np.full(n, 5, dtype=np.int64)
    raise KeyError(kind)


EXACT_KINDS = ('distinct', 'clusters', 'indefinite', 'rank3', 'rank10', 'scalar')
DIAGONAL_KINDS = ('scalar', 'diagonal', 'zero', 'identity')          # G is diagonal: the answer is exact, bit for bit


def householder_vector(n):
    """(v, s): integer v without a zero entry, s = v.v a power of two where entries 1, 2, 3 reach one below 16 n; else ones, s = n."""
    s = 1
    while s < 16 * n:
        d = s - n
        if d >= 0:
            for b in range(d // 8 + 1):
                a, rem = divmod(d - 8 * b, 3)
                if rem == 0 and a + b <= n:
                    v = np.ones(n, dtype=np.int64)
                    v[:a] = 2
                    v[a:a + b] = 3
                    return v, s
        s *= 2
    return np.ones(n, dtype=np.int64), n


def exact_matrix(n, D, seed=0):
    """dict(G float64, N = scale_den * G in int64, den, lam (the spectrum of G, one per column of Qs), Qs = s Q int64, s) with rows
    and columns permuted.  den = s^2 and lam = D where s is a power of two, else den = 1 and lam = s^2 D."""
    D = np.asarray(D, dtype=np.int64)
    v, s = householder_vector(n)
    vDv = int((v * v * D).sum())
    N = s * s * np.diag(D) - 2 * s * (np.outer(v, v * D) + np.outer(D * v, v)) + 4 * vDv * np.outer(v, v)
    Qs = s * np.eye(n, dtype=np.int64) - 2 * np.outer(v, v)
    perm = np.random.default_rng([n, seed, 11]).permutation(n)
    N, Qs = N[perm][:, perm], Qs[perm]
    dyadic = s & (s - 1) == 0
    den = s * s if dyadic else 1
    G = N.astype(np.float64) / float(den)
    return dict(G=G, N=N, den=den, lam=D if dyadic else s * s * D, Qs=Qs, s=s)


# ------------------------------------------------------------------------------------------------------------ structured
def diagonal_values(n):
    """Unsorted small integers with ties (n >= 3: at least one tie; both signs and zero from n = 9 on)."""
    return np.random.default_rng([n, 12]).integers(-4, 5, n).astype(np.int64) if n > 2 else np.arange(n, 0, -1, dtype=np.int64)


def gramian_snapshots(n):
    """S (n x 2 n, one snapshot per row) of integer entries and rank at most r = max(2, n / 4): integer coefficients times r integer rows
    scaled 8 : 3 : 1 : 1 ... (pod_build_cases.rank_snapshots), snapshot 1 all zero and snapshots 2 and n - 1 identical.  S and
    G = S S^T are exact."""
    assert n >= 4
    r = max(2, n // 4)
    rng = np.random.default_rng([n, 13])
    Cf = rng.integers(-4, 5, (n, r))
    B = rng.integers(-8, 9, (r, 2 * n)) * np.array([8, 3] + [1] * (r - 2))[:, None]
    Cf[1] = 0
    Cf[n - 1] = Cf[2]
    return (Cf @ B).astype(np.int64)


GRADED_BITS = 13


def graded(n):
    """The family of test_device_eigh, S S^T of a random S (n x (n + 3)) whose columns fall over three decades, with S rounded to
    multiples of 2^-13: the integer product is exact in int64 (below 2^38), so G = (2^13 S)(2^13 S)^T / 2^26 is symmetric bit for bit
    and does not depend on the order in which a library sums it."""
    rng = np.random.default_rng([n, 14])
    S = np.rint(rng.standard_normal((n, n + 3)) * np.logspace(0, -3, n + 3) * 2.0 ** GRADED_BITS).astype(np.int64)
    return (S @ S.T).astype(np.float64) / 4.0 ** GRADED_BITS


UP, DOWN = 2.0 ** 100, 2.0 ** -100

_CASES = {}


def case(kind, n):
    """dict(G, lam, Qs, s, zero_rows, base): lam the exact spectrum in the order of the columns of Qs (None for a real spectrum), Qs / s
    the exact orthogonal eigenvector matrix (None where there is none to compare), zero_rows the number of exactly zero rows of G,
    base = (kind, factor) where G is factor times another case (an exact scaling).  Cached; treat as read-only."""
    key = (kind, n)
    if key in _CASES:
        return _CASES[key]
    c = dict(kind=kind, n=n, lam=None, Qs=None, s=1, zero_rows=0, base=None, N=None, den=1)
    if kind in EXACT_KINDS:
        c.update(exact_matrix(n, spectrum(kind, n)))
    elif kind in ('diagonal', 'zero', 'identity'):
        d = diagonal_values(n) if kind == 'diagonal' else np.full(n, 0 if kind == 'zero' else 1, dtype=np.int64)
        c.update(G=np.diag(d).astype(np.float64), lam=d, Qs=np.eye(n, dtype=np.int64), N=np.diag(d), den=1)
        c['zero_rows'] = int((d == 0).sum())
    elif kind == 'gramian':
        S = gramian_snapshots(n)
        N = S @ S.T
        c.update(G=N.astype(np.float64), N=N, zero_rows=1)
    elif kind == 'graded':
        c.update(G=graded(n))
    elif kind in ('graded_up', 'graded_down'):
        f = UP if kind == 'graded_up' else DOWN
        c.update(G=case('graded', n)['G'] * f, base=('graded', f))
    else:
        raise KeyError(kind)
    c['G'].setflags(write=False)
    _CASES[key] = c
    return c


# ------------------------------------------------------------------------------------------------ reference eigenvalues
REAL_KINDS = ('gramian', 'graded')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eigh_reference_w.npz')
_GOLDEN = {}


def real_keys():
    return [(kind, n) for kind, n in matrix_keys() if kind in REAL_KINDS]


def reference_w(kind, n):
    """Ascending long-double eigenvalues of a real-spectrum case from the golden file (a scaled case: those of its base, scaled)."""
    c = case(kind, n)
    if c['base'] is not None:
        return reference_w(c['base'][0], n) * np.longdouble(c['base'][1])
    if not _GOLDEN:
        with np.load(GOLDEN) as f:
            _GOLDEN.update({k: f[k] for k in f.files})
    hl = _GOLDEN['%s_%d' % (kind, n)]
    return hl[0].astype(np.longdouble) + hl[1].astype(np.longdouble)


def write_golden():
    import eigh_reference as er
    out = {}
    for kind, n in real_keys():
        w, _, sweeps = er.jacobi(case(kind, n)['G'])
        hi = w.astype(np.float64)
        out['%s_%d' % (kind, n)] = np.stack((hi, (w - hi.astype(np.longdouble)).astype(np.float64)))
        print('%s n %d: %d sweeps' % (kind, n, sweeps), flush=True)
    np.savez(GOLDEN, **out)


if __name__ == '__main__':
    write_golden()
