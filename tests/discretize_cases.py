"""The cases of the discretisation kernel's exact tests (csrc/discretize.hip): inputs from seeds, exact cases written out, the
fixture tests/golden/g24_discretize.npz (tests/golden/make_golden_discretize.py) loaded by `load_fixture`.

ne = n + m + 1 is the order of the augmented matrix of zoh, NP = 16 ceil(ne / 16) its padded order.  "FEM" is the suite's
second-order model [[-D, -K], [I, 0]], K = Q diag(logspace(0, dec)) Q^T, D = 0.02 K + 0.5 I.  Every shape is the smallest that
reaches what it is listed for.

Constants of the device bounds (tests/test_discretize_exact_gpu.py), from the CPU measurement of tests/test_discretize_reference_cpu.py
(`pytest -s tests/test_discretize_reference_cpu.py -k yardstick` prints them), never from the kernel's own error:

  zoh:  max |err| <= C_Z ne 2^s 2^-53 max |expected| over the three outputs, s from the fixture.
        Ratio err / (ne 2^s 2^-53 max |expected|) of the float64 restatement of Higham's Alg. 2.3 (discretize_reference.expm_pade13)
        over the committed zoh cases: 0.035 .. 0.45 (z_one 0.45: one unit in the last place of a 3 x 3 result; z_unstable 0.31,
        z_mixed_batch 0.05 .. 0.18, z_threshold 0.08 .. 0.15, z_zero_A 0.11, z_nilpotent 0.09, z_rotation 0.08, z_stiff 0.04; the
        FEM cases of order 16 .. 66 0.035 .. 0.14).  scipy.linalg.expm: 0.004 .. 0.25 on those, 0.93 on z_unstable, 2.3 on
        z_rotation.
        C_Z = min(1, 4 x 0.45 rounded up to a power of two) = 1: the rule's cap holds (the factor four: the kernel's MFMA
        accumulation order and its own Gauss-Jordan solve in place of LAPACK's).
  be / bil:  max |err| <= 16 max(e_np, n 2^-53) max |expected|, e_np = E_NP[key]: the measured error of np.linalg.solve on the same
        case relative to max |expected|, rounded up to two digits (the factor 16: Gauss-Jordan lacks LU's backward stability)."""
import os
from fractions import Fraction

import numpy as np

import discretize_reference as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g24_discretize.npz')
CODE = {'fe': 0, 'be': 1, 'bil': 2, 'zoh': 3}
U = 2.0 ** -53

C_Z = 1.0
E_NP = {                      # measured by test_yardsticks_be_bil, rounded up
    'b_fem[12,3]/be': 2.1e-15, 'b_fem[12,3]/bil': 9.9e-16, 'b_fem[28,3]/be': 3.0e-15, 'b_fem[28,3]/bil': 1.2e-15,
    'b_far_pivot/be': 3.4e-16, 'b_far_pivot/bil': 3.4e-16,
}                             # (cond_inf of I - c A: 4e4 / 3e4, 8e4 / 6e4, 1.5 / 1.5; n 2^-53 = 1.3e-15, 3.1e-15, 7.8e-15)


def ne_np(n, m):
    ne = n + m + 1
    return ne, (ne + 15) // 16 * 16


# --------------------------------------------------------------------------------------------------------------- models
def fem(n, m, dec, seed):
    """One FEM-like model (n even): A (n x n), B (n x m; no input on the position rows), d (n)."""
    rng = np.random.default_rng(seed)
    h = n // 2
    Q, _ = np.linalg.qr(rng.standard_normal((h, h)))
    K = Q @ np.diag(np.logspace(0, dec, h)) @ Q.T
    D = 0.02 * K + 0.5 * np.eye(h)
    A = np.zeros((n, n))
    A[:h, :h], A[:h, h:], A[h:, :h] = -D, -K, np.eye(h)
    B = rng.standard_normal((n, m))
    B[h:] = 0.0
    return A, B, rng.standard_normal(n)


def _norm_at_unit_step(A, B, d):
    return dr.norm1(dr.augmented(A, B, d, 1.0))


def soft_model():
    """z_threshold's fixed model: n = 12, m = 3, a FEM model over half a decade."""
    return fem(12, 3, 0.5, 4100)


THRESHOLD_TARGETS = (0.99 * dr.THETA_13, 1.01 * dr.THETA_13, 0.99 * 2 * dr.THETA_13, 1.01 * 2 * dr.THETA_13)
THRESHOLD_S = (0, 1, 1, 2)
MIXED_S = (0, 1, 4, 9, 10, 0)
MIXED_DT = 0.05


def threshold_steps():
    """The four dt at which |M|_1 is 1 % below / above theta_13 and 2 theta_13 (never at a threshold: the device sums the norm in
    its own order)."""
    nrm = _norm_at_unit_step(*soft_model())
    return [t / nrm for t in THRESHOLD_TARGETS]


def mixed_batch():
    """n = 14, m = 2, batch 6: one FEM model scaled so that |M|_1 = theta_13 2^(s - 1/2) for s = 1, 4, 9, 10 (the middle of each
    interval of the rule) and 0.5 theta_13, 0.1 theta_13 for the two members with s = 0."""
    A, B, d = fem(14, 2, 3.0, 4200)
    nrm = _norm_at_unit_step(A, B, d) * MIXED_DT
    target = [0.5 * dr.THETA_13 if s == 0 else dr.THETA_13 * 2.0 ** (s - 0.5) for s in MIXED_S]
    target[-1] = 0.1 * dr.THETA_13
    f = np.array(target) / nrm
    return f[:, None, None] * A[None], f[:, None, None] * B[None], f[:, None] * d[None]


def nilpotent():
    """n = 10, m = 2: A strictly upper triangular, A, B, d small integers; with dt = 2^-2 the augmented matrix is strictly upper
    triangular with dyadic entries, M^13 = 0."""
    rng = np.random.default_rng(4300)
    A = np.triu(rng.integers(-3, 4, (10, 10)).astype(np.float64), 1)
    return A, rng.integers(-3, 4, (10, 2)).astype(np.float64), rng.integers(-3, 4, 10).astype(np.float64)


NILPOTENT_DT = 0.25
ROTATION_DT = 0.25
ROTATION_ANGLES = (0.3, 1.7, 5.5, 11.0, 23.5, 40.0)        # w dt of the six blocks; w = 4 angle, so w dt is exact


def rotation():
    """n = 12, m = 1: six undamped blocks [[0, w], [-w, 0]] (a normal matrix)."""
    rng = np.random.default_rng(4400)
    A = np.zeros((12, 12))
    for k, th in enumerate(ROTATION_ANGLES):
        w = 4.0 * th
        A[2 * k, 2 * k + 1], A[2 * k + 1, 2 * k] = w, -w
    return A, rng.integers(-8, 9, (12, 1)).astype(np.float64) / 4.0, rng.integers(-8, 9, 12).astype(np.float64) / 4.0


def rotation_closed_form():
    """exp(A t) = [[c, s], [-s, c]], int_0^t exp(A tau) dtau = [[s, 1 - c], [-(1 - c), s]] / w per block, in long double
    (1 - c = 2 sin^2(w t / 2)), rounded to float64."""
    A, B, d = rotation()
    L = np.longdouble
    Ad = np.zeros((12, 12), dtype=L)
    G = np.zeros((12, 12), dtype=L)
    for k, th in enumerate(ROTATION_ANGLES):
        th, w = L(th), L(4.0 * th)
        c, s, omc = np.cos(th), np.sin(th), 2 * np.sin(th / 2) ** 2
        i = 2 * k
        Ad[i, i], Ad[i, i + 1], Ad[i + 1, i], Ad[i + 1, i + 1] = c, s, -s, c
        G[i, i], G[i, i + 1], G[i + 1, i], G[i + 1, i + 1] = s / w, omc / w, -omc / w, s / w
    return Ad.astype(np.float64), (G @ B.astype(L)).astype(np.float64), (G @ d.astype(L)).astype(np.float64)


def unstable():
    """n = 8, m = 2, dt = 0.05: eigenvalues -2 / dt .. +8 / dt, mildly non-normal (entries of exp grow to e^8)."""
    rng = np.random.default_rng(4500)
    S = np.eye(8) + 0.2 * rng.standard_normal((8, 8))
    A = S @ np.diag(np.linspace(-2.0, 8.0, 8) / 0.05) @ np.linalg.inv(S)
    return A, rng.standard_normal((8, 2)), rng.standard_normal(8)


def stiff():
    """The stiff model of tests/test_tpwl_gpu.py::test_device_discretisation_edge_shapes (same seed, same draws)."""
    rng = np.random.default_rng(9)
    n, m = 12, 2
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = Q @ np.diag(-np.logspace(0, 7, n)) @ Q.T
    return A, rng.standard_normal((n, m)), rng.standard_normal(n)


# ----------------------------------------------------------------------------------------------------- be / bil, exact
DYADIC_DT = 0.125


def dyadic(method, shifted):
    """n = 8, m = 2: I - c A = P T with T unit upper triangular with entries in -2 .. 2 and P the identity (no swap in any column)
    or the cyclic shift that puts row i + 1 of T into row i (a swap in every column but the last, which has no row left to swap
    with).  c = dt (be) or dt / 2 (bil) is a power of two, B and d are integers: every number of the elimination is a small dyadic
    rational and every operation exact."""
    rng = np.random.default_rng(4600)
    n, m = 8, 2
    T = np.triu(rng.integers(-2, 3, (n, n)).astype(np.float64), 1) + np.eye(n)
    PT = np.roll(T, -1, axis=0) if shifted else T
    c = DYADIC_DT if method == 'be' else DYADIC_DT / 2
    A = (np.eye(n) - PT) / c
    return A, rng.integers(-4, 5, (n, m)).astype(np.float64), rng.integers(-4, 5, n).astype(np.float64)


def dyadic_expected(method, shifted):
    """The exact result (Fractions) as float64 arrays, and the pivot rows; every entry converts without rounding (asserted)."""
    A, B, d = dyadic(method, shifted)
    Ad, Bd, dd, piv = dr.eliminate(A, B, d, DYADIC_DT, method, number=Fraction)
    out = []
    for X in (Ad, Bd, dd):
        F = np.array(X, dtype=np.float64)
        assert all(Fraction(float(f)) == x for f, x in zip(F.ravel(), X.ravel()))
        out.append(F)
    return out[0], out[1], out[2], piv


FAR_PIVOT_DT = 0.05
FAR_PIVOT_ROWS = {0: 69, 3: 68}             # column -> row of its pivot; every other column pivots on its diagonal


def far_pivot(method):
    """n = 70, m = 1: I - c A = W (c = dt for be, dt / 2 for bil), a diagonally dominant matrix (diagonal 4 .. 6, off-diagonal
    ~1e-4) with rows 0 <-> 69 and 3 <-> 68 exchanged: the pivot of column 0 is found in row 69 = 0 + 5 + 64 and that of column 3 in
    row 68 = 3 + 1 + 64, both in the second pass of the lane-strided search; a search of the first pass alone finds ~3e-4 there."""
    rng = np.random.default_rng(4700)
    n = 70
    W = 1e-4 * rng.standard_normal((n, n))
    W[np.arange(n), np.arange(n)] = rng.uniform(4.0, 6.0, n)
    for a, b in ((0, 69), (3, 68)):
        W[[a, b]] = W[[b, a]]
    A = (np.eye(n) - W) / (FAR_PIVOT_DT if method == 'be' else FAR_PIVOT_DT / 2)
    return A, rng.standard_normal((n, 1)), rng.standard_normal(n)


def singular_batch(method):
    """n = 4, m = 2, batch 4 at dt = 0.5: members 1 and 3 have I - c A = 0."""
    rng = np.random.default_rng(4800)
    A = 0.3 * rng.standard_normal((4, 4, 4))
    A[1] = A[3] = (2.0 if method == 'be' else 4.0) * np.eye(4)
    return A, rng.standard_normal((4, 4, 2)), rng.standard_normal((4, 4))


SINGULAR_DT = 0.5


def small(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)), rng.standard_normal((n, m)), rng.standard_normal(n)


NONFINITE_DT = 0.05
NONFINITE_PLACES = ('nan_A', 'inf_A', 'nan_d', 'nan_B')


def nonfinite_batch(place):
    """n = 6, m = 2, batch 3: three ordinary models, member 1 with one non-finite entry."""
    rng = np.random.default_rng(4900)
    A, B, d = rng.standard_normal((3, 6, 6)), rng.standard_normal((3, 6, 2)), rng.standard_normal((3, 6))
    if place == 'nan_A':
        A[1, 2, 4] = np.nan
    elif place == 'inf_A':
        A[1, 5, 0] = -np.inf
    elif place == 'nan_d':
        d[1, 3] = np.nan
    elif place == 'nan_B':
        B[1, 5, 1] = np.nan
    else:
        raise ValueError(place)
    return A, B, d


# ------------------------------------------------------------------------------------------------------ the LDS limit
LDS_MAX = 160 * 1024


def lds_bytes(n, m, method):
    """discretize_lds of csrc/discretize.hip restated: the tableau (rows x ld, ld = cols | 1), the reduction scratch, 64 bytes of
    integers.  srh::lds_request rounds it up to a multiple of 2560 but never above 160 KB unless the request itself is: a model is
    accepted exactly when this number is <= 163840."""
    if method in ('be', 'bil'):
        cols = 2 * n + m + 1
        return 8 * (n * (cols | 1) + 8 + n) + 64
    ne, NP = ne_np(n, m)
    return 8 * (ne * ((2 * ne) | 1) + 8 + NP + 8) + 64


# With m = 1.  be / bil: 8 (n (2 n + 3) + 8 + n) + 64 = 16 (n + 1)^2 + 112 <= 163840  <=>  n + 1 <= 101.1:  n = 100 uses 163328
# bytes, n = 101 would need 166576.  zoh (ne = n + 2, NP = 112 for ne = 97 .. 112): 8 (ne (2 ne + 1) + 128) + 64 <= 163840  <=>
# ne (2 ne + 1) <= 20344:  ne = 100 (n = 98) uses 161888 bytes, ne = 101 (n = 99) would need 165112.
LDS_LIMIT = {'be': (100, 101), 'bil': (100, 101), 'zoh': (98, 99)}
LDS_DT = 0.05


def lds_model(n):
    """A well-conditioned dense model for the addressing run at the limit: |A| dt ~ 1, m = 1."""
    rng = np.random.default_rng(5000 + n)
    A = rng.standard_normal((n, n)) / np.sqrt(n) * 4.0 - 3.0 * np.eye(n)
    return A, rng.standard_normal((n, 1)), rng.standard_normal(n)


# ------------------------------------------------------------------------------------------- the fixture-backed cases
def _one(A, B, d):
    return A[None], B[None], d[None]


def fixture_cases():
    """[(key, method, dt, A, B, d)] with A (batch x n x n), B (batch x n x m), d (batch x n): every case whose expected value is in
    the fixture, in the fixture's order."""
    out = []
    out.append(('z_one', 'zoh', 0.1, np.array([[[-3.0]]]), np.array([[[2.0]]]), np.array([[0.5]])))
    out.append(('z_full_tile', 'zoh', 0.05) + _one(*fem(12, 3, 4.5, 4001)))
    out.append(('z_tile_plus_one@dt', 'zoh', 0.05) + _one(*fem(14, 2, 4.5, 4002)))
    out.append(('z_tile_plus_one@2dt', 'zoh', 0.1) + _one(*fem(14, 2, 4.5, 4002)))
    out.append(('z_two_tiles[28,3]', 'zoh', 0.05) + _one(*fem(28, 3, 4.5, 4003)))
    out.append(('z_two_tiles[30,2]', 'zoh', 0.05) + _one(*fem(30, 2, 4.5, 4004)))
    out.append(('z_wide', 'zoh', 0.05) + _one(*fem(64, 1, 3.0, 4005)))
    for k, dt in enumerate(threshold_steps()):
        out.append(('z_threshold[%d]' % k, 'zoh', dt) + _one(*soft_model()))
    rng = np.random.default_rng(4006)
    out.append(('z_zero_A', 'zoh', 0.05, np.zeros((1, 6, 6)), rng.standard_normal((1, 6, 2)), rng.standard_normal((1, 6))))
    out.append(('z_nilpotent', 'zoh', NILPOTENT_DT) + _one(*nilpotent()))
    out.append(('z_rotation', 'zoh', ROTATION_DT) + _one(*rotation()))
    out.append(('z_unstable', 'zoh', 0.05) + _one(*unstable()))
    out.append(('z_stiff', 'zoh', 0.05) + _one(*stiff()))
    out.append(('z_mixed_batch', 'zoh', MIXED_DT) + mixed_batch())
    for n in (12, 28):
        for method in ('be', 'bil'):
            out.append(('b_fem[%d,3]/%s' % (n, method), method, 0.05) + _one(*fem(n, 3, 4.5, 4010 + n)))
    for method in ('be', 'bil'):
        out.append(('b_far_pivot/%s' % method, method, FAR_PIVOT_DT) + _one(*far_pivot(method)))
    out.append(('f_small', 'fe', 0.05) + _one(*small(5, 2, 4020)))
    return out


REGENERATED = ('z_one', 'z_zero_A', 'z_nilpotent', 'b_fem[12,3]/be', 'b_fem[12,3]/bil')     # by the CPU test, under mpmath


def case(key):
    for c in fixture_cases():
        if c[0] == key:
            return c
    raise KeyError(key)


def fem_batch3(n, method):
    """b_fem's model and two more from the next seeds: the batch of the independence check (member 0 is the fixture's case)."""
    ms = [fem(n, 3, 4.5, 4010 + n + 100 * k) for k in range(3)]
    return tuple(np.stack([x[i] for x in ms]) for i in range(3))


_fixture = None


def load_fixture():
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def expected(key):
    """(A_d, B_d, d_d) of the fixture, with the batch dimension."""
    g = load_fixture()
    return g[key + '/Ad'], g[key + '/Bd'], g[key + '/dd']


def zoh_bound(key, n, m, member=0):
    """C_Z ne 2^s 2^-53 max |expected| over the three outputs of one member, s from the fixture."""
    g = load_fixture()
    ne, _ = ne_np(n, m)
    big = max(float(np.abs(g[key + '/' + o][member]).max()) for o in ('Ad', 'Bd', 'dd'))
    return C_Z * ne * 2.0 ** int(g[key + '/s'][member]) * U * big


def solve_bound(key, n):
    g = load_fixture()
    big = max(float(np.abs(g[key + '/' + o][0]).max()) for o in ('Ad', 'Bd', 'dd'))
    return 16.0 * max(E_NP[key], n * U) * big


def fe_diagonal_exact(dt, a):
    """1 + dt a, exactly."""
    return 1 + Fraction(float(dt)) * Fraction(float(a))


def fe_diagonal_ok(got, dt, a):
    """|got - (1 + dt a)| <= 2^-53 (|dt a| + |1 + dt a|), in exact rational arithmetic against the unrounded value: float64's product
    and sum lose that much at the most, an fma half of it.  (Against the fixture's rounded value the same bound would allow no
    difference at all wherever |1 + dt a| >= 1 -- differences there are multiples of 2^-52 -- and one rounding of dt a can move
    the sum to the neighbouring number.)"""
    x = fe_diagonal_exact(dt, a)
    return abs(Fraction(float(got)) - x) <= Fraction(1, 2 ** 53) * (abs(x - 1) + abs(x))


def max_err(got, exp):
    """The largest absolute error over the three outputs of one member."""
    return max(float(np.abs(a - b).max()) for a, b in zip(got, exp))
