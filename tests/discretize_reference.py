"""The time discretisation of csrc/discretize.hip restated twice, importing nothing from the package or the oracle.

  mp_discretize      the statement itself in multiprecision arithmetic (mpmath, mp.dps = 60), rounded once to float64: what
                     tests/golden/g24_discretize.npz holds.  mpmath is needed only to regenerate that fixture.
  f64_discretize     float64 restatements used as yardsticks only: Higham 2005 ("The scaling and squaring method for the matrix
                     exponential revisited"), Alg. 2.3 with m = 13 always, in numpy (`@`, np.linalg.solve), and np.linalg.solve for
                     be / bil.  Their distance from the fixture is what a float64 code of this kind loses; the device bounds of
                     tests/test_discretize_exact_gpu.py are set from it (tests/discretize_cases.py, top).
  squarings          the published rule s = max(0, ceil(log2(|M|_1 / theta_13))).
  gauss_jordan       the elimination the kernel runs (partial pivoting on the first maximum, every other row reduced), generic over
                     float64 / fractions.Fraction, returning the pivot rows: for the exact cases and the path-coverage checks.

Why multiprecision and not long double: a Taylor scaling-and-squaring exponential in np.longdouble is only ~1e-15 from a 60-digit
result on the stiff FEM-like cases (s = 9: the squarings amplify its rounding), no better than the float64 codes under test."""
from fractions import Fraction

import numpy as np

THETA_13 = 5.371920351148152
METHODS = ('fe', 'be', 'bil', 'zoh')
DPS = 60
# Higham 2005, table of the [13/13] Pade coefficients b_0 .. b_13
PADE_13 = (64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0, 129060195264000.0, 10559470521600.0,
           670442572800.0, 33522128640.0, 1323241920.0, 40840800.0, 960960.0, 16380.0, 182.0, 1.0)


def augmented(A, B, d, dt):
    """[[A, B, d], [0, 0, 0]] dt in float64 (the products rounded, as any float64 code forms them)."""
    n, m = B.shape
    M = np.zeros((n + m + 1, n + m + 1))
    M[:n, :n], M[:n, n:n + m], M[:n, n + m] = A, B, d
    return M * dt


def norm1(M):
    return float(np.abs(M).sum(axis=0).max())


def squarings(M):
    nrm = norm1(M)
    return max(0, int(np.ceil(np.log2(nrm / THETA_13)))) if nrm > 0 else 0


# ------------------------------------------------------------------------------------------------------ multiprecision
def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _mp_matrix(mp, a):
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])          # a float64 converts exactly


def _mp_round(X, rows, cols):
    return np.array([[float(X[i, j]) for j in cols] for i in rows], dtype=np.float64)


def mp_discretize(A, B, d, dt, method):
    """(A_d, B_d, d_d) at 60 digits, rounded once to float64."""
    mp = _mp()
    n, m = B.shape
    dtm = mp.mpf(float(dt))
    if method == 'zoh':
        ne = n + m + 1
        M = mp.zeros(ne, ne)
        Am, Bm = _mp_matrix(mp, A), _mp_matrix(mp, B)
        for i in range(n):
            for j in range(n):
                M[i, j] = Am[i, j] * dtm
            for j in range(m):
                M[i, n + j] = Bm[i, j] * dtm
            M[i, n + m] = mp.mpf(float(d[i])) * dtm
        E = mp.expm(M)
        return _mp_round(E, range(n), range(n)), _mp_round(E, range(n), range(n, n + m)), _mp_round(E, range(n), [n + m])[:, 0]
    Am = _mp_matrix(mp, A)
    Bd = mp.zeros(n, m + 1)
    for i in range(n):
        for j in range(m):
            Bd[i, j] = mp.mpf(float(B[i, j]))
        Bd[i, m] = mp.mpf(float(d[i]))
    I = mp.eye(n)
    if method == 'fe':
        Ad, R = I + dtm * Am, dtm * Bd
    elif method == 'be':
        Ad = mp.inverse(I - dtm * Am)
        R = dtm * (Ad * Bd)
    elif method == 'bil':
        h = dtm / 2
        W = mp.inverse(I - h * Am)
        Ad, R = (I + h * Am) * W, dtm * (W * Bd)
    else:
        raise ValueError(method)
    return _mp_round(Ad, range(n), range(n)), _mp_round(R, range(n), range(m)), _mp_round(R, range(n), [m])[:, 0]


# ---------------------------------------------------------------------------------------------------- float64 yardsticks
def expm_pade13(M):
    """Higham 2005, Alg. 2.3 with m = 13 whatever the norm: scale by 2^-s, r_13 = (V - U)^-1 (V + U), square s times."""
    b = PADE_13
    s = squarings(M)
    A = M * 2.0 ** -s
    I = np.eye(A.shape[0])
    A2 = A @ A
    A4 = A2 @ A2
    A6 = A4 @ A2
    U = A @ (A6 @ (b[13] * A6 + b[11] * A4 + b[9] * A2) + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I)
    V = A6 @ (b[12] * A6 + b[10] * A4 + b[8] * A2) + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    R = np.linalg.solve(V - U, V + U)
    for _ in range(s):
        R = R @ R
    return R


def f64_discretize(A, B, d, dt, method, expm=expm_pade13):
    n, m = B.shape
    Bd = np.concatenate([B, d[:, None]], axis=1)
    I = np.eye(n)
    if method == 'zoh':
        E = expm(augmented(A, B, d, dt))
        return E[:n, :n].copy(), E[:n, n:n + m].copy(), E[:n, n + m].copy()
    if method == 'fe':
        Ad, R = I + dt * A, dt * Bd
    elif method == 'be':
        Ad, R = np.linalg.solve(I - dt * A, I), dt * np.linalg.solve(I - dt * A, Bd)
    elif method == 'bil':
        h = 0.5 * dt
        Ad, R = np.linalg.solve(I - h * A, I + h * A), dt * np.linalg.solve(I - h * A, Bd)
    else:
        raise ValueError(method)
    return Ad, R[:, :m].copy(), R[:, m].copy()


# ------------------------------------------------------------------------------------------- the elimination, generic
def tableau(A, B, d, dt, method, number=float):
    """[I - c A | R | dt B | dt d], R = I (be) or I + c A (bil), c = dt (be) or dt / 2 (bil); entries of type `number`."""
    n, m = B.shape
    N = number
    c = N(dt) if method == 'be' else N(dt) / N(2)
    T = []
    for i in range(n):
        ca = [c * N(A[i, j]) for j in range(n)]
        eye = [N(1 if i == j else 0) for j in range(n)]
        left = [eye[j] - ca[j] for j in range(n)]
        mid = eye if method == 'be' else [eye[j] + ca[j] for j in range(n)]
        T.append(left + mid + [N(dt) * N(B[i, j]) for j in range(m)] + [N(dt) * N(d[i])])
    return T


def gauss_jordan(T, rows, search=None):
    """Gauss-Jordan with partial pivoting on the first maximum of column p over the rows `search(p)` (default: p .. rows - 1) of the
    list-of-lists tableau T, in place; the pivot row is scaled by the reciprocal of the pivot as the kernel does.  Returns the pivot
    rows.  A zero pivot raises ZeroDivisionError."""
    cols = len(T[0])
    one = T[0][0] * 0 + 1
    pivots = []
    for p in range(rows):
        cand = list(search(p)) if search else list(range(p, rows))
        piv = max(cand, key=lambda i: (abs(T[i][p]), -i))
        if T[piv][p] == 0:
            raise ZeroDivisionError('zero pivot in column %d' % p)
        pivots.append(piv)
        T[p], T[piv] = T[piv], T[p]
        inv = one / T[p][p]
        T[p] = [v * inv for v in T[p]]
        for i in range(rows):
            if i != p and T[i][p] != 0:
                f = T[i][p]
                T[i] = [T[i][j] - f * T[p][j] for j in range(cols)]
    return pivots


def eliminate(A, B, d, dt, method, number=float, search=None):
    """be / bil through the elimination: (A_d, B_d, d_d, pivot rows); float64 arrays for number=float, object arrays of Fractions
    for number=Fraction."""
    n, m = B.shape
    T = tableau(A, B, d, dt, method, number)
    piv = gauss_jordan(T, n, search)
    X = np.array([row[n:] for row in T], dtype=np.float64 if number is float else object)
    return X[:, :n], X[:, n:n + m], X[:, n + m], piv


def expm_nilpotent_fraction(M):
    """sum_k M^k / k! for a nilpotent M of Fractions (list of lists): a finite sum, exact."""
    ne = len(M)
    E = [[Fraction(int(i == j)) for j in range(ne)] for i in range(ne)]
    P = [row[:] for row in E]
    for k in range(1, ne + 1):
        P = [[sum(P[i][l] * M[l][j] for l in range(ne)) / k for j in range(ne)] for i in range(ne)]
        if all(v == 0 for row in P for v in row):
            return E
        E = [[E[i][j] + P[i][j] for j in range(ne)] for i in range(ne)]
    raise ValueError('not nilpotent')


def ulps(a, b):
    """|a - b| in units of the spacing of b, elementwise (float64)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))
