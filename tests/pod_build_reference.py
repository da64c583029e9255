"""Plain statements of the POD build products behind csrc/gramian.hip, csrc/abt_dev.h, csrc/snapshots.hip and csrc/eigh.hip
(test infrastructure only).  Nothing here imports the package under test.

Two kinds of reference, for the two kinds of data of tests/pod_build_cases.py:

  integer-valued data (entries in {-8..8}, stored as float64): every product and every partial sum of S S^T, S^T W and
  |y|^2 - 2 y.x + |x|^2 is an integer far below 2^53, so float64 arithmetic is exact in ANY order of accumulation, fused or not,
  split along K or not.  The reference is numpy float64 and the comparison is np.array_equal.  `*_pyint` restate single entries
  in Python int arithmetic (tests/test_pod_build_reference_cpu.py holds the float64 references against them).

  real data: np.longdouble (80-bit on x86: eps 1.1e-19) and the elementwise bound `dot_bound`.

The bound.  A dot product of length K evaluated in float64 in any order, with or without fused multiply-adds, whose K-range is cut
in at most 64 parts that are summed afterwards, carries at most K + 63 roundings on the path of any term, so its error is at most
((1 + u)^(K + 63) - 1) sum_k |a_k| |b_k| <= (K + 64) u sum_k |a_k| |b_k| with u = 2^-53 (the second-order term is below u for
K + 63 < 1e8).  64 is the largest number of parts anywhere in the family (abt_dev.h caps its split there; the Gramian tail uses 8,
the 64 lanes of row_sqnorm_kernel are summed in a 6-level tree).  Nothing in it is measured."""
import numpy as np

from lq_reference import LD, ld          # noqa: F401

U53 = 2.0 ** -53
MAX_PARTS = 64


# ---------------------------------------------------------------------------------------------- integer data, exact
def gramian(S):
    """G = S S^T in float64 (exact on integer data)."""
    S = np.asarray(S, dtype=np.float64)
    return S @ S.T


def modes(S, W):
    """U = S^T W in float64 (exact on integer data)."""
    return np.asarray(S, dtype=np.float64).T @ np.asarray(W, dtype=np.float64)


def row_sqnorms(S):
    S = np.asarray(S, dtype=np.float64)
    return (S * S).sum(axis=1)


def sqdist_rows(S, Y):
    """D[c][i] = max(0, |y_c|^2 - 2 y_c . x_i + |x_i|^2), (nc x n_s), in float64 (exact on integer data)."""
    S, Y = np.asarray(S, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return np.maximum(0.0, row_sqnorms(Y)[:, None] - 2.0 * (Y @ S.T) + row_sqnorms(S)[None, :])


def _ints(v):
    out = [int(x) for x in v]
    assert all(float(i) == float(x) for i, x in zip(out, v)), 'not integer data'
    return out


def gramian_entry_pyint(S, i, j):
    a, b = _ints(S[i]), _ints(S[j])
    return sum(x * y for x, y in zip(a, b))


def modes_entry_pyint(S, W, i, j):
    a, b = _ints(S[:, i]), _ints(W[:, j])
    return sum(x * y for x, y in zip(a, b))


def sqdist_entry_pyint(S, Y, c, i):
    x, y = _ints(S[i]), _ints(Y[c])
    return max(0, sum(v * v for v in y) - 2 * sum(a * b for a, b in zip(x, y)) + sum(v * v for v in x))


# ------------------------------------------------------------------------------------------------ real data, long double
def abt_ld(A, B):
    """A B^T in long double (shapes of at most 300 x 300 x 1100: numpy's long-double matmul is a plain loop)."""
    A, B = ld(A), ld(B)
    assert A.shape[0] <= 300 and B.shape[0] <= 300 and A.shape[1] <= 1100
    return A @ B.T


def dot_bound(absprod, K):
    """(K + 64) 2^-53 (|A| |B|^T)_ij for dots of length K (see the module docstring); absprod = |A| |B|^T."""
    return (K + MAX_PARTS) * U53 * np.asarray(absprod, dtype=np.float64)


def abt_bound(A, B):
    A, B = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(B, dtype=np.float64))
    return dot_bound(A @ B.T, A.shape[1])


def row_sqnorms_ld(S):
    S = ld(S)
    return (S * S).sum(axis=1)


def sqdist_rows_ld(S, Y):
    """(D in long double without the clamp at zero, bound): the three dots |y|^2, y.x, |x|^2 each inside dot_bound, the factor 2
    exact, and the two float64 additions that join them one rounding each of a partial sum that is at most
    T = |y|^2 + 2 |y|.|x| + |x|^2 in magnitude: (K + 64) u T + 2 u T (1 + (K + 64) u) <= (K + 67) u T."""
    S, Y = ld(S), ld(Y)
    K = S.shape[1]
    xn, yn = (S * S).sum(axis=1), (Y * Y).sum(axis=1)
    D = yn[:, None] - 2 * abt_ld(Y, S) + xn[None, :]
    T = yn[:, None] + 2 * (np.abs(Y) @ np.abs(S).T) + xn[None, :]
    return D, (K + MAX_PARTS + 3) * U53 * T.astype(np.float64)


def mode_floor(n):
    return max(1e-28, n * 2.0 ** -52)


def scaled_modes(V, w, k):
    """select_modes: Wk[j][i] = V[n-1-i][j] / sqrt(w[n-1-i]) in float64 for ascending w (rows of V = eigenvectors); a zero column
    where w_i <= max(1e-28, n eps) w_max or w_i <= 0 (csrc/mode_rule.h: the rounding noise of an eigensolver on a formed Gramian)."""
    V, w = np.asarray(V, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    Wk = np.zeros((n, k))
    for i in range(k):
        wi = w[n - 1 - i]
        if wi > mode_floor(n) * w[n - 1] and wi > 0.0:
            Wk[:, i] = V[n - 1 - i] / np.sqrt(wi)
    return Wk


def within_ulps(got, ref, ulps):
    """|got - ref| <= ulps * spacing(ref), elementwise (a correctly rounded divide and square root leave nothing else)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return bool(np.all(np.abs(got - ref) <= ulps * np.spacing(np.abs(ref))))
