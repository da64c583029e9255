"""Extended-precision solution of the continuous algebraic Riccati equation behind csrc/care.hip (test infrastructure only).

    A'X + X A - X G X + Q = 0,   G = B R^-1 B',   K = -R^-1 B' X   (u = +K x)

Plain numpy in np.longdouble with a hand-written pivoted elimination, in the style of tests/lq_reference.py; nothing here imports
the package under test.  The solution comes from the structure-preserving doubling recursion on the Cayley transform of the
Hamiltonian (Chu, Fan, Lin 2005) followed by defect corrections, all in long double.  How it is obtained does not make it a
reference; its certificate does (`certificate`, asserted per case by tests/test_care_reference_cpu.py and by the GPU tests): a
relative residual at least 30 times below that of scipy.linalg.solve_continuous_are on the same inputs, and a closed loop
A - G X with every eigenvalue in the open left half plane."""
import numpy as np

from lq_reference import LD, ld, err, chol_solve, sym  # noqa: F401  (err, sym: re-exported for the tests)

CERTIFICATE_RATIO = 30.0


def gauss_jordan(W, B):
    """W^-1 B by Gauss-Jordan elimination with partial pivoting (physical row swaps) on the tableau [W | B], long double."""
    W, B = ld(W), ld(B)
    n = W.shape[0]
    T = np.concatenate([W, B.reshape(n, -1)], axis=1)
    for j in range(n):
        pv = j + int(np.argmax(np.abs(T[j:, j])))
        if not np.abs(T[pv, j]) > 0:
            raise np.linalg.LinAlgError('gauss_jordan: singular matrix')
        if pv != j:
            T[[j, pv]] = T[[pv, j]]
        T[j] = T[j] / T[j, j]
        f = T[:, j].copy()
        f[j] = 0
        T[:, j:] -= np.outer(f, T[j, j:])          # the columns left of j are already those of the identity
    return T[:, n:].reshape(B.shape)


def _doubling(A, G, H, max_iter=100):
    """Stabilising solution of A'X + X A - X G X + H = 0 by doubling, long double.  Returns X and the number of steps."""
    n = A.shape[0]
    I = np.eye(n, dtype=LD)
    gamma = LD(1.5) * max(np.abs(A).sum(axis=1).max(), LD(1e-3))
    Ag = A - gamma * I
    T1, Ainv = np.split(gauss_jordan(Ag, np.concatenate([G, I], axis=1)), 2, axis=1)
    W = Ag.T + H @ T1
    Hs, Winv = np.split(gauss_jordan(W, np.concatenate([H @ Ainv, I], axis=1)), 2, axis=1)
    E, Gk, Hk = I + 2 * gamma * Winv.T, 2 * gamma * T1 @ Winv, 2 * gamma * Hs
    done = False
    for it in range(1, max_iter + 1):
        V1, V2 = np.split(gauss_jordan(I + Gk @ Hk, np.concatenate([E, Gk], axis=1)), 2, axis=1)
        dH = E.T @ (Hk @ V1)
        E, Gk, Hk = E @ V1, Gk + E @ V2 @ E.T, Hk + dH
        if not np.all(np.isfinite(Hk)):
            raise np.linalg.LinAlgError('care: the doubling recursion overflowed (not stabilisable?)')
        if done:                                   # one step past the stopping rule: the recursion converges quadratically
            return Hk, it
        done = bool(np.abs(dH).max() <= LD(1e-17) * max(np.abs(Hk).max(), LD(1e-300)))
    raise np.linalg.LinAlgError('care: no convergence within max_iter doubling steps')


def input_weight(B, R):
    """G = B R^-1 B' (symmetrised), long double."""
    B = ld(B)
    return sym(B @ chol_solve(R, B.T))


def residual_matrix(A, G, Q, X):
    return A.T @ X + X @ A - X @ G @ X + Q


def residual(A, B, Q, R, X):
    """Relative CARE residual in long double: max|A'X + X A - X G X + Q| over the largest of its four terms."""
    A, Q, X = ld(A), ld(Q), ld(X)
    G = input_weight(B, R)
    scale = max(np.abs(A.T @ X).max(), np.abs(X @ A).max(), np.abs(X @ G @ X).max(), np.abs(Q).max())
    return float(np.abs(residual_matrix(A, G, Q, X)).max() / scale)


def care(A, B, Q, R, corrections=1):
    """The stabilising solution X (long double) and the doubling steps of the first solve.  Each defect correction solves the
    Riccati equation of the error about the current closed loop, (A - G X)'D + D (A - G X) - D G D + res(X) = 0, by the same
    recursion, and adds D.  One correction is what the certificate needs on the lightly damped cases (without it the residual of
    some is only 20 times below scipy's); a second one changes nothing."""
    A, Q = ld(A), ld(Q)
    G = input_weight(B, R)
    X, it = _doubling(A, G, Q)
    X = sym(X)
    for _ in range(corrections):
        D, _ = _doubling(A - G @ X, G, sym(residual_matrix(A, G, Q, X)))
        X = sym(X + D)
    return X, it


def gain(B, R, X):
    """K = -R^-1 B' X (u = +K x), long double."""
    return -chol_solve(R, ld(B).T @ ld(X))


def closed_loop_eigenvalues(A, B, R, X):
    """Eigenvalues of A - G X = A + B K (float64 eigensolver on the long-double closed loop)."""
    return np.linalg.eigvals(np.asarray(ld(A) - input_weight(B, R) @ ld(X), dtype=np.float64))


def certificate(A, B, Q, R, X, X_scipy):
    """(residual of X, residual of scipy's solution, largest real part of the closed-loop eigenvalues).  X is a reference when
    CERTIFICATE_RATIO * residual(X) <= residual(X_scipy) and the largest real part is negative."""
    return (residual(A, B, Q, R, X), residual(A, B, Q, R, X_scipy), float(closed_loop_eigenvalues(A, B, R, X).real.max()))
