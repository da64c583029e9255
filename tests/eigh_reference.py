"""The symmetric eigenproblem of csrc/eigh.hip (srom_eigh_dev) checked in np.longdouble: certificates that need no reference
eigenvectors, exact subspaces where the case has them, and a plain independent Jacobi for real spectra.  Nothing is imported from
the package or the oracle.

Certificates.  For a candidate (w, W) of a symmetric G, in long double,

    defect = max |W^T W - I|          resid = max |G W - W diag(w)|          (max over entries)

Let n be the size, d = n defect < 1 and R = G W - W diag(w), |R|_2 <= n resid.  W = U H with U orthogonal and H = (W^T W)^(1/2),
|H - I|_2 <= d; then G U - U diag(w) = R H^-1 + U (diag(w) H - H diag(w)) H^-1 has norm at most (n resid + 2 d max |w|) / (1 - d)
=: eta, and U^T G U = diag(w) + E with |E|_2 <= eta.  By Weyl's theorem every w_i, taken in ascending order, lies within eta of the
i-th eigenvalue of G: the two numbers bound the distance of every w_i to the spectrum without a reference.  For a cluster c of
the exact spectrum (a set of equal eigenvalues, at distance gap from the others) with m columns W_c, R_c = G W_c - W_c diag(w_c),
the Davis-Kahan sin-Theta theorem gives | sin Theta(span W_c, invariant subspace) |_F <= |R_c|_F (1 + m defect) / (gap - eta):
residual over gap.  The projectors then differ by sqrt(2) times that in the Frobenius norm, plus what W_c lacks of
orthonormality, |W_c W_c^T - U_c U_c^T|_2 <= 1.5 m defect.  `subspace_bound` is the resulting bound on the largest entry of
W_c W_c^T - P_c, with the constants rounded up:

    2 sqrt(n m) resid / (gap - eta) + 2 m defect.

With repeated eigenvalues only subspaces are compared -- the vectors inside a cluster are arbitrary -- and for a simple eigenvalue
the vector itself up to its sign, inside the same bound (m = 1).

Reference.  `jacobi` is the classical row-cyclic Jacobi method (Golub and Van Loan, Matrix Computations, section 8.5: pairs
(0, 1), (0, 2), ..., (n - 2, n - 1), one after the other, each rotation applied before the next angle is taken) in long double,
until off(A) <= 1e-19 |diag(A)| in the Frobenius norm (a 64-bit mantissa); an entry below half that bound divided by n is left alone
(the classical threshold variant: n^2 such entries cannot keep the stopping test from passing).  The kernels use round-robin orderings with n / 2
rotations at once from stale angles, other thresholds and other stopping rules: the reference shares neither pairing nor stopping
rule with them."""
import numpy as np

L = np.longdouble
STOP = L(1e-19)
MAX_SWEEPS = 60
BIG = L(2.0) ** 2000


class NotConverged(Exception):
    pass


def jacobi(G):
    """(w ascending, W with the eigenvectors as columns, sweeps), all long double, of the symmetric G."""
    n = G.shape[0]
    A = np.array(G, dtype=L)
    assert np.array_equal(A, A.T), 'G is not symmetric'
    M = np.concatenate((A, np.eye(n, dtype=L)))          # [A; V]: the column rotation is applied to both at once
    R = np.empty((2, 2), dtype=L)
    one = L(1)
    sweeps = 0
    while True:
        A = M[:n]
        d2 = (np.diag(A) ** 2).sum()
        off2 = ((A - np.diag(np.diag(A))) ** 2).sum()          # (not |A|^2 - d2: that cancels at 1e-19 d2)
        if off2 <= STOP * STOP * d2:
            break
        if sweeps == MAX_SWEEPS:
            raise NotConverged('row-cyclic Jacobi: off / diag = %.3e after %d sweeps' % (float(np.sqrt(off2 / d2)), sweeps))
        sweeps += 1
        skip = STOP * np.sqrt(d2) / (2 * n)
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if abs(apq) <= skip:
                    continue
                th = (A[q, q] - A[p, p]) / (2 * apq)
                if abs(th) > BIG:                            # th^2 would overflow: tan = 1 / (2 th) to the last bit
                    t = one / (2 * th)
                else:
                    t = (one if th >= 0 else -one) / (abs(th) + np.sqrt(th * th + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                R[0, 0] = c; R[0, 1] = s; R[1, 0] = -s; R[1, 1] = c
                M[:, (p, q)] = M[:, (p, q)] @ R              # columns of A and of V
                A[(p, q), :] = R.T @ A[(p, q), :]            # rows of A
                A[p, q] = A[q, p] = 0
    w = np.diag(M[:n]).copy()
    order = np.argsort(w, kind='stable')
    return w[order], M[n:][:, order].copy(), sweeps


def certificates(G, w, W):
    """(defect, resid, ascending) in long double."""
    Gl, wl, Wl = np.asarray(G, dtype=L), np.asarray(w, dtype=L), np.asarray(W, dtype=L)
    n = Gl.shape[0]
    defect = np.abs(Wl.T @ Wl - np.eye(n, dtype=L)).max()
    resid = np.abs(Gl @ Wl - Wl * wl).max()
    return float(defect), float(resid), bool(np.all(np.diff(wl) >= 0))


def eta(n, defect, resid, w_max):
    """The Weyl bound of the docstring on the distance of every w_i to the i-th eigenvalue."""
    d = n * defect
    return (n * resid + 2 * d * w_max) / (1 - d)


def clusters(lam_sorted):
    """[(first index, multiplicity, gap)] of an ascending exact spectrum; gap = inf for a spectrum of one value."""
    vals, first, counts = np.unique(lam_sorted, return_index=True, return_counts=True)
    out = []
    for i, (f, m) in enumerate(zip(first, counts)):
        gap = float(vals[i] - vals[i - 1]) if i > 0 else np.inf
        if i + 1 < len(vals):
            gap = min(gap, float(vals[i + 1] - vals[i]))
        out.append((int(f), int(m), gap))
    return out


def subspace_bound(n, m, gap, defect, resid, w_max):
    """Bound on max |W_c W_c^T - P_c| for a cluster of m columns at distance gap from the rest of the spectrum (docstring)."""
    if not np.isfinite(gap):
        return 2 * m * defect
    e = eta(n, defect, resid, w_max)
    assert e < gap, 'the eigenvalue bound does not separate the cluster'
    return 2 * np.sqrt(n * m) * resid / (gap - e) + 2 * m * defect


def subspace_errors(W, lam, Qs, s):
    """[(first, m, gap, error)] per cluster of the exact spectrum lam (one entry per column of Qs; Q = Qs / s): error = max entry of
    W_c W_c^T - Q_c Q_c^T for m > 1, of W_c -+ Q_c (the better sign) for m = 1.  Columns of W in ascending order of eigenvalue."""
    order = np.argsort(lam, kind='stable')
    Q = np.asarray(Qs, dtype=L)[:, order] / L(s)
    Wl = np.asarray(W, dtype=L)
    out = []
    for f, m, gap in clusters(np.asarray(lam)[order]):
        Wc, Qc = Wl[:, f:f + m], Q[:, f:f + m]
        if m == 1:
            err = min(np.abs(Wc - Qc).max(), np.abs(Wc + Qc).max())
        else:
            err = np.abs(Wc @ Wc.T - Qc @ Qc.T).max()
        out.append((f, m, gap, float(err)))
    return out


def is_permutation(W):
    """W has entries exactly 0 or 1, one 1 per row and per column."""
    W = np.asarray(W)
    return bool(np.isin(W, (0.0, 1.0)).all() and np.array_equal(W.sum(0), np.ones(W.shape[0])) and
                np.array_equal(W.sum(1), np.ones(W.shape[0])))
