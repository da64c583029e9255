"""The Euclidean projection onto a polyhedron, min 1/2 |p - x|^2 s.t. A p <= b (csrc/poly.hip, spoly_project), restated as an
active-set method in np.longdouble that proves its own answer.  No interior point, nothing imported from the package or the oracle.

  project            Goldfarb and Idnani's dual active-set iteration (Math. Programming 27, 1983) for H = I: start at p = x with no
                     row active, add the most violated row, stepping along the part of its normal orthogonal to the active normals
                     and dropping the active row whose multiplier reaches zero first; a violated row that depends on the active ones
                     with no multiplier to give up proves the polyhedron empty (`Infeasible`).  Finite without an anti-cycling rule and
                     without a starting guess.  The point and the multipliers of the final active set W are then solved once more
                     from the data, p = x - A_W^T lam, (A_W A_W^T) lam = A_W x - b_W, by a hand-written long-double elimination, and
                     the certificate is evaluated on that pair.
  Certificate        the projection is unique, and a pair (p, lam) with A p <= b, lam >= 0, p - x + A^T lam = 0 and lam_i (b - A p)_i
                     = 0 is it.  Stationarity holds by construction (p is formed from lam), complementarity too (lam is zero off W,
                     the rows of W are solved as equalities).  What is checked is max(A p - b) <= 64 eps scale and
                     min lam >= -64 eps scale, eps = 2^-63, scale = max(1, |x|_inf, |b|_inf): `project` raises `NotCertified`
                     otherwise.  margin = min(min lam over W, min slack off W): how far the case is from a change of active set.
  kkt_residuals      for an arbitrary candidate p: the rows within `tol` of active (|a_i p - b_i| <= tol |a_i|_2), the best multipliers
                     lam >= 0 on them (Lawson-Hanson NNLS, refined in long double on its support), and the residuals
                     |x - p - A^T lam|_2 and max(A p - b).  A necessary condition with teeth: a point moved by d > tol along a face
                     leaves a stationarity residual d, a point moved by d > tol off a face loses that row and with it lam_i |a_i|
                     of stationarity.  The proof of a bound is the distance to the certified point; this is the second
                     opinion that does not use the reference's active set.
  enumerate_projection   brute force over every active set of at most n rows, for the cross-check at n <= 3.

The bound the kernel can promise.  Let (p, lam, s) be the interior point's last iterate, lam, s > 0, with the residuals
rd = p - x + A^T lam, rp = A p + s - b, mu = lam.s / rows, and (p*, lam*, s*) the solution, lam*.s* = 0.  Subtracting the
stationarity equations, (p - p*) + A^T (lam - lam*) = rd; multiplied by (p - p*), with A (p - p*) = rp - s + s*:

    e^2 = rd.(p - p*) - (lam - lam*).rp + lam.s - lam.s* - lam*.s,        e = |p - p*|_2

The cross terms lam.s* and lam*.s are non-negative, so

    e^2 <= e |rd|_2 + |lam - lam*|_1 |rp|_inf + rows mu.

At a weakly active row (s*_i = lam*_i = 0) nothing but the last term holds the iterate: e ~ sqrt(rows mu).  A stopping rule
mu <= 1e-13 scale therefore allows 2.5e-6 at 64 rows; the contract e <= 1e-9 scale (CONTRACT) needs rows mu <= 1e-18 scale^2, with
rd and rp near their rounding floor.  float64 does not give that where strongly and weakly active rows meet at an angle: the
multiplier step of a strongly active row is d_i (a_i.dp + rp_i) with d_i = lam_i / s_i ~ lam_i^2 / mu, and a_i.dp carries
eps |a_i| |dp| of rounding while dp still moves by ~sqrt(mu) along the weakly active rows, so rd stalls near eps lam^2 / sqrt(mu)
(1e-7 .. 1e-6 at mu = 1e-20) and the iterate with it.  The kernel therefore uses the interior point only to find the active set
and returns the point of an active-set step on it, with its own certificate (csrc/poly.hip, DESIGN.md "Exact projection tests")."""
import itertools

import numpy as np

L = np.longdouble
EPS = float(np.finfo(L).eps)
CERT = 64.0 * EPS
DEPENDENT = 2.0 ** -50          # |z|^2 / |a|^2 below this: the row depends on the active ones (an angle of 3e-8)
CONTRACT = 1e-9                 # |p - p*|_2 <= CONTRACT scale, for every certified case whatever its margin


class Infeasible(Exception):
    """The polyhedron is empty."""


class NotCertified(Exception):
    """The active-set iteration ended without a pair (p, lam) that meets the certificate."""


def scale_of(b, x):
    """The kernel's own: max(1, |x|_inf, |b|_inf)."""
    return max(1.0, float(np.abs(np.asarray(x, dtype=np.float64)).max()), float(np.abs(np.asarray(b, dtype=np.float64)).max()))


def solve_ld(G, R):
    """G^-1 R by Gaussian elimination with partial pivoting in long double, one step of iterative refinement."""
    G, R = np.array(G, dtype=L), np.array(R, dtype=L)
    k = G.shape[0]
    vec = R.ndim == 1
    R = R.reshape(k, -1)

    def once(rhs):
        T = np.concatenate([G, rhs], axis=1)
        for c in range(k):
            piv = c + int(np.argmax(np.abs(T[c:, c])))
            if T[piv, c] == 0:
                raise ZeroDivisionError('singular matrix')
            if piv != c:
                T[[c, piv]] = T[[piv, c]]
            for r in range(c + 1, k):
                if T[r, c] != 0:
                    T[r, c:] -= (T[r, c] / T[c, c]) * T[c, c:]
        X = np.zeros_like(rhs)
        for r in range(k - 1, -1, -1):
            X[r] = (T[r, k:] - T[r, r + 1:k] @ X[r + 1:]) / T[r, r]
        return X
    X = once(R)
    X = X + once(R - G @ X)
    return X[:, 0] if vec else X


def _on_active_set(A, b, x, W):
    """(p, lam over W) with the rows of W held as equalities."""
    if not W:
        return x.copy(), np.zeros(0, dtype=L)
    Aw = A[W]
    G = Aw @ Aw.T
    lam = solve_ld(G, Aw @ x - b[W])
    p = x - Aw.T @ lam
    # where the active normals nearly cancel (a sharp wedge) lam is large and its own rounding moves p: one more correction of
    # the point along the normals, from the residual of the equalities at p itself
    dl = solve_ld(G, Aw @ p - b[W])
    return p - Aw.T @ dl, lam + dl


class Projection:
    def __init__(self, p, lam, W, violation, min_lam, margin, steps):
        self.p, self.lam, self.W = p, lam, W                # long double point, multipliers of every row, the active set
        self.violation, self.min_lam, self.margin, self.steps = violation, min_lam, margin, steps

    @property
    def p64(self):
        return self.p.astype(np.float64)


def project(A, b, x, max_steps=2000):
    """The certified projection of x onto {p : A p <= b}; raises Infeasible or NotCertified."""
    A, b, x = np.array(A, dtype=L), np.array(b, dtype=L), np.array(x, dtype=L)
    rows, n = A.shape
    if not (np.isfinite(A.astype(np.float64)).all() and np.isfinite(b.astype(np.float64)).all() and np.isfinite(x.astype(np.float64)).all()):
        raise ValueError('non-finite data')
    tol = CERT * scale_of(b, x)
    W, lam = [], np.zeros(0, dtype=L)
    p = x.copy()
    steps = 0
    while True:
        v = A @ p - b
        if W:
            v[W] = -np.inf
        q = int(np.argmax(v))
        if not v[q] > tol:
            break
        aq = A[q]
        lq = L(0)
        while True:                                                 # bring row q in, giving up rows of W as their multipliers vanish
            steps += 1
            if steps > max_steps:
                raise NotCertified('no end after %d steps' % max_steps)
            if W:
                Aw = A[W]
                r = solve_ld(Aw @ Aw.T, Aw @ aq)
                z = aq - Aw.T @ r
            else:
                r, z = np.zeros(0, dtype=L), aq.copy()
            dependent = not (z @ z > DEPENDENT * (aq @ aq))
            t2 = np.inf if dependent else (aq @ p - b[q]) / (z @ aq)
            t1, k1 = np.inf, -1
            for k in range(len(W)):
                if r[k] > 0 and lam[k] / r[k] < t1:
                    t1, k1 = lam[k] / r[k], k
            if dependent and k1 < 0:
                raise Infeasible('row %d is violated and depends on the active rows with no multiplier to give up' % q)
            t = min(t1, t2)
            if not dependent:
                p = p - t * z
            lam = lam - t * r
            lq = lq + t
            if t2 <= t1:
                W.append(q)
                lam = np.append(lam, lq)
                break
            del W[k1]
            lam = np.delete(lam, k1)
    p, lam_w = _on_active_set(A, b, x, W)
    lam_all = np.zeros(rows, dtype=L)
    lam_all[W] = lam_w
    slack = b - A @ p
    violation = float(-slack.min())
    min_lam = float(lam_w.min()) if W else np.inf
    off = np.ones(rows, dtype=bool)
    off[W] = False
    # duplicates of an active row and further rows through a degenerate vertex are weakly active: slack 0 off W, margin 0
    margin = min(min_lam, float(slack[off].min()) if off.any() else np.inf)
    if violation > tol or min_lam < -tol:
        raise NotCertified('violation %.3e, smallest multiplier %.3e, tolerance %.3e' % (violation, min_lam, tol))
    return Projection(p, lam_all, sorted(W), violation, min_lam, max(margin, 0.0), steps)


def kkt_residuals(A, b, x, p, tol):
    """(stationarity |x - p - A^T lam|_2, feasibility max(A p - b), lam) of a candidate p, lam >= 0 fitted on the rows with
    |a_i p - b_i| <= tol |a_i|_2."""
    from scipy.optimize import nnls
    A, b, x, p = np.array(A, dtype=L), np.array(b, dtype=L), np.array(x, dtype=L), np.array(p, dtype=L)
    res = A @ p - b
    norms = np.sqrt((A * A).sum(axis=1))
    act = np.flatnonzero(np.abs(res) <= tol * norms)             # within tol of the face, as a distance
    g = x - p
    lam = np.zeros(A.shape[0], dtype=L)
    if len(act):
        l64, _ = nnls(A[act].T.astype(np.float64), g.astype(np.float64), maxiter=50 * A.shape[0] + 100)
        lam[act] = l64
        S = [int(i) for i, v in zip(act, l64) if v > 0]
        while S:                       # refine on the support: least squares in long double over an independent subset
            As = A[S]
            try:
                ls = solve_ld(As @ As.T, As @ g)
                for _ in range(3):                 # the normal equations square the condition (1e8 at the sharp wedge, with
                    ls = ls + solve_ld(As @ As.T, As @ (g - As.T @ ls))      # lam = 5000): corrected from the residual itself
            except ZeroDivisionError:
                ls = None
            if ls is not None and np.isfinite(ls.astype(np.float64)).all() and np.abs(As @ As.T @ ls - As @ g).max() <= 1e-6 * max(1.0, float(np.abs(As @ g).max())):
                if (ls >= 0).all() and float(np.sqrt(((g - As.T @ ls) ** 2).sum())) <= float(np.sqrt(((g - A.T @ lam) ** 2).sum())):
                    lam[:] = 0
                    lam[S] = ls
                break
            S = S[:-1]                 # a dependent support (duplicated rows): the fit needs only an independent part of it
    stat = float(np.sqrt(((g - A.T @ lam) ** 2).sum()))
    return stat, float(res.max()), lam


def enumerate_projection(A, b, x):
    """Brute force: of the KKT points of every set of at most n independent active rows, the feasible one with lam >= 0 nearest to
    x (long double; tolerances 64 eps scale as in `project`)."""
    A, b, x = np.array(A, dtype=L), np.array(b, dtype=L), np.array(x, dtype=L)
    rows, n = A.shape
    tol = CERT * scale_of(b, x)
    best, bestd = None, np.inf
    for k in range(0, min(rows, n) + 1):
        for W in itertools.combinations(range(rows), k):
            W = list(W)
            if k:
                Aw = A[W]
                G = Aw @ Aw.T
                if abs(float(np.linalg.det(G.astype(np.float64)))) <= 1e-12 * float(np.prod(np.diag(G).astype(np.float64))):
                    continue
            try:
                p, lam = _on_active_set(A, b, x, W)
            except ZeroDivisionError:
                continue
            if k and lam.min() < -tol:
                continue
            if (A @ p - b).max() <= tol:
                d = float(np.sqrt(((p - x) ** 2).sum()))
                if d < bestd:
                    best, bestd = p, d
    return best
