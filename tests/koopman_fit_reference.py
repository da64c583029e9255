"""The Koopman fit (EDMD) as its definition states it, in np.longdouble and np.float64 on the same float64 records.  No GPU and no product
import: the observable order is stated here (tests/test_koopman_fit_reference_cpu.py cross-checks it against observable_exponents).

  kept rows 0, s, 2s, ..; zeta_i = [y_i, y_{i-1} .. y_{i-d}, u_{i-1} .. u_{i-d}] of scaled samples, i >= d; psi_i the monomials of zeta_i
  (graded; inside a degree ascending in the exponent tuple read from the last variable to the first; then the constant unless dmd);
  v_i = scale_down(u[i + u_lag]); pairs (i, i + 1), d <= i <= T' - 2, inside an episode; Phi_i = [psi_i; v_i];
  G = sum Phi_i Phi_i^T, R = sum psi_{i+1} Phi_i^T, Q = sum |psi_{i+1}|^2, S = pairs; [A B] = R (G + ridge I)^-1."""
import itertools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
E_ORACLE_MAX = 1e-11


def exponents(nzeta, degree, dmd):
    """(P, nzeta) exponent rows in the lift's order."""
    rows = []
    for deg in range(1, degree + 1):
        level = _level(nzeta, deg)
        level.sort(key=lambda e: e[::-1])
        rows += level
    if not dmd:
        rows.append((0,) * nzeta)
    return np.array(rows, dtype=np.int64).reshape(len(rows), nzeta)


def _level(nzeta, deg):
    """Every exponent tuple of total degree deg (combinations with repetition of the variables)."""
    out = []
    for combo in itertools.combinations_with_replacement(range(nzeta), deg):
        e = [0] * nzeta
        for v in combo:
            e[v] += 1
        out.append(tuple(e))
    return out


def scale_from(adds, stride, dtype=np.float64):
    """offset = (max + min) / 2, factor = (max - min) / 2 per channel over the kept rows of every (Y, U) of `adds`."""
    out = {}
    for k, name in ((0, 'y'), (1, 'u')):
        rows = np.concatenate([a[k][:, ::stride].reshape(-1, a[k].shape[2]) for a in adds]).astype(dtype)
        hi, lo = rows.max(axis=0), rows.min(axis=0)
        out[name + '_offset'], out[name + '_factor'] = (hi + lo) / 2, (hi - lo) / 2
    return out


def scale_down(v, off, fac, dtype):
    """(v - off) / fac.  In long double as written.  In float64 rounded once, as the fit's kernel does it: the subtraction's error (TwoSum)
    and the division's remainder (a two-product with Dekker's split; the kernel has an fma) are folded back into the quotient.  The
    bounds are stated against the long-double value, and a sum's term is a product of up to 2 degree scaled samples: a sample that
    occurs g times in a term brings g times its own error."""
    v, off, fac = v.astype(dtype), off.astype(dtype), fac.astype(dtype)
    d = v - off
    if dtype is not np.float64:
        return d / fac
    t = d - v
    e = (v - (d - t)) - (off + t)                 # v - off = d + e exactly
    q = d / fac
    p = q * fac
    qh, fh = (x * 134217729.0 - (x * 134217729.0 - x) for x in (q, fac))       # the upper 26 bits (2^27 + 1)
    ql, fl = q - qh, fac - fh
    pe = ((qh * fh - p) + qh * fl + ql * fh) + ql * fl          # q fac = p + pe exactly
    return q + (((d - p) - pe) + e) / fac


def lift(zeta, exps, dtype):
    """(rows, P) monomials of the rows of zeta."""
    out = np.ones((zeta.shape[0], exps.shape[0]), dtype=dtype)
    for k in range(exps.shape[0]):
        for j in np.flatnonzero(exps[k]):
            for _ in range(int(exps[k, j])):
                out[:, k] = out[:, k] * zeta[:, j]
    return out


def pairs(adds, scale, d, degree, dmd, stride, u_lag, dtype):
    """(Phi (S, n), Psi1 (S, P)) of every pair of the records `adds` = [(Y (E, T, n_y), U (E, T, m)), ..]."""
    ny, m = adds[0][0].shape[2], adds[0][1].shape[2]
    exps = exponents(ny * (d + 1) + m * d, degree, dmd)
    yo, yf, uo, uf = (np.ravel(scale[k]) for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor'))
    Phi, Psi1 = [np.zeros((0, exps.shape[0] + m), dtype=dtype)], [np.zeros((0, exps.shape[0]), dtype=dtype)]
    for Y, U in adds:
        for e in range(Y.shape[0]):
            y = scale_down(Y[e, ::stride], yo, yf, dtype)
            u = scale_down(U[e, ::stride], uo, uf, dtype)
            Tk = y.shape[0]
            if Tk <= d + 1:
                continue
            zeta = np.hstack([y[d:]] + [y[d - j:Tk - j] for j in range(1, d + 1)] + [u[d - j:Tk - j] for j in range(1, d + 1)])
            psi = lift(zeta, exps, dtype)
            Phi.append(np.hstack([psi[:-1], u[d + u_lag:Tk - 1 + u_lag]]))
            Psi1.append(psi[1:])
    return np.concatenate(Phi), np.concatenate(Psi1)


def sums(adds, scale, d, degree, dmd, stride, u_lag, dtype):
    """dict G, R, Q, pairs, and absG, absR: the sums of the absolute terms (the bounds are stated on them)."""
    Phi, Psi1 = pairs(adds, scale, d, degree, dmd, stride, u_lag, dtype)
    return dict(G=Phi.T @ Phi, R=Psi1.T @ Phi, Q=(Psi1 * Psi1).sum(), pairs=Phi.shape[0], absG=np.abs(Phi).T @ np.abs(Phi),
                absR=np.abs(Psi1).T @ np.abs(Phi))


def solve(G, R, ridge, dtype):
    """X = R (G + ridge I)^-1 by Cholesky in `dtype`; None when a pivot is not positive."""
    n = G.shape[0]
    M = G.astype(dtype) + dtype(ridge) * np.eye(n, dtype=dtype)
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = R.astype(dtype).T.copy()                 # L Z = R^T, L^T X^T = Z
    for j in range(n):
        Z[j] = (Z[j] - L[j, :j] @ Z[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Z[j] = (Z[j] - L[j + 1:, j] @ Z[j + 1:]) / L[j, j]
    return Z.T


def fit(adds, scale, d, degree, dmd, stride, u_lag, ridge, dtype):
    """(A, B, sums) of the definition."""
    s = sums(adds, scale, d, degree, dmd, stride, u_lag, dtype)
    X = solve(s['G'], s['R'], ridge, dtype)
    P = s['R'].shape[0]
    return (None, None, s) if X is None else (X[:, :P], X[:, P:], s)


def err(a, b):
    """max |a - b| / max(1, max |b|), in long double."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / max(LD(1), np.abs(b).max())) if b.size else 0.0


def tolerance(e_oracle):
    return max(100.0 * e_oracle, 1e-13)


def sums_bound(ref, degree):
    """Elementwise bounds of G and R: (S + 2 degree + 2) eps sum |terms| -- S roundings of the accumulation in any order, 2 per factor for
    the scaling's subtraction and division, one per product of the monomial recurrence."""
    c = (ref['pairs'] + 2 * degree + 2) * EPS
    return c * ref['absG'], c * ref['absR']


def sums_use(got_G, got_R, ref, degree):
    """The largest share of the sums bound that (got_G, got_R) use against the long-double sums `ref`."""
    bG, bR = sums_bound(ref, degree)
    use = 0.0
    for got, want, b in ((got_G, ref['G'], bG), (got_R, ref['R'], bR)):
        d = np.abs(np.asarray(got, dtype=LD) - want)
        pos = b > 0
        assert not np.any(d[~pos] > 0), 'a sum whose terms all vanish must be zero'
        if pos.any():
            use = max(use, float((d[pos] / b[pos]).max()))
    return use


def certificate(X, G, R, ridge):
    """(|X (G + ridge I) - R|_F, 4 n^2 eps |X|_F |G + ridge I|_F) in long double: the backward error of an SPD elimination (Higham:
    gamma_{3n+1} with | |L| |L^T| |_2 <= n |G|_2); it holds whatever the conditioning."""
    n = G.shape[0]
    X, M, R = np.asarray(X, dtype=LD), np.asarray(G, dtype=LD) + LD(ridge) * np.eye(n, dtype=LD), np.asarray(R, dtype=LD)
    fro = lambda v: np.sqrt((v * v).sum())
    return float(fro(X @ M - R)), float(4 * n * n * EPS * fro(X) * fro(M))
