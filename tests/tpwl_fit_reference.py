"""The TPWL fit ("TPWL model identification") as its definition states it, parameterised by dtype: np.longdouble is the
reference, float64 the oracle.  No GPU and no product import.

  kept rows 0, s, 2s, ..; samples: the kept rows with a kept successor in their episode;
  p(i) = the first minimum over the points of w_q |q_p - q_i| + w_v |v_p - v_i| (x = [v; q]); every search records its margin;
  phi_i = [x_i - x_p; u_i; 1], g_i = (x_{i+1} - x_i) / Ts;
  per point G = sum phi phi^T, R = sum g phi^T, Q = sum |g|^2, S = the samples;
  (D^-1/2 G D^-1/2 + ridge I) z = D^-1/2 r, [A_c | B_c | c] = D^-1/2 z, D = diag(G); d_c = c - A_c x_p; u = G[inputs, constant] / S."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
TR = 64


def nearest(x, q, v, w, dtype=LD):
    """(index (B,), margin (B,)) of the states x (B, n_x): the first minimum of d, and (d_second - d_first) / d_second over the points
    that are no exact copy of an earlier point (a copy ties exactly in every arithmetic: the first-minimum rule decides, not rounding);
    inf with one distinct point."""
    x, q, v = np.atleast_2d(x).astype(dtype), np.asarray(q, dtype=dtype), np.asarray(v, dtype=dtype)
    r = q.shape[1]
    d = dtype(w['q']) * np.sqrt(((q[None] - x[:, None, r:]) ** 2).sum(axis=2))
    if w['v'] != 0.0:
        d = d + dtype(w['v']) * np.sqrt(((v[None] - x[:, None, :r]) ** 2).sum(axis=2))
    idx = np.argmin(d, axis=1)
    pts = np.hstack([np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)])
    first = [p for p in range(pts.shape[0]) if not any(np.array_equal(pts[p], pts[o]) for o in range(p))]
    if len(first) < 2:
        return idx, np.full(x.shape[0], np.inf)
    ds = np.sort(d[:, first], axis=1)
    return idx, ((ds[:, 1] - ds[:, 0]) / ds[:, 1]).astype(np.float64)


def samples(adds, q, v, w, Ts, dtype=LD):
    """(region (S,), phi (S, n), g (S, n_x), margin (S,), where (S, 3): add, episode, kept row) over the samples of
    `adds` = [(X, U, stride), ..] in the order add, episode, row."""
    xp = np.hstack([np.asarray(v), np.asarray(q)]).astype(dtype)
    reg, Phi, Gt, mar, where = [], [], [], [], []
    for a, (X, U, stride) in enumerate(adds):
        for e in range(X.shape[0]):
            x, u = X[e, ::stride].astype(dtype), U[e, ::stride].astype(dtype)
            if x.shape[0] < 2:
                continue
            idx, mg = nearest(x[:-1], q, v, w, dtype)
            reg.append(idx); mar.append(mg)
            Phi.append(np.hstack([x[:-1] - xp[idx], u[:-1], np.ones((x.shape[0] - 1, 1), dtype=dtype)]))
            Gt.append((x[1:] - x[:-1]) / dtype(Ts))
            where.append(np.stack([np.full(x.shape[0] - 1, a), np.full(x.shape[0] - 1, e), np.arange(x.shape[0] - 1)], axis=1))
    nx, m = adds[0][0].shape[2], adds[0][1].shape[2]
    if not reg:
        return np.zeros(0, dtype=np.int64), np.zeros((0, nx + m + 1), dtype=dtype), np.zeros((0, nx), dtype=dtype), np.zeros(0), np.zeros((0, 3), dtype=np.int64)
    return np.concatenate(reg), np.concatenate(Phi), np.concatenate(Gt), np.concatenate(mar), np.concatenate(where)


def sums(adds, q, v, w, Ts, dtype=LD):
    """dict: region, margin (the least over the searches), and per point the lists G, R, Q, S, absG, absR (the sums of the absolute
    terms the bound is stated on)."""
    reg, Phi, Gt, mar, where = samples(adds, q, v, w, Ts, dtype)
    P = np.asarray(q).shape[0]
    out = dict(region=reg, where=where, margin=float(mar.min()) if mar.size else np.inf, G=[], R=[], Q=[], S=[], absG=[], absR=[])
    for p in range(P):
        sel = reg == p
        ph, g = Phi[sel], Gt[sel]
        out['G'].append(ph.T @ ph); out['R'].append(g.T @ ph); out['Q'].append((g * g).sum()); out['S'].append(int(sel.sum()))
        out['absG'].append(np.abs(ph).T @ np.abs(ph)); out['absR'].append(np.abs(g).T @ np.abs(ph))
    return out


def sums_constant(S):
    """(S + 4) eps, eps = 2^-53.  A term of G is a product of two entries of phi: x_i - x_p is rounded once, u_i and the constant are
    exact, so the term carries at most 2 roundings (the product itself is exact inside the FMA).  A term of R is g times an entry of
    phi: g = (x_{i+1} - x_i) / Ts carries 2 (the subtraction and the division), the entry of phi 1: 3.  The term then passes through at
    most S + 1 additions: those of the samples behind it in its own granule, one per granule behind its own in the reduce, and the
    one onto the running sum; every granule holds at least one sample of the point, so they are S at the most, over any number of add
    calls.  3 + 1 = 4."""
    return (S + 4) * EPS


def sums_use(got_G, got_R, ref, p):
    """The largest share of the entrywise bound that one point's device sums use against the long-double sums."""
    c = sums_constant(ref['S'][p])
    use = 0.0
    for got, k in ((got_G, 'G'), (got_R, 'R')):
        d, b = np.abs(np.asarray(got, dtype=LD) - ref[k][p]), c * ref['abs' + k][p]
        pos = b > 0
        assert not np.any(d[~pos] > 0), 'a sum whose terms all vanish must be zero'
        if pos.any():
            use = max(use, float((d[pos] / b[pos]).max()))
    return use


def solve(G, R, ridge=0.0, dtype=LD):
    """(X, kappa): R (D^-1/2 (D^-1/2 G D^-1/2 + ridge I)^-1 D^-1/2) by Cholesky in `dtype`, the scaled diagonal set to 1 + ridge, and the
    2-norm condition number of the equilibrated block (float64 of the long-double block)."""
    Gs = np.asarray(G, dtype=dtype)
    n = Gs.shape[0]
    d = 1 / np.sqrt(np.diag(Gs))
    M = Gs * d[:, None] * d[None, :]
    M[np.arange(n), np.arange(n)] = dtype(1) + dtype(ridge)
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        assert p > 0
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = (np.asarray(R, dtype=dtype) * d[None, :]).T.copy()
    for j in range(n):
        Z[j] = (Z[j] - L[j, :j] @ Z[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Z[j] = (Z[j] - L[j + 1:, j] @ Z[j + 1:]) / L[j, j]
    return Z.T * d[None, :], float(np.linalg.cond(M.astype(np.float64)))


def tables(s, q, v, m, points, ridge=0.0, dtype=LD):
    """dict A_c, B_c, d_c, u, c (lists over `points`) and kappa (the largest) of the sums `s`."""
    xp = np.hstack([np.asarray(v), np.asarray(q)]).astype(dtype)
    nx = xp.shape[1]
    out = dict(A_c=[], B_c=[], d_c=[], u=[], c=[], kappa=0.0)
    for p in points:
        X, kap = solve(s['G'][p], s['R'][p], ridge, dtype)
        A, B, c = X[:, :nx], X[:, nx:nx + m], X[:, nx + m]
        out['A_c'].append(A); out['B_c'].append(B); out['c'].append(c); out['d_c'].append(c - A @ xp[p])
        out['u'].append(np.asarray(s['G'][p], dtype=dtype)[nx:nx + m, nx + m] / dtype(s['S'][p]))
        out['kappa'] = max(out['kappa'], kap)
    return out
