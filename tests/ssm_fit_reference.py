"""The SSM fit ("SSM model identification") as its definition states it, in np.longdouble on float64 records, the known
models the tests fit, and their records from the numpy oracle (oracle/ssm.py).  No GPU and no product import.

  kept rows 0, s, 2s, ..; x_i = V^T (y_i - y_ref); samples: interior rows 1 <= i <= T' - 2 inside an episode;
  Phi_i = [phi(x_i); u_i], phi the graded monomials up to P = max(ROM_order, SSM_order);
  G = sum Phi Phi^T, R_d = sum x_{i+1} Phi_i^T, R_c = sum ((x_{i+1} - x_{i-1}) / (2 Ts)) Phi_i^T, R_w = sum (y_i - y_ref) phi(x_i)^T;
  a block S of columns is solved as (D^-1/2 G_S D^-1/2 + ridge I) z = D^-1/2 r, coeff = D^-1/2 z, D = diag(G_S)."""
import os

import numpy as np

from oracle import ssm as ossm

LD = np.longdouble
EPS = 2.0 ** -53
TR = 64
HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (n_x, n_y, m, ROM_order, SSM_order, n): one partial tile; two tiles, the second partial, ROM_order != SSM_order; the shipped shape
SHAPES = {'n6': (2, 3, 1, 2, 2, 6), 'n21': (3, 5, 2, 3, 2, 21), 'n87': (6, 6, 4, 3, 3, 87)}
TS = 0.01
_cache = {}


def nmon(dim, order):
    return ossm.exponents(dim, order).shape[0]


def known_model(name):
    """A consistent model: V with orthonormal columns, w_coeff = [V | N K] with N orthogonal to V (so V^T W phi(x) = x exactly in exact
    arithmetic), rd_coeff / Bd contractive.  n87 takes the shipped Diamond model's rd_coeff and Bd (golden g17): its rollout under the
    inputs of `records` stays bounded (|x| < 1.2e3 over 70 steps, linear part of spectral radius 0.966; checked on the CPU by
    tests/test_ssm_fit_surface_cpu.py), so it is used unscaled."""
    if name in _cache:
        return _cache[name]
    nx, ny, m, ro, so, _ = SHAPES[name]
    rng = np.random.default_rng(700 + nx)
    Q, _ = np.linalg.qr(rng.standard_normal((ny, ny)))
    V, N = np.ascontiguousarray(Q[:, :nx]), Q[:, nx:]
    n_ssm, n_rom = nmon(nx, so), nmon(nx, ro)
    W = np.zeros((ny, n_ssm))
    W[:, :nx] = V
    if ny > nx and so > 1:
        W[:, nx:] = N @ (0.3 * rng.standard_normal((ny - nx, n_ssm - nx)))
    if name == 'n87':
        g = np.load(os.path.join(HERE, 'golden', 'g17_ssm_hardware.npz'))
        Rd, Bd, amp, x0 = g['model_rd_coeff'].copy(), g['model_Bd'].copy(), 200.0, 1.0
    else:
        A, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        Rd = np.hstack([0.9 * A, 0.01 * rng.standard_normal((nx, n_rom - nx))])
        Bd, amp, x0 = 0.3 * rng.standard_normal((nx, m)), 1.0, 0.5
    y_ref = rng.uniform(-2.0, 2.0, ny)
    Vc = np.zeros((nx, nmon(ny, so)))
    Vc[:, :ny] = V.T                                # v_coeff = [V^T | 0] over the basis of n_y variables
    model = ossm.make_model(nx, m, ro, so, np.zeros((nx, n_rom)), np.zeros((nx, m)), W, Vc, y_ref, Rd, Bd)
    _cache[name] = dict(name=name, V=V, N=N, W=W, Rd=Rd, Bd=Bd, y_ref=y_ref, oracle=model, amp=amp, x0=x0, nx=nx, ny=ny, m=m, ro=ro, so=so)
    return _cache[name]


def records(name, E, T, seed, scale=1.0):
    """(Y (E, T, n_y), U (E, T, m), X (E, T, n_x)) of E oracle rollouts of the known model in its discrete map: random x0, inputs drawn
    anew every step (uniform in [0, amp] for n87, the shipped model's pressures; in [-amp, amp] otherwise).  Row i of U is the input
    applied after y_i; the last row's is never used.  `scale` shrinks x0 and the inputs alike."""
    key = (name, E, T, seed, scale)
    if key not in _cache:
        k = known_model(name)
        rng = np.random.default_rng(seed)
        Y, U, X = np.zeros((E, T, k['ny'])), np.zeros((E, T, k['m'])), np.zeros((E, T, k['nx']))
        for e in range(E):
            U[e] = scale * rng.uniform(0.0 if name == 'n87' else -k['amp'], k['amp'], (T, k['m']))
            x, z = ossm.rollout(k['oracle'], scale * k['x0'] * rng.standard_normal(k['nx']), U[e, :T - 1], TS, discrete=True)
            Y[e], X[e] = z, x
        _cache[key] = (Y, U, X)
    return _cache[key]


def lift(x, exps, dtype=LD):
    out = np.ones((x.shape[0], exps.shape[0]), dtype=dtype)
    for k in range(exps.shape[0]):
        for j in np.flatnonzero(exps[k]):
            for _ in range(int(exps[k, j])):
                out[:, k] = out[:, k] * x[:, j]
    return out


def samples(adds, V, y_ref, P, Ts, dtype=LD):
    """(Phi (S, n), X1 (S, n_x), Xm (S, n_x), DY (S, n_y)) over the samples of `adds` = [(Y, U, stride), ..]: the regressor, x_{i+1},
    x_{i-1} and y_i - y_ref."""
    nx, ny = V.shape[1], V.shape[0]
    exps = ossm.exponents(nx, P)
    m = adds[0][1].shape[2]
    Phi, X1, Xm, DY = [np.zeros((0, exps.shape[0] + m), dtype=dtype)], [np.zeros((0, nx), dtype=dtype)], [np.zeros((0, nx), dtype=dtype)], \
        [np.zeros((0, ny), dtype=dtype)]
    Vl, rl = V.astype(dtype), y_ref.astype(dtype)
    for Y, U, stride in adds:
        for e in range(Y.shape[0]):
            dy = Y[e, ::stride].astype(dtype) - rl
            if dy.shape[0] < 3:
                continue
            x = dy @ Vl
            Phi.append(np.hstack([lift(x[1:-1], exps, dtype), U[e, ::stride][1:-1].astype(dtype)]))
            X1.append(x[2:]); Xm.append(x[:-2]); DY.append(dy[1:-1])
    return np.concatenate(Phi), np.concatenate(X1), np.concatenate(Xm), np.concatenate(DY)


def sums(adds, V, y_ref, P, Ts, dtype=LD):
    """dict G, Rd, Rc, Rw, Q (3), samples, and absG, absRd, absRc, absRw, absQ: the sums of the absolute terms the bounds are stated on.
    The central difference counts as two terms, x_{i+1} / (2 Ts) and x_{i-1} / (2 Ts)."""
    Phi, X1, Xm, DY = samples(adds, V, y_ref, P, Ts, dtype)
    nmono = Phi.shape[1] - adds[0][1].shape[2]
    two = dtype(2) * dtype(Ts)
    Xc, Xca, aP = (X1 - Xm) / two, (np.abs(X1) + np.abs(Xm)) / two, np.abs(Phi)
    return dict(G=Phi.T @ Phi, Rd=X1.T @ Phi, Rc=Xc.T @ Phi, Rw=DY.T @ Phi[:, :nmono], samples=Phi.shape[0],
                Q=np.array([(X1 * X1).sum(), (Xc * Xc).sum(), (DY * DY).sum()]), absG=aP.T @ aP, absRd=np.abs(X1).T @ aP, absRc=Xca.T @ aP,
                absRw=np.abs(DY).T @ aP[:, :nmono], absQ=np.array([(X1 * X1).sum(), (Xca * Xca).sum(), (DY * DY).sum()]))


def sums_constant(S, P):
    """(S + 4 P + 2) eps.  A term of a sum is a product of chart coordinates: x is the exact V^T (y - y_ref) rounded once; a monomial of
    degree g carries g such roundings and g - 1 of its products, 2 g - 1; a term of G is a product of two monomials, at most 4 P - 2
    (the product itself is exact inside the FMA); a term of R_d is x_{i+1} times a monomial, 2 P; of R_c the same with the subtraction
    and the division, 2 P + 2, each relative to its own |x| / (2 Ts); of R_w (y - y_ref), one rounding, times a monomial, 2 P.  A term
    then passes through at most S + 1 additions: those of its own workgroup's samples and the workgroups behind it in the reduce, and
    every workgroup holds a sample.  4 P + 2 covers the largest of these and the + 1."""
    return (S + 4 * P + 2) * EPS


def sums_use(got, ref, P):
    """The largest share of the elementwise bound that the device sums `got` use against the long-double sums `ref`, per sum."""
    c = sums_constant(ref['samples'], P)
    use = {}
    for k in ('G', 'Rd', 'Rc', 'Rw'):
        d, b = np.abs(np.asarray(got[k], dtype=LD) - ref[k]), c * ref['abs' + k]
        pos = b > 0
        assert not np.any(d[~pos] > 0), 'a sum whose terms all vanish must be zero'
        use[k] = float((d[pos] / b[pos]).max()) if pos.any() else 0.0
    return use


def block(name):
    """(dynamics columns, observation columns) of Phi."""
    nx, ny, m, ro, so, n = SHAPES[name]
    return list(range(nmon(nx, ro))) + list(range(n - m, n)), list(range(nmon(nx, so)))


def solve(G, R, cols, ridge=0.0, dtype=LD):
    """(X, kappa): R[:, cols] (D^-1/2 (D^-1/2 G_S D^-1/2 + ridge I)^-1 D^-1/2) by Cholesky in `dtype`, and the 2-norm condition number of
    the equilibrated block (float64 of the long-double block)."""
    Gs = np.asarray(G, dtype=dtype)[np.ix_(cols, cols)]
    d = 1 / np.sqrt(np.diag(Gs))
    M = Gs * d[:, None] * d[None, :] + dtype(ridge) * np.eye(len(cols), dtype=dtype)
    n = M.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        assert p > 0
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = (np.asarray(R, dtype=dtype)[:, cols] * d[None, :]).T.copy()
    for j in range(n):
        Z[j] = (Z[j] - L[j, :j] @ Z[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Z[j] = (Z[j] - L[j + 1:, j] @ Z[j + 1:]) / L[j, j]
    return Z.T * d[None, :], float(np.linalg.cond(M.astype(np.float64)))
