"""Seeded known TPWL models and their records for the tests of the TPWL fit.  No GPU and no product import.

A model has P points (q_p, v_p) and per point a mass-damping-stiffness block: with x = [v; q],
  A_p = [[-D_p, -K_p], [I, 0]], B_p = [[H_p], [0]], d_p = -A_p x_p - B_p u_p (x_p = [v_p; q_p] is an equilibrium under u_p),
D_p, K_p symmetric positive definite (K_p's spectrum in [4, 40], D_p's in [0.5, 2]: stable under forward Euler at Ts = 0.01).
Records are rolled out by x <- x + Ts (A_p x + B_p u + d_p), p the nearest point to x by the search rule (tpwl_fit_reference.nearest
in float64), in short episodes started near every point under inputs drawn anew every step."""
import numpy as np

import tpwl_fit_reference as fr

TS = 0.01
# name -> (r, m, P, point spacing, start spread, episodes per point, rows, (w_q, w_v)): n = 2 r + m + 1 = 12 (one partial tile), 16 and 17
# (the tile edge), 77 (the shipped Diamond shape r = 36 with m = 4), 128 (the largest the plan accepts)
CASES = {
    'n12': (4, 3, 7, 0.6, 0.5, 8, 41, (1.0, 0.0)),
    'n16': (6, 3, 5, 0.6, 0.5, 8, 41, (1.0, 0.3)),
    'n17': (6, 4, 5, 0.6, 0.5, 8, 41, (1.0, 0.0)),
    'n77': (36, 4, 8, 0.1, 0.3, 120, 5, (1.0, 0.0)),
    'n128': (60, 7, 2, 0.1, 0.3, 200, 3, (1.0, 0.0)),
}
_cache = {}


def _spd(rng, r, lo, hi):
    Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
    return (Q * rng.uniform(lo, hi, r)) @ Q.T


def known_model(name):
    if ('model', name) in _cache:
        return _cache[('model', name)]
    r, m, P, spacing, spread, epp, T, (wq, wv) = CASES[name]
    rng = np.random.default_rng(4700 + 2 * r + m)
    q = spacing * rng.standard_normal((P, r))
    v = 0.2 * spacing * rng.standard_normal((P, r)) if wv != 0.0 else np.zeros((P, r))
    u = 0.5 * rng.standard_normal((P, m))
    A, B, d = np.zeros((P, 2 * r, 2 * r)), np.zeros((P, 2 * r, m)), np.zeros((P, 2 * r))
    for p in range(P):
        A[p, :r, :r], A[p, :r, r:], A[p, r:, :r] = -_spd(rng, r, 0.5, 2.0), -_spd(rng, r, 4.0, 40.0), np.eye(r)
        B[p, :r] = rng.standard_normal((r, m))
        d[p] = -A[p] @ np.concatenate([v[p], q[p]]) - B[p] @ u[p]
    mdl = dict(name=name, r=r, m=m, P=P, q=q, v=v, u=u, A_c=A, B_c=B, d_c=d, w={'q': wq, 'v': wv}, Ts=TS)
    _cache[('model', name)] = mdl
    return mdl


def step(mdl, x, u):
    """One step of the generating map and the point it used."""
    p = int(fr.nearest(x[None], mdl['q'], mdl['v'], mdl['w'], np.float64)[0][0])
    return x + mdl['Ts'] * (mdl['A_c'][p] @ x + mdl['B_c'][p] @ u + mdl['d_c'][p]), p


def records(name, seed=0, epp=None, T=None):
    """(X (E, T, n_x), U (E, T, m), switches): epp episodes started near every point (x_p + spread N(0, 1)), inputs u_p0 + N(0, 1) drawn
    anew every step, p0 the starting point; switches = the changes of region inside the episodes."""
    r, m, P, spacing, spread, epp0, T0, _ = CASES[name]
    epp, T = epp or epp0, T or T0
    key = ('rec', name, seed, epp, T)
    if key in _cache:
        return _cache[key]
    mdl = known_model(name)
    rng = np.random.default_rng(9100 + seed)
    E = P * epp
    X, U, switches = np.zeros((E, T, 2 * r)), np.zeros((E, T, m)), 0
    for e in range(E):
        p0 = e % P
        x = np.concatenate([mdl['v'][p0], mdl['q'][p0]]) + spread * rng.standard_normal(2 * r)
        U[e] = mdl['u'][p0] + rng.standard_normal((T, m))
        last = None
        for i in range(T):
            X[e, i] = x
            x, p = step(mdl, x, U[e, i])
            switches += int(last is not None and i < T - 1 and p != last)
            last = p
    _cache[key] = (X, U, switches)
    return _cache[key]


def reference(name, seed=0, dtype=fr.LD):
    """The sums of the case's records in `dtype` (computed once per dtype)."""
    key = ('ref', name, seed, np.dtype(dtype).name)
    if key not in _cache:
        mdl = known_model(name)
        X, U, _ = records(name, seed)
        _cache[key] = fr.sums([(X, U, 1)], mdl['q'], mdl['v'], mdl['w'], mdl['Ts'], dtype)
    return _cache[key]


def counted_records(mdl, counts, seed=3, jitter=0.05):
    """(X (E, 2, n_x), U (E, 2, m)): episodes of two rows, hence one sample each, counts[p] of them started at x_p + jitter N(0, 1) --
    nearer to point p than to any other for the models here (the reference states the assignment; this only aims) -- in an order
    shuffled over the points; the second row is a step of the generating map."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(np.repeat(np.arange(mdl['P']), counts))
    r, m = mdl['r'], mdl['m']
    X, U = np.zeros((order.size, 2, 2 * r)), rng.standard_normal((order.size, 2, m))
    for e, p in enumerate(order):
        X[e, 0] = np.concatenate([mdl['v'][p], mdl['q'][p]]) + jitter * rng.standard_normal(2 * r)
        X[e, 1] = step(mdl, X[e, 0], U[e, 0])[0]
    return X, U
