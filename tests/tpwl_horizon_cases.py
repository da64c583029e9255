"""Seeded cases for the tests of the TPWL horizon error: known models (the structure of tpwl_fit_cases.known_model) and records rolled
out by their generating map with a small process noise, so that the k-step error is neither zero nor large.  No GPU and no product import.

A case: name -> (model, E, T, H, stride, every).  The models: 'n4' the smallest (n_x = 4, m = 1, P = 1); 'n12' (n_x = 12,
m = 3, P = 7, w_v = 0: the held search) with starts spread over the points, so that windows cross regions; 'n12v' the same tables with
w_v != 0 (the general search); 'p65' P = 65 points (one more than a wave holds); 'r33' r = 33 (n_x = 66: one more than the held search
takes); 'n84' n_x = 84, m = 4 (above the rollout's 64 KB staged limit); 'n128' n_x = 128, m = 16 (the plant limits; 'n128l2' at a horizon
beyond which the unit's staged layout no longer fits)."""
import numpy as np

import tpwl_fit_cases as fc
import tpwl_fit_reference as fr

TS = fc.TS
_cache = {}

# name -> (r, m, P, spacing, (w_q, w_v), n_z)
MODELS = {
    'n4': (2, 1, 1, 0.6, (1.0, 0.0), 2),
    'n12': (6, 3, 7, 0.6, (1.0, 0.0), 6),
    'n12v': (6, 3, 7, 0.6, (1.0, 0.3), 6),
    'p65': (4, 3, 65, 0.6, (1.0, 0.0), 3),
    'r33': (33, 2, 5, 0.15, (1.0, 0.0), 3),
    'n84': (42, 4, 4, 0.15, (1.0, 0.0), 3),
    'n128': (64, 16, 3, 0.1, (1.0, 0.0), 2),
}
# name -> (model, E, T, H, stride, every)
CASES = {
    'n4': ('n4', 1, 2, 1, 1, 1),
    'n12': ('n12', 7, 38, 9, 1, 2),
    'n12v': ('n12v', 5, 38, 9, 1, 2),
    'p65': ('p65', 4, 24, 6, 1, 2),
    'r33': ('r33', 2, 17, 5, 1, 1),
    'n84': ('n84', 2, 12, 4, 1, 2),
    'n128': ('n128', 2, 9, 3, 1, 2),
    'n12s3': ('n12', 5, 38, 4, 3, 1),           # T = 38 is no multiple of s = 3: T' = 13
    'n128l2': ('n128', 1, 143, 141, 1, 2),      # H = 141: the staged layout plus the accumulators pass 160 KB, the L2-fed step; one window
}


def model(name):
    if ('m', name) in _cache:
        return _cache[('m', name)]
    r, m, P, spacing, (wq, wv), nz = MODELS[name]
    if name == 'n12v':
        mdl = dict(model('n12'))
        mdl['v'] = 0.2 * spacing * np.random.default_rng(81).standard_normal((P, r))
        mdl['w'], mdl['name'] = {'q': wq, 'v': wv}, name
    else:
        rng = np.random.default_rng(5300 + 2 * r + m + P)
        q = spacing * rng.standard_normal((P, r))
        v, u = np.zeros((P, r)), 0.5 * rng.standard_normal((P, m))
        A, B, d = np.zeros((P, 2 * r, 2 * r)), np.zeros((P, 2 * r, m)), np.zeros((P, 2 * r))
        for p in range(P):
            A[p, :r, :r], A[p, :r, r:], A[p, r:, :r] = -fc._spd(rng, r, 0.5, 2.0), -fc._spd(rng, r, 4.0, 40.0), np.eye(r)
            B[p, :r] = rng.standard_normal((r, m))
            d[p] = -A[p] @ np.concatenate([v[p], q[p]]) - B[p] @ u[p]
        mdl = dict(name=name, r=r, m=m, P=P, q=q, v=v, u=u, A_c=A, B_c=B, d_c=d, w={'q': wq, 'v': wv}, Ts=TS)
    mdl['n_z'] = nz
    _cache[('m', name)] = mdl
    return mdl


def output_matrix(mdl):
    """H (n_z x n_x), dense and seeded: what TPWL.set_output_model gives for Hf = output_Hf(mdl) under tests' rom_info (U = [I; 0])."""
    return np.random.default_rng(17 + mdl['r']).standard_normal((mdl['n_z'], 2 * mdl['r']))


def output_Hf(mdl):
    r, H = mdl['r'], output_matrix(mdl)
    Hf = np.zeros((mdl['n_z'], 6 * r))
    Hf[:, :r], Hf[:, 3 * r:4 * r] = H[:, :r], H[:, r:]
    return Hf


def records(mname, E, T, seed=0, noise=2e-3, spread=0.5, uamp=30.0):
    """(X (E, T, n_x), U (E, T, m)): episodes started at x_p + spread N(0, 1) (p = episode % P), stepped by the generating map under
    inputs u_p + uamp N(0, 1) drawn anew every step (large: the episodes cross regions), plus a process noise of `noise` N(0, 1) per
    step: the model's k-step error grows from it."""
    key = ('r', mname, E, T, seed, noise, spread, uamp)
    if key in _cache:
        return _cache[key]
    mdl = model(mname)
    r, m, P = mdl['r'], mdl['m'], mdl['P']
    rng = np.random.default_rng(7700 + seed)
    p0 = np.arange(E) % P
    x = np.hstack([mdl['v'][p0], mdl['q'][p0]]) + spread * MODELS[mname][3] * rng.standard_normal((E, 2 * r))
    X, U = np.zeros((E, T, 2 * r)), mdl['u'][p0][:, None, :] + uamp * rng.standard_normal((E, T, m))
    for i in range(T):
        X[:, i] = x
        p = fr.nearest(x, mdl['q'], mdl['v'], mdl['w'], np.float64)[0]
        x = x + mdl['Ts'] * (np.einsum('eij,ej->ei', mdl['A_c'][p], x) + np.einsum('eij,ej->ei', mdl['B_c'][p], U[:, i]) + mdl['d_c'][p])
        x = x + noise * rng.standard_normal(x.shape)
    _cache[key] = (X, U)
    return _cache[key]


def case(name):
    """dict(model, X, U, H, stride, every, Hm) of a case."""
    mname, E, T, H, stride, every = CASES[name]
    mdl = model(mname)
    X, U = records(mname, E, T)
    return dict(model=mdl, X=X, U=U, H=H, stride=stride, every=every, Hm=output_matrix(mdl))
