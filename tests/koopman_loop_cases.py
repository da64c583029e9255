"""Seeded cases of the batched closed-loop Koopman MPC shared by tests/test_koopman_loop_reference_cpu.py (input conditions, without a
GPU) and tests/test_koopman_loop_gpu.py (the kernels of csrc/koopman_loop.hip on the same numbers).

The plants are the models of cl_cases.MODELS at dt_sim = Ts / r (Ts = 0.05), measured by a seeded y = C x + y_ref.  The Koopman models are
the shipped Diamond model (tests/golden/g22_koopman.npz; four inputs, so it stands on the r36 plant alone) and seeded synthetic ones
whose n_u is the plant's: with two delays, with a W truncation, and without the constant observable (dmd).  Every (plant, model kind)
pair that exists has a case; the other rows of the table -- r in {1, 5}, rollout_horizon in {1, 3, N}, B in {1, 3, 260}, with and
without W / V, replay with and without U_applied -- are spread over them so that every value is met by several cases, of every plant
where the plant takes part.  Plans are seeded scaled inputs whose raw values lie in the range the plants' own cases use."""
import os

import numpy as np

import cl_cases as cc
import koopman_loop_reference as kr

TS, N = 0.05, 5
DT_SIM = {1: 0.05, 5: 0.01}            # Ts / r, as the plants' tables are keyed
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_koopman.npz')

# name -> (n_y, m, delays, degree, dmd, rows of W or None, seed); 'ship' is the golden file's
SPECS = {
    'ship': None,
    'syn2-g6': (2, 3, 2, 2, False, None, 1),            # 12 zeta entries: 91 observables
    'syn2-r36': (1, 4, 2, 2, False, None, 2),           # 11: 78
    'syn2-m8': (1, 8, 2, 2, False, 24, 3),              # 19: 210, W to 24 is mandatory for the QP limit
    'w-g6': (3, 3, 1, 2, False, 20, 4),                 # 9: 55 -> 20
    'w-r36': (3, 4, 1, 2, False, 30, 5),                # the shipped shape: 66 -> 30
    'w-m8': (3, 8, 1, 2, False, 24, 6),                 # 14: 120 -> 24, mandatory
    'dmd-g6': (3, 3, 1, 2, True, None, 7),              # 54
    'dmd-r36': (3, 4, 1, 2, True, None, 8),             # 65
    'dmd-m8': (3, 8, 1, 2, True, 24, 9),                # 119 -> 24, mandatory
}

# (name, plant, model, r, rollout_horizon, batch, W, V, mode: 'sim' | 'replay' | 'replay-u', seed)
ADVANCE = [
    ('r36-ship-5-1', 'r36', 'ship', 5, 1, 3, True, True, 'sim', 1),
    ('r36-ship-1-N', 'r36', 'ship', 1, N, 3, False, False, 'sim', 2),
    ('r36-ship-replay', 'r36', 'ship', 5, 3, 3, False, False, 'replay', 3),
    ('r36-ship-replay-u', 'r36', 'ship', 5, 1, 1, False, False, 'replay-u', 4),
    ('g6-syn2-5-3', 'g6', 'syn2-g6', 5, 3, 3, True, False, 'sim', 5),
    ('g6-syn2-260', 'g6', 'syn2-g6', 1, 3, 260, True, True, 'sim', 6),                # more members than CUs
    ('r36-syn2-1-1', 'r36', 'syn2-r36', 1, 1, 1, False, True, 'sim', 7),
    ('m8-syn2-5-N', 'm8', 'syn2-m8', 5, N, 3, True, True, 'sim', 8),
    ('g6-w-1-N', 'g6', 'w-g6', 1, N, 3, False, True, 'sim', 9),
    ('r36-w-5-3', 'r36', 'w-r36', 5, 3, 3, True, True, 'sim', 10),
    ('m8-w-1-1', 'm8', 'w-m8', 1, 1, 3, True, False, 'sim', 11),
    ('g6-dmd-5-1', 'g6', 'dmd-g6', 5, 1, 1, False, False, 'sim', 12),
    ('r36-dmd-1-3', 'r36', 'dmd-r36', 1, 3, 3, True, True, 'sim', 13),
    ('m8-dmd-replay-u', 'm8', 'dmd-m8', 5, 3, 3, False, False, 'replay-u', 14),
    ('g6-dmd-replay', 'g6', 'dmd-g6', 1, 1, 3, False, False, 'replay', 15),
    ('m8-dmd-5-3', 'm8', 'dmd-m8', 5, 3, 3, False, False, 'sim', 16),
]

RECORDS = ('X', 'Y', 'U', 'ring')
_cache = {}


def golden():
    if 'golden' not in _cache:
        _cache['golden'] = dict(np.load(GOLDEN))
    return _cache['golden']


def spec(key):
    """dict n_y, m, delays, degree, dmd, y_offset, y_factor, u_offset, u_factor (1-D), W (n_w, n_psi) or None, A (n_lift, n_lift), B, H
    (n_y, n_lift), n_lift, n_psi of a Koopman model."""
    if ('spec', key) in _cache:
        return _cache[('spec', key)]
    if key == 'ship':
        g = golden()
        s = dict(n_y=3, m=4, delays=1, degree=2, dmd=False, W=None, A=g['model_A'], B=g['model_B'], H=g['model_C'],
                 **{k: np.ravel(g['scale_' + k]) for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')})
    else:
        ny, m, d, deg, dmd, nw, seed = SPECS[key]
        rng = np.random.default_rng(7000 + seed)
        nzeta = ny * (d + 1) + m * d
        P = len(kr.exponents(nzeta, deg, dmd))
        n = P if nw is None else nw
        W = None if nw is None else np.linalg.qr(rng.standard_normal((P, nw)))[0].T
        A = rng.standard_normal((n, n))
        A *= 0.9 / np.abs(np.linalg.eigvals(A)).max()
        s = dict(n_y=ny, m=m, delays=d, degree=deg, dmd=dmd, W=W, A=A, B=0.1 * rng.standard_normal((n, m)),
                 H=rng.standard_normal((ny, n)) / np.sqrt(n), y_offset=rng.uniform(-2.0, 2.0, ny), y_factor=rng.uniform(0.5, 3.0, ny),
                 u_offset=rng.uniform(20.0, 60.0, m), u_factor=rng.uniform(30.0, 80.0, m))
    nzeta = s['n_y'] * (s['delays'] + 1) + s['m'] * s['delays']
    s['n_psi'] = len(kr.exponents(nzeta, s['degree'], s['dmd']))
    s['n_lift'] = s['A'].shape[0]
    s['nzeta'] = nzeta
    _cache[('spec', key)] = s
    return s


def measurement(mname, ny, seed):
    """Seeded (C (n_y, n_plant), y_ref (n_y)) of a plant."""
    n = 2 * cc.MODELS[mname][0]
    rng = np.random.default_rng(8000 + 10 * n + ny + seed)
    return rng.standard_normal((ny, n)) / np.sqrt(n), rng.standard_normal(ny)


def advance_case(case):
    """The inputs of an ADVANCE row: dict spec, plant (tables or None), C, y_ref, uopt (B, N, m) scaled, x (B, n_plant), W (n_keep, B,
    n_plant) / V (n_keep, B, n_y) / Y_plant (B, n_keep + 1, n_y) / U_applied (B, n_keep, m) or None, r, n_keep, dt_sim."""
    name, mname, key, r, rh, B, dist, noise, mode, seed = case
    if ('case', name) in _cache:
        return _cache[('case', name)]
    s = spec(key)
    nk, dt_sim = rh * r, DT_SIM[r]
    ny, m = s['n_y'], s['m']
    assert m == cc.MODELS[mname][1], 'the model\'s inputs are the plant\'s'
    base = cc.advance_case((name, mname, B, dt_sim, nk, False, dist, 70 + seed))
    rng = np.random.default_rng(9000 + seed)
    scale = np.abs(cc.model(mname)['model']['q']).max()
    Cm, y_ref = measurement(mname, ny, seed)
    uopt = kr.scale_down(base['uopt'][:, :N], s['u_offset'], s['u_factor'], np.float64)
    replay = mode != 'sim'
    Yp = Ua = None
    if replay:
        Yp = y_ref + np.cumsum(0.05 * rng.standard_normal((B, nk + 1, ny)), axis=1)
    if mode == 'replay-u':
        Ua = rng.uniform(0.0, 100.0, (B, nk, m))
    c = dict(spec=s, plant=None if replay else cc.table_dict(mname, dt_sim), C=Cm, y_ref=y_ref, uopt=uopt, x=base['x'],
             W=base['W'] if not replay else None, V=0.01 * scale * rng.standard_normal((nk, B, ny)) if noise and not replay else None,
             Y_plant=Yp, U_applied=Ua, r=r, n_keep=nk, dt_sim=dt_sim)
    _cache[('case', name)] = c
    return c


def advance_reference(case, dtype):
    """The reference advance of every member, stacked: dict X (None in replay), Y, U, ring (B, n_keep, .), picks (B, n_keep), margin."""
    c = advance_case(case)
    B = c['uopt'].shape[0]
    outs = [kr.advance(c['spec'], c['plant'], c['C'], c['y_ref'], c['uopt'][b], c['x'][b], c['r'], c['n_keep'],
                       None if c['W'] is None else c['W'][:, b], None if c['V'] is None else c['V'][:, b],
                       None if c['Y_plant'] is None else c['Y_plant'][b], None if c['U_applied'] is None else c['U_applied'][b], dtype)
            for b in range(B)]
    res = {k: (None if outs[0][k] is None else np.stack([o[k] for o in outs])) for k in outs[0] if k != 'margin'}
    res['margin'] = min(o['margin'] for o in outs)
    return res


def e_oracle(case):
    """(e_oracle, long-double reference, float64 statement) of a case, cached: the worst record's distance."""
    name = case[0]
    if ('ref', name) not in _cache:
        ref, f64 = advance_reference(case, kr.LD), advance_reference(case, np.float64)
        _cache[('ref', name)] = (max(kr.err(f64[k], ref[k]) for k in RECORDS if ref[k] is not None), ref, f64)
    return _cache[('ref', name)]


def history(case, B):
    """Seeded raw samples in front of the first solve: y_hist (B, delays, n_y), u_hist (B, delays, m), u_prev0 (B, m), v0 (B, n_y)."""
    s = spec(case[2])
    rng = np.random.default_rng(9500 + case[-1])
    d = s['delays']
    return dict(y_hist=s['y_offset'] + s['y_factor'] * rng.uniform(-1.0, 1.0, (B, d, s['n_y'])), u_hist=rng.uniform(0.0, 100.0, (B, d, s['m'])),
                u_prev0=rng.uniform(0.0, 100.0, (B, s['m'])), v0=1e-3 * rng.standard_normal((B, s['n_y'])))


def fixup_case(B, n, m, seed):
    """Seeded plans, request states and status words for the fix-up kernel: every second member reports a failure."""
    rng = np.random.default_rng(9800 + seed)
    status = np.zeros(B, dtype=np.int32)
    status[1::2] = np.array([3, -7, 1, 2] * B)[:len(status[1::2])]
    return dict(xsol=rng.standard_normal((B, N + 1, n)), usol=rng.standard_normal((B, N, m)), x0=rng.standard_normal((B, n)),
                xprev=rng.standard_normal((B, N + 1, n)), uprev=rng.standard_normal((B, N, m)), status=status, u0=rng.uniform(0.0, 100.0, m))
