"""Seeded cases of the observed closed loop, shared by tests/test_clobs_reference_cpu.py (input conditions, without a GPU) and
tests/test_gusto_loop_observer_gpu.py (the kernels of csrc/gusto_loop.hip and csrc/observer.hip on the same numbers).

Models are those of tests/cl_cases.py (golden_problem), with one more at the Diamond's r = 30: n_x = 8 (the filter's VALU path), 60
(MFMA <60>) and 72 (wide).  The plans, plant states, gains and disturbances of an advance case are cl_cases.advance_case's; the
measurement model (dense C / sqrt(n_x), y_ref), the filter's W, V, Sigma0 (ekf_cases.spd at the scaling 100, 1, 1), the wrong initial
estimate and the measurement noise are drawn here.  The filter's model is either the plant's own or a mismatched copy: the same points
with B_c scaled by 1.05 and d_c by 0.95, discretised at dt_sim like the plant."""
import numpy as np

import cl_cases as cc
import clobs_reference as cor
import ekf_cases as ec
from oracle import tpwl as otpwl

cc.MODELS.setdefault('r30', (30, 4, 8, 40, 35, 0.2))        # n_x = 60: the Diamond shape (cl_cases.model / tables serve it like the others)

B = 3
N_Y = {'g6': 6, 'r30': 30, 'r36': 30}

# (name, model, filter model is the plant's, dt_sim, n_keep, gains, disturbance, measurement noise, seed)
CASES = [
    ('g6-knots-1', 'g6', True, 0.05, 1, False, False, False, 1),
    ('g6-frac-3', 'g6', False, 0.03, 3, True, True, True, 2),
    ('g6-knots-3-exact', 'g6', True, 0.05, 3, True, False, False, 3),
    ('r30-knots-3', 'r30', True, 0.05, 3, True, False, True, 4),
    ('r30-frac-1', 'r30', False, 0.03, 1, True, True, True, 5),
    ('r36-frac-3', 'r36', True, 0.03, 3, True, True, True, 6),
    ('r36-knots-1', 'r36', False, 0.05, 1, False, True, False, 7),
]
IDS = [c[0] for c in CASES]

# seeds replaced because the default one misses an input condition (tests/test_clobs_reference_cpu.py): a lookup within MARGIN of a
# second point, or e_oracle above E_ORACLE_MAX
SEEDS = {}

_cache = {}


def mismatched_model(mname):
    """The filter's model where it is not the plant's: same points, B_c * 1.05, d_c * 0.95."""
    if ('mis', mname) not in _cache:
        mdl = dict(cc.model(mname)['model'])
        mdl['B_c'] = 1.05 * np.asarray(mdl['B_c'])
        mdl['d_c'] = 0.95 * np.asarray(mdl['d_c'])
        _cache[('mis', mname)] = mdl
    return _cache[('mis', mname)]


def filter_tables(mname, same, dt_sim):
    """dict q, v, w_q, w_v, A_d, B_d, d_d of the filter's model at dt_sim."""
    if same:
        return cc.table_dict(mname, dt_sim)
    key = ('mis-tab', mname, float(dt_sim))
    if key not in _cache:
        _cache[key] = otpwl.pre_discretize(mismatched_model(mname), dt_sim, 'zoh')
    mdl = mismatched_model(mname)
    Ad, Bd, dd = _cache[key]
    return dict(q=mdl['q'], v=mdl['v'], w_q=mdl['w_q'], w_v=mdl['w_v'], A_d=Ad, B_d=Bd, d_d=dd)


def measurement(mname):
    """C, y_ref, W, V, Sigma0 of a model (one per model: the loops and the advance cases share it)."""
    if ('meas', mname) not in _cache:
        n, ny = 2 * cc.MODELS[mname][0], N_Y[mname]
        rng = np.random.default_rng(5000 + n)
        C = rng.standard_normal((ny, n)) / np.sqrt(n)
        y_ref = rng.standard_normal(ny)
        sw, sv, s0 = ec.SCALINGS[0]
        _cache[('meas', mname)] = dict(C=C, y_ref=y_ref, W=ec.spd(n, sw, rng), V=ec.spd(ny, sv, rng), Sigma0=ec.spd(n, s0, rng), ny=ny)
    return _cache[('meas', mname)]


def case(cs):
    """The inputs of a CASES row: cl_cases.advance_case's xopt, uopt, x, K, W, j, theta plus x_hat (B, n), V (n_keep, B, n_y) or None."""
    if cs[0] not in _cache:
        name, mname, same, dt_sim, n_keep, gains, dist, noise, seed = cs
        seed = SEEDS.get(name, seed)
        c = dict(cc.advance_case((name, mname, B, dt_sim, n_keep, gains, dist, 100 + seed)))
        n, ny = c['x'].shape[1], N_Y[mname]
        rng = np.random.default_rng(7000 + seed)
        scale = np.abs(cc.model(mname)['model']['q']).max()
        exact = name.endswith('exact')
        c['x_hat'] = c['x'].copy() if exact else c['x'] + 0.02 * scale * rng.standard_normal((B, n))
        c['V'] = 0.05 * rng.standard_normal((n_keep, B, ny)) if noise else None
        _cache[cs[0]] = c
    return _cache[cs[0]]


def reference(cs, dtype, H=None):
    """The observed advance of every member in `dtype`: dict of stacked X, U, Z, Xhat, Y (B, n_keep, .), idx_* (B, n_keep), margin."""
    name, mname, same, dt_sim, n_keep, gains, dist, noise, seed = cs
    c, ms = case(cs), measurement(mname)
    planner, plant, filt = cc.table_dict(mname), cc.table_dict(mname, dt_sim), filter_tables(mname, same, dt_sim)
    H = cc.model(mname)['H'] if H is None else H
    outs = [cor.observed_advance(planner, plant, filt, H, ms['C'], ms['y_ref'], ms['W'], ms['V'], c['K'], c['xopt'][b], c['uopt'][b], c['x'][b],
                                 c['x_hat'][b], ms['Sigma0'], c['j'], c['theta'], None if c['W'] is None else c['W'][:, b],
                                 None if c['V'] is None else c['V'][:, b], dtype) for b in range(B)]
    res = {k: np.stack([o[k] for o in outs]) for k in outs[0] if k != 'margin'}
    res['margin'] = min(o['margin'] for o in outs)
    return res


FIELDS = ('X', 'U', 'Z', 'Xhat', 'Y')
_refs = {}


def measured(cs, H=None):
    """(long-double reference, e_oracle = the float64 statement against it over all sub-steps and fields) -- computed once per case for the
    default H; with the product's own H (the GPU test) computed again."""
    key = (cs[0], None if H is None else H.tobytes())
    if key not in _refs:
        ref, f64 = reference(cs, cor.LD, H), reference(cs, np.float64, H)
        for k in ('idx_plant', 'idx_gain', 'idx_filter'):
            assert np.array_equal(ref[k], f64[k]), (cs[0], k)
        _refs[key] = (ref, max(cor.err(f64[k], ref[k]) for k in FIELDS))
    return _refs[key]
