"""Seeded cases for the tests of the SSM horizon error.  No GPU and no product import.

Models: ssm_cases.model(shape) for the shapes that reach every in-kernel inverse path at the smallest size (ssm_cases.STAGED_SHAPES), plus
(17, 4, 2, 1) (the un-gathered loop) and (32, 8, 1, 1) (the n_x limit), plus 'shipped': the reference's shipped Diamond model of golden g17
(n_x = n_o = 6, m = 4, cubic).
Records of a synthetic shape: a perturbed copy of the model (ssm_loop_cases.plant_model: the coefficients mixed by MIX = 0.02 towards
another model) stepped by its discrete map from x0 = 0.3 N(0, 1) under inputs 0.5 N(0, 1), measured by y = C_plant(x) + z_ref + 1e-3
N(0, 1): the model's errors are then not zero and the maxima are decided by more than rounding.  The shipped model reads the
reference's own record (g17: z_true_qv, u_interp), windows every 49 rows.  H <= 12 everywhere (test_ssm_horizon_reference_cpu.py holds
e_np <= ssm_cases.E_ORACLE_MAX on every case).  Whatever the functions return is cached: treat it as read-only."""
import os

import numpy as np

import ssm_cases as sc
import ssm_horizon_reference as shr
import ssm_loop_cases as slc
from oracle import ssm as ossm

HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = 'shipped'
SHAPES = list(sc.STAGED_SHAPES) + [(17, 4, 2, 1), (32, 8, 1, 1), SHIPPED]
BLOCK = 16               # windows of a block at these sizes (the plan reports it; the GPU and surface tests assert it)
NOISE = 1e-3
# name -> (shape, E, T, H, stride, every, modes: labels of ssm_cases.DISCRETE or None for all)
CASES = {}
for _s in SHAPES:
    CASES['m-' + (_s if _s == SHIPPED else sc.shape_id(_s))] = (_s, 1, 1002, 12, 1, 49, None) if _s == SHIPPED else (_s, 2, 14, 5, 1, 2, None)
EDGE = (5, 5, 3, 3)      # a cubic chart: C_map(W_map(.)) is not the identity, so row 0 of ez is not rounding
CASES.update({
    'e1-b15': (EDGE, 1, 18, 3, 1, 1, ('be@0.01',)),          # windows per episode = block - 1
    'e1-b16': (EDGE, 1, 19, 3, 1, 1, ('be@0.01',)),          # = block
    'e3-b17': (EDGE, 3, 20, 3, 1, 1, ('be@0.01',)),          # = block + 1: two blocks per episode, three episodes
    'e3-one': (EDGE, 3, 4, 3, 1, 1, ('map',)),               # T' = H + 1: exactly one window per episode
    's3': (EDGE, 2, 38, 4, 3, 1, ('fe@0.01',)),              # T = 38 is no multiple of s = 3: T' = 13
    'w2': (EDGE, 1, 30, 4, 1, 2, ('bil@0.05',)),
    'w5': (EDGE, 1, 30, 4, 1, 5, ('bil@0.05',)),
    'h1': (EDGE, 2, 6, 1, 1, 1, ('be@0.05',)),               # H = 1
})
MODES = {m[0]: m for m in sc.DISCRETE}


def modes_of(name):
    return [m for m in sc.DISCRETE if CASES[name][6] is None or m[0] in CASES[name][6]]


def case_modes():
    return [(name, m[0]) for name in sorted(CASES) for m in modes_of(name)]


@sc.cached
def golden():
    g = np.load(os.path.join(HERE, 'golden', 'g17_ssm_hardware.npz'))
    return {k: g[k] for k in g.files}


@sc.cached
def model(shape):
    """The float64 coefficient arrays of a shape in the layout of ssm_cases.model."""
    if shape != SHIPPED:
        return sc.model(shape)
    g = golden()
    i = lambda k: int(g['params_' + k][0, 0])
    return dict(n=i('state_dim'), m=i('input_dim'), n_o=i('output_dim'), rom_order=i('ROM_order'), ssm_order=i('SSM_order'), R=g['model_r_coeff'],
                B=g['model_B'], W=g['model_w_coeff'], V=g['model_v_coeff'], z_ref=g['z_eq'], Rd=g['model_rd_coeff'], Bd=g['model_Bd'])


@sc.cached
def records(shape, E, T):
    """(Y (E, T, n_o), U (E, T, m)) in float64."""
    if shape == SHIPPED:
        g = golden()
        assert (E, T) == (1, g['z_true_qv'].shape[0])
        return g['z_true_qv'][None].copy(), g['u_interp'][None].copy()
    n, m = shape[0], shape[1]
    Mp = sc.oracle_model(slc.plant_model(shape))
    rng = np.random.default_rng(8800 + 7 * n + E + T)
    x = 0.3 * rng.standard_normal((E, n))
    U, Y = 0.5 * rng.standard_normal((E, T, m)), np.zeros((E, T, n))
    for i in range(T):
        for e in range(E):
            Y[e, i] = ossm.observe(Mp, x[e]) + Mp['z_ref'] + NOISE * rng.standard_normal(n)
            x[e] = ossm.dynamics(Mp, x[e], U[e, i], True)
    assert np.isfinite(Y).all()
    return Y, U


def linear_chart(name):
    """True where the ssm basis has order 1: V is then the inverse of W, C_map(W_map(y)) = y up to rounding, and row 0 of ez is rounding
    alone (its maximum is not decided by the data)."""
    return case(name)['d']['ssm_order'] == 1


def case(name):
    shape, E, T, H, stride, every, _ = CASES[name]
    Y, U = records(shape, E, T)
    return dict(shape=shape, d=model(shape), Y=Y, U=U, H=H, stride=stride, every=every)


@sc.cached
def reference(name, label):
    """(the long-double chain, the float64 restatement) of a case in a mode: the dicts of ssm_horizon_reference.predict."""
    c = case(name)
    _, _, method, dt = MODES[label]
    args = (method, dt, c['Y'], c['U'], c['H'], c['stride'], c['every'])
    return shr.predict(sc.reference_model(c['d']), *args, dtype=shr.LD), shr.predict(sc.oracle_model(c['d']), *args, dtype=np.float64)


def e_np(ld, f8):
    """{quantity: the float64 restatement's distance from the long-double chain relative to the largest entry} for x_obs, x_pred, z_pred,
    sse_x, sse_z."""
    cl = shr.curves(ld['x_pred'], ld['z_pred'], ld['Xow'], ld['Yw'], ld['status'])
    ex, ez = f8['x_pred'] - f8['Xow'], f8['z_pred'] - f8['Yw']
    own = dict(x_obs=f8['x_obs'], x_pred=f8['x_pred'], z_pred=f8['z_pred'], sse_x=(ex * ex).sum(axis=(0, 2)), sse_z=(ez * ez).sum(axis=(0, 2)))
    ref = dict(x_obs=ld['x_obs'], x_pred=ld['x_pred'], z_pred=ld['z_pred'], sse_x=cl['sse_x'], sse_z=cl['sse_z'])
    return {k: shr.rel_err(own[k], ref[k]) for k in own}, ref
