"""Seeded cases of the SSM closed loop on a TPWL plant, shared by tests/test_ssm_loop_tpwl_reference_cpu.py (input conditions, without a
GPU) and tests/test_gusto_ssm_loop_tpwl_gpu.py (ssm_loop_advance_tpwl_kernel on the same numbers).

A case pairs an entry of cl_cases.ADVANCE -- its plant tables at dt_sim, x, uopt, W, j, theta; the plan's states and gains are ignored: the
law has no gain -- with an observer shape of ssm_cases (n, m, rom order, ssm order; n_o = n; m is the plant's).  C is a seeded
standard-normal (n_o, n_p) matrix scaled by one factor so that max |C x0| over the batch is 0.3, y_ref the observer's z_ref plus
0.05 N(0, 1), V 1e-3 N(0, 1), all from default_rng(8100 + the cl case's seed + 37 n).  Tolerance: the project's rule,
cl_reference.tolerance(e_oracle) = max(100 e_oracle, 1e-13) with e_oracle <= cl_reference.E_ORACLE_MAX asserted.  Whatever the functions
return is cached: treat it as read-only.

Edges covered: n_p = 8, 12 and 72 (fewer columns than a wave; more columns than the slice layout has lanes per slice); m = 3, 4 and 8;
linear, quadratic and cubic observers; n_o below and above 8; n_keep of 1 and of 60; fractional dt / dt_sim; a batch of 1 and one above the
CU count; with and without W."""
import numpy as np

import cl_cases as cc
import ssm_cases as sc
import ssm_loop_tpwl_reference as ref

# (entry of cl_cases.ADVANCE, observer shape)
PAIRS = [
    ('g6-knots-1', (2, 3, 4, 1)),
    ('g6-knots-max', (2, 3, 4, 1)),
    ('g6-5-max', (3, 3, 3, 3)),
    ('g6-frac-10', (2, 3, 4, 1)),
    ('g6-single', (2, 3, 4, 1)),
    ('g6-260', (2, 3, 4, 1)),
    ('r36-5-10', (6, 4, 3, 3)),
    ('r36-knots-max', (9, 4, 2, 2)),
    ('m8-frac-10', (12, 8, 2, 2)),
    ('m8-frac-10', (10, 8, 3, 2)),
]
SMALL = [p for p in PAIRS if p[0] != 'g6-260']           # the B <= 3 pairings
# Members whose gain-free chain stays in ONE region over all the sub-steps (their panel is loaded once); every other member of a case with
# more than one sub-step changes region inside the window (2-5 regions).  r36-5-10: ten steps of 0.01 move members 1 and 2 of the stiff
# n_p = 72 model too little to leave their region -- as in tests/test_tpwl_step_rule_gpu.py, where the same case is stated the same way.
STAYING = {'r36-5-10': [1, 2]}
FIELDS = ref.FIELDS


def case_id(p):
    return '%s+%s' % (p[0], sc.shape_id(p[1]))


def cl_case(p):
    return [c for c in cc.ADVANCE if c[0] == p[0]][0]


@sc.cached
def observer_model(s):
    """The float64 coefficient arrays of an observer shape: ssm_cases.model where it has the shape, else the same generator and seed."""
    if s in sc.SHAPES:
        return sc.model(s)
    import workloads
    n, m, ro, so = s
    d = workloads.ssm_model(n, m, ro, so, seed=500 + n)
    d['n_o'] = n
    return d


@sc.cached
def inputs(p):
    """dict x (B, n_p), uopt (B, N, m), W (n_keep, B, n_p) or None, j, theta (n_keep) of the cl case; C (n_o, n_p), y_ref (n_o), V (n_keep,
    B, n_o); and N, dt_sim, n_keep, B, model (the cl_cases model name)."""
    case = cl_case(p)
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    c = cc.advance_case(case)
    d = observer_model(p[1])
    n_o, n_p = d['n_o'], c['x'].shape[1]
    assert d['m'] == c['uopt'].shape[2], (d['m'], c['uopt'].shape)
    rng = np.random.default_rng(8100 + seed + 37 * d['n'])
    C = rng.standard_normal((n_o, n_p))
    C *= 0.3 / np.abs(c['x'] @ C.T).max()
    y_ref = d['z_ref'] + 0.05 * rng.standard_normal(n_o)
    V = 1e-3 * rng.standard_normal((n_keep, B, n_o))
    return dict(x=c['x'], uopt=c['uopt'], W=c['W'], j=np.asarray(c['j']), theta=np.asarray(c['theta']), C=C, y_ref=y_ref, V=V, N=cc.N, dt_sim=dt_sim,
                n_keep=n_keep, B=B, model=mname)


def chain(p, dtype):
    """The chain of every member in `dtype`: ({field: (B, n_keep, .)}, picks (B, n_keep), the least margin)."""
    i = inputs(p)
    make = sc.reference_model if dtype is ref.LD else sc.oracle_model
    obs = make(observer_model(p[1]))
    plant = cc.table_dict(i['model'], i['dt_sim'])
    out = [ref.advance(plant, i['C'], i['y_ref'], obs, i['uopt'][b], i['x'][b], i['j'], i['theta'], None if i['W'] is None else i['W'][:, b],
                       i['V'][:, b], dtype) for b in range(i['B'])]
    return {f: np.stack([o[k] for o in out]) for k, f in enumerate(FIELDS)}, np.stack([o[5] for o in out]), min(o[6] for o in out)


@sc.cached
def reference(p):
    """dict ref ({field: long-double chain}), picks (B, n_keep) of the long-double chain, picks64 of the float64 chain, margin (the least of
    both chains), e_oracle ({field: error of the float64 chain})."""
    r, picks, margin = chain(p, ref.LD)
    f64, picks64, margin64 = chain(p, np.float64)
    return dict(ref=r, picks=picks, picks64=picks64, margin=min(margin, margin64), e_oracle={f: ref.err(f64[f], r[f]) for f in FIELDS})
