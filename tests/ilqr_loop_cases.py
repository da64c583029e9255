"""Seeded cases of the batched closed-loop iLQR, shared by tests/test_ilqr_loop_reference_cpu.py (input conditions, without a GPU) and
tests/test_ilqr_loop_gpu.py (the kernels of csrc/ilqr_loop.hip on the same numbers).

Models are those of tests/cl_cases.py (golden_problem) plus a one-point plant; the plant's tables are discretised at dt_sim with
oracle.tpwl.pre_discretize on the CPU and installed on the device as they are, so the reference and the kernels read the same tables.
A policy is seeded, not solved: x_bar runs from one table point to another (cl_cases.advance_case's plans), u_bar is uniform in
(0, 100), K a seeded (N, n_u, n_x) array per member -- all members distinct; the plant starts at x_bar[0] plus an offset."""
import numpy as np

import cl_cases as cc
import clobs_cases as oc
import ilqr_loop_reference as ir

cc.MODELS.setdefault('p1', (4, 3, 1, 20, 51, 0.05))         # a one-point plant: the panel is loaded once, the search has one candidate

DT = cc.DT          # the controller step of every case

# (name, model, batch, N, r, steps, non-zero idle input, disturbance, seed); dt_sim = DT / r
ADVANCE = [
    ('g6-r1', 'g6', 3, 12, 1, 12, False, False, 1),             # every step fires; rows 3, 6, 7 read 2, 5, 6
    ('g6-r5-tail', 'g6', 3, 12, 5, 67, True, True, 2),          # held inputs between controller steps, the row quirk, the u0 tail (j = 13)
    ('g6-N1', 'g6', 3, 1, 1, 3, True, False, 3),                # one policy row, then idle
    ('g6-single', 'g6', 1, 12, 5, 20, False, True, 4),
    ('g6-260', 'g6', 260, 12, 5, 20, False, True, 5),           # more members than CUs, all distinct
    ('r36-r5', 'r36', 3, 12, 5, 20, False, True, 6),            # n_x = 72: more rows than lanes, two columns of K per lane
    ('m8-r1', 'm8', 3, 12, 1, 15, True, True, 7),               # eight inputs: two gain rows per wave; steps 13, 14 idle
    ('p1-r5', 'p1', 3, 12, 5, 20, False, True, 8),
]
IDS = [c[0] for c in ADVANCE]

# seeds replaced because the default one misses an input condition (tests/test_ilqr_loop_reference_cpu.py): a lookup within MARGIN of a
# second point, or e_oracle above E_ORACLE_MAX
SEEDS = {}

_cache = {}


def dt_sim_of(case):
    return {1: 0.05, 5: 0.01}[case[4]]


def policy(mname, B, N, seed):
    """x_bar (B, N+1, n), u_bar (B, N, m), K (B, N, m, n), x (B, n): cl_cases.advance_case's plans cut to N rows, with seeded gains."""
    r, m, P = cc.MODELS[mname][:3]
    rng = np.random.default_rng(9000 + seed)
    if P >= 2:
        c = cc.advance_case(('ilqr', mname, B, 0.05, 1, False, False, 300 + seed))
    else:                                                   # one point: the plan wanders around it
        q0 = cc.model(mname)['model']['q'][0]
        scale = np.abs(q0).max()
        xopt = 0.1 * scale * rng.standard_normal((B, cc.N + 1, 2 * r))
        xopt[:, :, r:] += q0
        c = dict(xopt=xopt, uopt=rng.uniform(0.0, 100.0, (B, cc.N, m)), x=xopt[:, 0] + 0.05 * scale * rng.standard_normal((B, 2 * r)))
    K = 20.0 * rng.standard_normal((B, N, m, 2 * r))
    return dict(xbar=np.ascontiguousarray(c['xopt'][:, :N + 1]), ubar=np.ascontiguousarray(c['uopt'][:, :N]), K=K, x=c['x'])


def advance_case(case):
    """The inputs of an ADVANCE row: dict xbar, ubar, K, x, rows, u0, W (steps, B, n) or None."""
    if case[0] not in _cache:
        name, mname, B, N, r, steps, idle, dist, seed = case
        seed = SEEDS.get(name, seed)
        c = policy(mname, B, N, seed)
        m = cc.MODELS[mname][1]
        rng = np.random.default_rng(9500 + seed)
        scale = np.abs(cc.model(mname)['model']['q']).max()
        c['rows'] = ir.rows_table(N, DT, N + 2)
        c['u0'] = rng.uniform(10.0, 60.0, m) if idle else np.zeros(m)
        c['W'] = 0.01 * scale * rng.standard_normal((steps, B, c['x'].shape[1])) if dist else None
        _cache[case[0]] = c
    return _cache[case[0]]


def advance_reference(case, dtype, H=None):
    """The reference advance of every member from a reset (step0 = 0, u_held = u0): X (B, steps, n), U, Z, picks and the least margin."""
    name, mname, B, N, r, steps, idle, dist, seed = case
    c = advance_case(case)
    plant = cc.table_dict(mname, dt_sim_of(case))
    H = cc.model(mname)['H'] if H is None else H
    outs = [ir.advance(plant, H, c['xbar'][b], c['ubar'][b], c['K'][b], c['rows'], r, c['u0'], c['x'][b], c['u0'], steps, 0,
                       None if c['W'] is None else c['W'][:, b], dtype) for b in range(B)]
    stack = lambda i: np.stack([o[i] for o in outs])
    return stack(0), stack(1), stack(2), stack(3), min(o[4] for o in outs)


_refs = {}


def advance_measured(case, H=None):
    """(long-double reference (X, U, Z, picks, margin), e_oracle of the float64 statement over X, U, Z), once per case and H."""
    key = (case[0], None if H is None else H.tobytes())
    if key not in _refs:
        ref, f64 = advance_reference(case, ir.LD, H), advance_reference(case, np.float64, H)
        assert np.array_equal(ref[3], f64[3]), case[0]
        _refs[key] = (ref, max(ir.err(f64[i], ref[i]) for i in range(3)))
    return _refs[key]


# ---- the observed loop on g6: the measurement model, filter covariances and the mismatched filter model of tests/clobs_cases.py
# (name, filter model is the plant's, r, steps, disturbance, measurement noise, seed)
OBSERVED = [
    ('obs-r1', True, 1, 6, False, False, 11),
    ('obs-r5-mismatch', False, 5, 12, True, True, 12),
]
OBS_IDS = [c[0] for c in OBSERVED]
OBS_B, OBS_N = 3, 12


def observed_case(cs):
    if cs[0] not in _cache:
        name, same, r, steps, dist, noise, seed = cs
        seed = SEEDS.get(name, seed)
        c = policy('g6', OBS_B, OBS_N, seed)
        n, ny = c['x'].shape[1], oc.N_Y['g6']
        rng = np.random.default_rng(9700 + seed)
        scale = np.abs(cc.model('g6')['model']['q']).max()
        c['rows'] = ir.rows_table(OBS_N, DT, OBS_N + 2)
        c['u0'] = np.zeros(3)
        c['x_hat'] = c['x'] + 0.02 * scale * rng.standard_normal((OBS_B, n))
        c['W'] = 0.01 * scale * rng.standard_normal((steps, OBS_B, n)) if dist else None
        c['V'] = 0.05 * rng.standard_normal((steps, OBS_B, ny)) if noise else None
        _cache[cs[0]] = c
    return _cache[cs[0]]


def observed_reference(cs, dtype, H=None):
    name, same, r, steps, dist, noise, seed = cs
    c, ms = observed_case(cs), oc.measurement('g6')
    dt_sim = {1: 0.05, 5: 0.01}[r]
    plant, filt = cc.table_dict('g6', dt_sim), oc.filter_tables('g6', same, dt_sim)
    H = cc.model('g6')['H'] if H is None else H
    outs = [ir.observed(plant, filt, H, ms['C'], ms['y_ref'], ms['W'], ms['V'], c['xbar'][b], c['ubar'][b], c['K'][b], c['rows'], r, c['u0'],
                        c['x'][b], c['x_hat'][b], ms['Sigma0'], steps, None if c['W'] is None else c['W'][:, b],
                        None if c['V'] is None else c['V'][:, b], dtype) for b in range(OBS_B)]
    res = {k: np.stack([o[k] for o in outs]) for k in outs[0] if k != 'margin'}
    res['margin'] = min(o['margin'] for o in outs)
    return res


# ---- the reference's own traces (tests/golden/g25_ilqr_loop.npz, written by tests/golden/make_golden_ilqr_loop.py)
G25_N, G25_R, G25_STEPS = 12, 5, 70


def g25():
    """The golden file plus the model it was made on (the g8 problem: golden_problem(4, 3, 7, 20, 40, q_scale=0.05)) as the table dicts
    of the statement -- the plant and the filter at dt_sim, with the reference's own discrete tables -- and the row table."""
    import os
    from helpers import golden_problem
    if 'g25' not in _cache:
        g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g25_ilqr_loop.npz')))
        mdl, U, q_ref, v_ref, Hf = golden_problem(4, 3, 7, 20, 40, q_scale=0.05)
        g['problem'] = (mdl, U, q_ref, v_ref, Hf)
        g['plant'] = dict(q=mdl['q'], v=mdl['v'], w_q=mdl['w_q'], w_v=mdl['w_v'], A_d=g['Ad_sim'], B_d=g['Bd_sim'], d_d=g['dd_sim'])
        g['rows'] = ir.rows_table(G25_N, float(g['dt']), G25_N + 2, final_time=float(g['final_time']))
        _cache['g25'] = g
    return _cache['g25']


def g25_statement(tag, dtype, policy=None):
    """The statement on the golden's inputs under `policy` = (x_bar, u_bar, K) (default: the golden's own): dict U, X, Xhat rows as the
    golden's u, x[1:], x_hat[1:], and the least margin.  'full': 70 steps from x0 without noise; 'ekf': the 69 steps whose measurement
    noise the golden holds, from (x0, x_hat[0], the covariance behind the reference's first update)."""
    g = g25()
    xb, ub, K = policy if policy is not None else (g[tag + '_x_bar'], g[tag + '_u_bar'], g[tag + '_K'])
    if tag == 'full':
        X, U, Z, ip, margin = ir.advance(g['plant'], g['H'], xb, ub, K, g['rows'], G25_R, g['u0'], g['x0'], g['u0'], G25_STEPS, 0, None, dtype)
        return dict(U=U, X=X, Xhat=X[:-1], margin=margin)
    S = G25_STEPS - 1
    o = ir.observed(g['plant'], g['plant'], g['H'], g['C'], g['y_ref'], g['Wf'], g['Vf'], xb, ub, K, g['rows'], G25_R, g['u0'], g['x0'],
                    g['ekf_x_hat'][0], g['ekf_Sigma_first'], S, g['w'][:S], g['v'][1:], dtype)
    return dict(U=o['U'], X=o['X'], Xhat=o['Xhat'], margin=o['margin'])


def g25_golden(tag):
    """The golden's rows that g25_statement's answer to."""
    g = g25()
    S = G25_STEPS if tag == 'full' else G25_STEPS - 1
    return dict(U=g[tag + '_u'][:S], X=g[tag + '_x'][1:S + 1], Xhat=g[tag + '_x_hat'][1:S] if tag == 'full' else g[tag + '_x_hat'][1:S + 1])


def g25_measured(tag):
    """(long-double statement, e_oracle of the float64 one over U, X, Xhat)."""
    if ('g25m', tag) not in _refs:
        ref, f64 = g25_statement(tag, ir.LD), g25_statement(tag, np.float64)
        _refs[('g25m', tag)] = (ref, max(ir.err(f64[k], ref[k]) for k in ('U', 'X', 'Xhat')))
    return _refs[('g25m', tag)]


OBS_FIELDS = ('X', 'U', 'Z', 'Xhat', 'Y')


def observed_measured(cs, H=None):
    key = (cs[0], None if H is None else H.tobytes())
    if key not in _refs:
        ref, f64 = observed_reference(cs, ir.LD, H), observed_reference(cs, np.float64, H)
        for k in ('idx_plant', 'idx_filter'):
            assert np.array_equal(ref[k], f64[k]), (cs[0], k)
        _refs[key] = (ref, max(ir.err(f64[k], ref[k]) for k in OBS_FIELDS))
    return _refs[key]
