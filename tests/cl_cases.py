"""Seeded closed-loop cases shared by tests/test_cl_reference_cpu.py (input conditions, without a GPU) and tests/test_gusto_loop_gpu.py
(the kernels of csrc/gusto_loop.hip on the same numbers).

A model is helpers.golden_problem (oracle.tpwl.synthetic_model with its points scaled by q_scale); the planner's tables are discretised
at DT, the plant's at dt_sim, both with oracle.tpwl.pre_discretize on the CPU and installed on the device as they are, so the reference
and the kernels read the same tables.  An advance case is a batch of synthetic plans: the plan's position part runs from one table point to
another (so the gain lookup at x_bar changes region on the way), the plant starts at the plan's first state plus an offset and is driven
through regions by the model's own stiff dynamics; gains are seeded (P, n_u, n_x) arrays, disturbances seeded (n_keep, B, n_x)."""
import numpy as np

import cl_reference as cr
from helpers import golden_problem
from oracle import tpwl as otpwl

DT = 0.05
N = 12

# name -> (r, m, P, n_nodes, seed, q_scale)
MODELS = {
    'g6': (4, 3, 7, 20, 30, 0.05),          # the problem of tests/test_gusto_gpu.py:21
    'r36': (36, 4, 8, 40, 33, 0.2),         # n_x = 72: more rows than lanes
    'm8': (6, 8, 5, 20, 41, 0.1),           # eight inputs
}

# (name, model, batch, dt_sim, n_keep, gains, disturbance, seed)
ADVANCE = [
    ('g6-knots-1', 'g6', 3, 0.05, 1, False, False, 1),          # dt / dt_sim = 1: the plan's knots are hit exactly
    ('g6-knots-max', 'g6', 3, 0.05, 12, True, True, 2),         # ... and the largest n_keep: the held last input interval is sampled
    ('g6-5-10', 'g6', 3, 0.01, 10, True, False, 3),             # the example's 0.05 / 0.01
    ('g6-5-max', 'g6', 3, 0.01, 60, False, True, 4),
    ('g6-frac-10', 'g6', 3, 0.03, 10, True, True, 5),           # non-integer ratio: theta varies
    ('g6-frac-max', 'g6', 3, 0.03, 20, True, False, 6),
    ('g6-single', 'g6', 1, 0.01, 10, True, True, 7),
    ('g6-260', 'g6', 260, 0.03, 10, True, True, 8),             # more rollouts than CUs
    ('r36-5-10', 'r36', 3, 0.01, 10, True, True, 9),
    ('r36-knots-max', 'r36', 3, 0.05, 12, False, False, 10),
    ('m8-frac-10', 'm8', 3, 0.03, 10, True, True, 11),
]

_models = {}


def direct_schedule(N, dt, dt_sim, n_keep, t_start, k):
    """The schedule of period k stated directly (scalars, Python floats = IEEE doubles): t_k, idx0, j, theta."""
    step = n_keep * dt_sim
    t_k = t_start + k * step
    idx0 = 0
    if k > 0:
        t_prev = t_start + (k - 1) * step
        idx0 = N
        for i in range(N + 1):
            if t_prev + dt * i >= t_k:
                idx0 = i
                break
    j, theta = [], []
    for s in range(n_keep):
        tau = s * dt_sim
        js = min(int(tau / dt), N - 1)
        j.append(js)
        theta.append((tau - js * dt) / dt)
    return t_k, idx0, np.array(j), np.array(theta)


def model(name):
    """{'model', 'U', 'q_ref', 'v_ref', 'Hf', 'H' (n_z, n_x)} of MODELS[name]; H = Hf [[U, 0], [0, U]] rows [v; q] as the product forms it."""
    if name not in _models:
        r, m, P, n_nodes, seed, q_scale = MODELS[name]
        mdl, U, q_ref, v_ref, Hf = golden_problem(r, m, P, n_nodes, seed, q_scale=q_scale)
        n_f = U.shape[0]
        V = np.zeros((2 * n_f, 2 * r))
        V[:n_f, :r] = U
        V[n_f:, r:] = U
        _models[name] = dict(model=mdl, U=U, q_ref=q_ref, v_ref=v_ref, Hf=Hf, H=np.asarray(Hf @ V))
    return _models[name]


def tables(name, dt):
    """Zero-order-hold tables of the model at dt (CPU), cached."""
    key = (name, float(dt))
    if key not in _models:
        _models[key] = otpwl.pre_discretize(model(name)['model'], dt, 'zoh')
    return _models[key]


def table_dict(name, dt=None):
    mdl = model(name)['model']
    d = dict(q=mdl['q'], v=mdl['v'], w_q=mdl['w_q'], w_v=mdl['w_v'])
    if dt is not None:
        d['A_d'], d['B_d'], d['d_d'] = tables(name, dt)
    return d


def advance_case(case):
    """The inputs of an ADVANCE row: dict xopt (B, N+1, n), uopt (B, N, m), x (B, n), K or None, W (n_keep, B, n) or None, j, theta."""
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    r, m, P = MODELS[mname][:3]
    mdl = model(mname)['model']
    rng = np.random.default_rng(1000 + seed)
    n = 2 * r
    s = np.linspace(0.0, 1.0, N + 1)[:, None]
    xopt = np.zeros((B, N + 1, n))
    for b in range(B):
        a, e = rng.choice(P, size=2, replace=False)
        qa, qe = mdl['q'][a], mdl['q'][e]
        xopt[b, :, r:] = qa + (0.07 + 0.86 * s) * (qe - qa) + 0.02 * np.abs(qe - qa).max() * rng.standard_normal((N + 1, r))
        xopt[b, :, :r] = 0.1 * np.abs(qe - qa).max() * rng.standard_normal((N + 1, r))
    uopt = rng.uniform(0.0, 100.0, (B, N, m))
    scale = np.abs(mdl['q']).max()
    x = xopt[:, 0] + 0.05 * scale * rng.standard_normal((B, n))
    K = 20.0 * rng.standard_normal((P, m, n)) if gains else None
    W = 0.01 * scale * rng.standard_normal((n_keep, B, n)) if dist else None
    _, _, j, theta = direct_schedule(N, DT, dt_sim, n_keep, 0.0, 0)
    return dict(xopt=xopt, uopt=uopt, x=x, K=K, W=W, j=j, theta=theta)


def advance_reference(case, dtype, H=None):
    """The reference advance of every member: X (B, n_keep, n), U, Z, plant picks, gain picks (B, n_keep) and the least margin.
    H: the output map to use (the product's own on the GPU box), default the one formed here."""
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    c = advance_case(case)
    planner, plant = table_dict(mname), table_dict(mname, dt_sim)
    H = model(mname)['H'] if H is None else H
    outs = [cr.advance(planner, plant, H, c['K'], c['xopt'][b], c['uopt'][b], c['x'][b], c['j'], c['theta'],
                       None if c['W'] is None else c['W'][:, b], dtype) for b in range(B)]
    stack = lambda i: np.stack([o[i] for o in outs])
    return stack(0), stack(1), stack(2), stack(3), stack(4), min(o[5] for o in outs)


# ---- whole loops on the g6 problem (targets, cost and input box of tests/golden/g6_gusto.npz)
# name -> (dt_sim, n_keep, terminal cost and input target)
LOOPS = {'frac': (0.03, 10, False), 'zf-u': (0.01, 10, True)}
PERIODS = 4


def g6():
    import os
    if 'g6_golden' not in _models:
        _models['g6_golden'] = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g6_gusto.npz')))
    return _models['g6_golden']


def loop_inputs(B, n_keep):
    """x0 (B, 8), phase (B,), K (7, 3, 8), W (PERIODS, n_keep, B, 8), u target table (T, 3): members 0..2 are the same for every B >= 3, and
    differ; member 0 asks for targets before t[0], member 2 behind t[-1] (the clamped ends of the table)."""
    g = g6()
    rng, more = np.random.default_rng(77), np.random.default_rng(78)
    extra = max(B, 3) - 3
    x0 = np.concatenate((1e-3 * rng.standard_normal((3, 8)) * rng.uniform(0.5, 5.0, (3, 1)),
                         1e-3 * more.standard_normal((extra, 8)) * more.uniform(0.1, 30.0, (extra, 1))))
    phase = np.concatenate(([-0.2, 0.37, float(g['t'][-1]) - 0.5], more.uniform(-0.3, 3.0, extra)))
    K = 20.0 * rng.standard_normal((7, 3, 8))
    W = 1e-4 * np.concatenate((rng.standard_normal((PERIODS, n_keep, 3, 8)), more.standard_normal((PERIODS, n_keep, extra, 8))), axis=2)
    ut = 10.0 + 5.0 * np.sin(np.outer(g['t'], [1.0, 2.0, 3.0]))
    return dict(x0=x0[:B], phase=phase[:B], K=K, W=np.ascontiguousarray(W[:, :, :B]), ut=ut)
