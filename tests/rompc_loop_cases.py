"""Seeded cases of the batched closed-loop ROMPC shared by tests/test_rompc_loop_reference_cpu.py (input conditions, without a GPU)
and tests/test_rompc_loop_gpu.py (the kernels of csrc/rompc_loop.hip on the same numbers).

They stand on the models of cl_cases.MODELS.  The controller's linear model is the model's first table point discretised at dt_sim (the
choice of TPWL2LinearROM), its measurement map a seeded (n_y, n_x) matrix, its gains the DARE's (scipy): u = ubar + K (x_hat - xbar) with
rho(A + B K) < 1, and L with rho(A - L C) < 1.  The plant is the whole table at dt_sim (simulated), its first point alone (a one-point
plant), or a seeded record (replayed).  Plans are those of cl_cases.advance_case; the estimate starts a seeded offset from the state."""
import numpy as np

import cl_cases as cc
import rompc_loop_reference as rr

DT, N = cc.DT, cc.N

# (name, model, batch, n_y, dt_sim, n_replan, W, V, with H, plant: 'sim' | 'replay' | 'one', seed)
ADVANCE = [
    ('g6-knots-1', 'g6', 3, 3, 0.05, 1, False, False, True, 'sim', 1),            # the plan's knots are hit exactly; n_y below the pad width
    ('g6-knots-max', 'g6', 3, 30, 0.05, N, True, True, True, 'sim', 2),           # theta == 1 at the chain end
    ('g6-5-10', 'g6', 3, 30, 0.01, 10, True, False, False, 'sim', 3),             # the example's 0.05 / 0.01; without an output model
    ('g6-5-max', 'g6', 3, 3, 0.01, 5 * N, False, True, True, 'sim', 4),
    ('g6-frac-10', 'g6', 3, 64, 0.03, 10, True, True, True, 'sim', 5),            # non-integer ratio: theta varies
    ('g6-single', 'g6', 1, 30, 0.01, 10, True, True, True, 'sim', 6),
    ('g6-260', 'g6', 260, 30, 0.03, 10, True, True, True, 'sim', 7),              # more members than CUs
    ('g6-replay', 'g6', 3, 30, 0.01, 10, False, True, True, 'replay', 8),
    ('g6-one', 'g6', 3, 30, 0.03, 10, True, True, True, 'one', 9),
    ('r36-5-10', 'r36', 3, 30, 0.01, 10, True, True, True, 'sim', 10),            # n_x = 72: more rows than lanes
    ('r36-knots-max', 'r36', 3, 64, 0.05, N, False, False, True, 'sim', 11),
    ('r36-replay', 'r36', 3, 3, 0.03, 10, False, False, False, 'replay', 12),
    ('m8-frac-10', 'm8', 3, 30, 0.03, 10, True, True, True, 'sim', 13),           # eight inputs
]

_cache = {}


def controller(mname, ny, dt_sim, with_H):
    """dict A, B, d, C, y_ref, K, L, H (the map of the z record: the model's H, or C without an output model), H_model (None without),
    z_ref of the controller at dt_sim."""
    key = ('ctrl', mname, ny, float(dt_sim), with_H)
    if key not in _cache:
        import scipy.linalg as sl
        Ad, Bd, dd = cc.tables(mname, dt_sim)
        A, B, d = np.array(Ad[0]), np.array(Bd[0]), np.array(dd[0])
        n, m = B.shape
        rng = np.random.default_rng(100 * n + ny)
        C = rng.standard_normal((ny, n)) / np.sqrt(n)
        y_ref = rng.standard_normal(ny)
        P = sl.solve_discrete_are(A, B, np.eye(n), 1e2 * np.eye(m))
        K = -np.linalg.solve(1e2 * np.eye(m) + B.T @ P @ B, B.T @ P @ A)
        S = sl.solve_discrete_are(A.T, C.T, np.eye(n), 1e-1 * np.eye(ny))
        L = np.linalg.solve(1e-1 * np.eye(ny) + C @ S @ C.T, C @ S @ A.T).T
        H = cc.model(mname)['H'] if with_H else None
        _cache[key] = dict(A=A, B=B, d=d, C=C, y_ref=y_ref, K=K, L=L, H=C if H is None else H, H_model=H,
                           z_ref=None if H is None else rng.standard_normal(H.shape[0]))
    return _cache[key]


def spectral_radii(ctrl):
    rho = lambda M: float(np.abs(np.linalg.eigvals(M)).max())
    return rho(ctrl['A'] - ctrl['L'] @ ctrl['C']), rho(ctrl['A'] + ctrl['B'] @ ctrl['K'])


def plant_tables(mname, dt_sim, mode):
    """The plant of a case as the reference reads it: the whole table, its first point, or None (replay)."""
    if mode == 'replay':
        return None
    t = cc.table_dict(mname, dt_sim)
    if mode == 'one':
        t = {k: (v[:1] if k in ('q', 'v', 'A_d', 'B_d', 'd_d') else v) for k, v in t.items()}
    return t


def advance_case(case):
    """The inputs of an ADVANCE row: dict ctrl, plant, xopt (B, N+1, n), uopt (B, N, m), x, x_hat (B, n), W (n_replan, B, n) / V
    (n_replan, B, n_y) / X_plant (B, n_replan + 1, n) or None, j, theta."""
    name, mname, B, ny, dt_sim, nk, dist, noise, with_H, mode, seed = case
    if ('case', name) in _cache:
        return _cache[('case', name)]
    base = cc.advance_case((name, mname, B, dt_sim, nk, False, dist, 50 + seed))
    rng = np.random.default_rng(2000 + seed)
    scale = np.abs(cc.model(mname)['model']['q']).max()
    n = base['x'].shape[1]
    x = base['x']
    Xp = None
    if mode == 'replay':
        Xp = np.concatenate((x[:, None], x[:, None] + np.cumsum(0.01 * scale * rng.standard_normal((B, nk, n)), axis=1)), axis=1)
    c = dict(ctrl=controller(mname, ny, dt_sim, with_H), plant=plant_tables(mname, dt_sim, mode), xopt=base['xopt'], uopt=base['uopt'], x=x,
             x_hat=x + 0.02 * scale * rng.standard_normal((B, n)), W=base['W'] if mode != 'replay' else None,
             V=0.01 * scale * rng.standard_normal((nk, B, ny)) if noise else None, X_plant=Xp, j=base['j'], theta=base['theta'])
    _cache[('case', name)] = c
    return c


def advance_reference(case, dtype, ctrl=None):
    """The reference advance of every member, stacked: dict X, XH, Z, Y, U, Ubar, Xbar (B, n_replan, .), picks (B, n_replan), margin.
    ctrl: the controller to use (e.g. with the product's own output map on the GPU box), default the case's."""
    c = advance_case(case)
    B = c['x'].shape[0]
    outs = [rr.advance(ctrl or c['ctrl'], c['plant'], c['xopt'][b], c['uopt'][b], c['x'][b], c['x_hat'][b], c['j'], c['theta'],
                       None if c['W'] is None else c['W'][:, b], None if c['V'] is None else c['V'][:, b],
                       None if c['X_plant'] is None else c['X_plant'][b], dtype) for b in range(B)]
    res = {k: np.stack([o[k] for o in outs]) for k in outs[0] if k != 'margin'}
    res['margin'] = min(o['margin'] for o in outs)
    return res


RECORDS = ('X', 'XH', 'Z', 'Y', 'U', 'Ubar', 'Xbar')


def e_oracle(case):
    """(e_oracle, long-double reference, float64 statement) of a case, cached: the worst record's distance."""
    name = case[0]
    if ('ref', name) not in _cache:
        ref, f64 = advance_reference(case, rr.LD), advance_reference(case, np.float64)
        _cache[('ref', name)] = (max(rr.err(f64[k], ref[k]) for k in RECORDS), ref, f64)
    return _cache[('ref', name)]


def chain_case(B, N, n, m, seed):
    """Seeded plans, request states and status words for the chain kernel: members 1 and 3 (where there are that many) report a failure."""
    rng = np.random.default_rng(3000 + seed)
    status = np.zeros(B, dtype=np.int32)
    status[1::2] = np.array([3, -7, 1, 2] * B)[:len(status[1::2])]
    return dict(xsol=rng.standard_normal((B, N + 1, n)), usol=rng.uniform(0, 100, (B, N, m)), x0=rng.standard_normal((B, n)),
                xprev=rng.standard_normal((B, N + 1, n)), uprev=rng.uniform(0, 100, (B, N, m)), status=status)
