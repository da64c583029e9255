"""Koopman baseline on the device: lift (csrc/koopman.hip) against the reference's lift_data / add_zeta_offline, W projection
and a degree-4 model against a numpy statement, limits, the resident Koopman MPC step against the exact QP, the host
composition and batched solves, and the KoopmanMPC.evaluate trace of the reference (g22_koopman.npz)."""
import io
import contextlib
import os

import numpy as np
import pytest

from sofacontrol_amd.baselines.koopman import koopman_utils as ku
from sofacontrol_amd.baselines.koopman.koopman import KoopmanMPC
from sofacontrol_amd.baselines import mpc as bmpc
from sofacontrol_amd.utils import Polyhedron

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_koopman.npz')


@pytest.fixture(scope='module')
def g():
    return dict(np.load(GOLDEN))


def model_of(g, DMD=False, **over):
    model = {k: g['model_' + k] for k in ('A', 'B', 'C', 'M', 'K')}
    model.update(over)
    params = {'n': 3, 'm': 4, 'N': model['A'].shape[0], 'nzeta': 10, 'delays': 1, 'obs_degree': 2, 'obs_type': 'poly',
              'Ts': 0.05, 'scale': {k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}}
    return ku.KoopmanModel(model, params, DMD=DMD)


def np_lift(Z, exps):
    """The observables as a numpy statement: prod_j zeta_j ** e_j for every exponent row."""
    return np.stack([np.prod(Z ** e[None, :], axis=1) for e in exps], axis=1)


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


class Cost:
    def __init__(self, Q, R, Qf=None):
        self.Q, self.R, self.Qf = Q, R, Qf


class Target:
    def __init__(self, t, z, u):
        self.t, self.z, self.u = t, z, u


def diamond_problem(g):
    cost = Cost(g['cost_Q'], g['cost_R'])
    target = Target(g['cost_t'], g['cost_z'], g['cost_u'])
    U = Polyhedron(g['cost_UA'], g['cost_Ub'])
    return cost, target, U


@pytest.mark.parametrize('dmd', [False, True])
def test_lift_matches_reference(g, dmd):
    km = model_of(g, DMD=dmd)
    Z = g['zeta_offline_1']
    want = g['lift_dmd' if dmd else 'lift']
    got = km.lift_batch(Z)
    assert got.shape == want.shape
    assert rel(got, want) <= 1e-13
    assert rel(km.lift_data(*Z[3]), want[3]) <= 1e-13


@pytest.mark.parametrize('d', [1, 2, 3])
def test_bulk_embed_lift(g, d):
    s = {k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}
    Y, U = g['rec_y'], g['rec_u']
    emb = ku.KoopmanLift(3, 4, d, 1, DMD=True, **s)
    np.testing.assert_allclose(emb.embed_lift(Y, U), g['zeta_offline_%d' % d], rtol=0, atol=0)
    # add_zeta_offline on the host class goes through the same kernel
    od = ku.KoopmanOfflineData(s, d)
    od.y_norm, od.u_norm = od.scaling.scale_down(y=Y), od.scaling.scale_down(u=U)
    od.add_zeta_offline()
    np.testing.assert_array_equal(od.zeta, g['zeta_offline_%d' % d])
    # degree 2 lift of the record == lift of the golden zetas (T = 9: not a multiple of any tile)
    lf = ku.KoopmanLift(3, 4, d, 2, **s)
    Z = g['zeta_offline_%d' % d]
    assert rel(lf.embed_lift(Y, U), np_lift(Z, ku.observable_exponents(Z.shape[1], 2))) <= 1e-13
    # fewer than delay + 1 samples: no rows
    assert lf.embed_lift(Y[:d], U[:d]).shape == (0, lf.n_out)


def test_bulk_embed_lift_long_record(g):
    km = model_of(g)
    rng = np.random.default_rng(5)
    T = 1000 + 37
    Y = g['scale_y_offset'] + 10 * rng.standard_normal((T, 3))
    U = 200 + 1300 * rng.random((T, 4))
    Yn, Un = km.scaling.scale_down(y=Y), km.scaling.scale_down(u=U)
    Z = np.hstack([Yn[1:], Yn[:-1], Un[:-1]])
    assert rel(km.lift_record(Y, U), np_lift(Z, ku.observable_exponents(10, 2))) <= 1e-13


def test_truncated_W_and_degree4(g):
    rng = np.random.default_rng(7)
    W = rng.standard_normal((40, 66))
    Z = rng.standard_normal((203, 10))
    lw = ku.KoopmanLift.for_zeta(10, 2, W=W)
    assert lw.has_w and lw.n_out == 40
    want = np_lift(Z, ku.observable_exponents(10, 2)) @ W.T
    assert rel(lw.lift(Z), want) <= 1e-12
    Z4 = rng.uniform(-1.5, 1.5, (131, 4))
    l4 = ku.KoopmanLift.for_zeta(4, 4)
    assert l4.n_out == 70
    assert rel(l4.lift(Z4), np_lift(Z4, ku.observable_exponents(4, 4))) <= 1e-13
    W4 = rng.standard_normal((70, 70))
    assert rel(ku.KoopmanLift.for_zeta(4, 4, W=W4).lift(Z4), np_lift(Z4, ku.observable_exponents(4, 4)) @ W4.T) <= 1e-12


def test_limits_raise():
    with pytest.raises(RuntimeError):
        ku.KoopmanLift.for_zeta(65, 1)
    with pytest.raises(RuntimeError):
        ku.KoopmanLift.for_zeta(4, 5)
    with pytest.raises(RuntimeError):
        ku.KoopmanLift.for_zeta(64, 2)                              # 2145 observables > 1024
    with pytest.raises(RuntimeError):
        ku.KoopmanLift.for_zeta(10, 2, W=np.ones((67, 66)))        # more rows than observables
    lf = ku.KoopmanLift.for_zeta(5, 2)
    with pytest.raises(RuntimeError):
        lf.lift(np.zeros((3, 6)))


def solve_exact(g, km, x0, t0, N, cost, target, U):
    from oracle import locp as olocp
    from scipy.interpolate import interp1d
    t = t0 + km.Ts * np.arange(N + 1)
    z = interp1d(target.t, target.z, axis=0, bounds_error=False, fill_value=(target.z[0], target.z[-1]))(t)
    qp = olocp.build_qp(N, km.H, cost.Q, cost.R, [km.A_d] * N, [km.B_d] * N, [np.zeros(km.N)] * N, x0, None, 0.0, 0.0,
                        z=z, u_des=np.tile(target.u, (N, 1)), U=(U.A, U.b), tr_active=False)
    w, _, _ = olocp.solve_exact(qp)
    x, u, _ = olocp.split(qp, w)
    return x, u, olocp.objective(qp, w)


def push_history(node, g, k0, count, batch=1, jitter=None):
    for k in range(k0, k0 + count):
        y = np.tile(g['trace_y'][k], (batch, 1))
        if jitter is not None:
            y = y + jitter[:, None] * (k - k0 + 1)
        node.push(y, np.tile(g['tr_1_0_u'][k], (batch, 1)))


def test_resident_step_matches_exact_qp_and_host_path(g):
    km = model_of(g)
    cost, target, U = diamond_problem(g)
    N = 5
    node = bmpc.KoopmanSolverNode(km, N, km.Ts, cost, target, U=U)
    push_history(node, g, 200, 2)
    t0 = 0.1
    x0, x, u, J, st = node.step(t0)
    assert st[0] == 0
    # x0 == the numpy lift of the same history
    yn = km.scaling.scale_down(y=g['trace_y'][200:202]); un = km.scaling.scale_down(u=g['tr_1_0_u'][200:202])
    zeta = np.hstack([yn[1], yn[0], un[0]])
    x0_np = np_lift(zeta[None, :], ku.observable_exponents(10, 2))[0]
    assert rel(x0[0], x0_np) <= 1e-14
    xe, ue, Je = solve_exact(g, km, x0_np, t0, N, cost, target, U)
    assert abs(J[0] - Je) <= 1e-7 * abs(Je)
    assert rel(u[0], ue) <= 1e-6
    # host composition: numpy lift + MPCSolver (no device lift involved)
    host = bmpc.MPCSolver(km, N, km.Ts, cost, x0_np, target, U=U)
    host.solve(t0, x0_np)
    xh, uh, _, _ = host.get_solution()
    assert rel(u[0], uh) <= 1e-9 and rel(x[0], xh) <= 1e-9
    # the next step reuses the transposed horizon of the first (slocp_plan_solve_dev_resident): same inputs, same results
    x0b, xb, ub, Jb, stb = node.step(t0)
    np.testing.assert_array_equal(xb, x)
    np.testing.assert_array_equal(ub, u)
    assert Jb[0] == J[0] and stb[0] == 0


def test_nodes_on_one_model_keep_their_own_history(g):
    """Two controllers on one model stepped in lockstep: each node lifts its own samples (the ring is per node)."""
    km = model_of(g)
    cost, target, U = diamond_problem(g)
    a = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U)
    b = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U)
    exps = ku.observable_exponents(10, 2)
    ys, us = g['trace_y'], g['tr_1_0_u']
    hist = {id(a): [], id(b): []}
    for k in range(205, 211):
        for node, off in ((a, 0.0), (b, 0.7)):
            y = ys[k] + off
            node.push(y, us[k])
            hist[id(node)].append((y, us[k]))
        for node in (a, b):
            if len(hist[id(node)]) < 2:
                continue
            (y0, u0), (y1, _) = hist[id(node)][-2:]
            zeta = np.hstack([km.scaling.scale_down(y=y1)[0], km.scaling.scale_down(y=y0)[0], km.scaling.scale_down(u=u0)[0]])
            x0, _, _, _, st = node.step(0.05)
            assert st[0] == 0
            assert rel(x0[0], np_lift(zeta[None, :], exps)[0]) <= 1e-14
    # the stateless lift of the model is not disturbed by the nodes either
    Z = g['zeta_offline_1']
    assert rel(km.lift_batch(Z), g['lift']) <= 1e-13


def test_step_records(g):
    """One blocking wait per step (with or without a push inside the step); the device time of the QP, recorded by events."""
    km = model_of(g)
    cost, target, U = diamond_problem(g)
    node = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U)
    push_history(node, g, 200, 2)
    node.step(0.0)
    assert node.stats()['waits_last_step'] == 1
    node.push(g['trace_y'][202], g['tr_1_0_u'][202])
    node.push(g['trace_y'][203], g['tr_1_0_u'][203])
    node.step(0.05)
    assert node.stats()['waits_last_step'] == 1
    node.set_timing(True)
    node.step(0.1, g['trace_y'][204], g['tr_1_0_u'][204])
    st = node.stats()
    assert st['waits_last_step'] == 1 and st['steps'] == 3
    assert st['qp_ms'] > 0 and st['pre_qp_ms'] > 0 and st['copy_back_ms'] > 0
    assert st['qp_ms'] + st['pre_qp_ms'] <= st['device_ms'] * (1 + 1e-6) + 1e-3
    node.set_timing(False)
    node.step(0.15)
    assert node.stats()['qp_ms'] == -1.0


def test_unsupported_node_options_raise(g):
    km = model_of(g)
    cost, target, U = diamond_problem(g)
    with pytest.raises(RuntimeError):
        bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U, input_nullspace=np.ones(4))
    # x_char reaches the resident QP as it reaches LOCP: the same solution as the host node with the same option
    xc = np.linspace(0.5, 2.0, 66)
    node = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U, x_char=xc)
    push_history(node, g, 200, 2)
    x0, x, u, J, st = node.step(0.1)
    host = bmpc.MPCSolverNode(km, 5, km.Ts, cost, target, U=U, x_char=xc)
    _, xh, uh, _, _ = host.mpc_callback(0.1, x0[0])
    assert st[0] == 0 and rel(u[0], uh) <= 1e-9 and rel(x[0], xh) <= 1e-9


def test_closed_loop_example_runs():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'examples', 'diamond_koopman_closed_loop.py'), '--steps', '260'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('koopman closed loop')]
    assert line and '260 steps, 32 solves' in line[0], r.stdout[-2000:]


def test_batch64_one_launch(g):
    km = model_of(g)
    cost, target, U = diamond_problem(g)
    N, B = 5, 64
    jit = np.linspace(-0.5, 0.5, B)
    nb = bmpc.KoopmanSolverNode(km, N, km.Ts, cost, target, U=U, batch=B)
    push_history(nb, g, 210, 3, batch=B, jitter=jit)
    x0, x, u, J, st = nb.step(0.35)
    assert (st == 0).all()
    km1 = model_of(g)
    for b in (0, 17, 40, 63):
        n1 = bmpc.KoopmanSolverNode(km1, N, km1.Ts, cost, target, U=U)
        push_history(n1, g, 210, 3, batch=1, jitter=jit[b:b + 1])
        a0, a, au, aJ, ast = n1.step(0.35)
        np.testing.assert_allclose(x0[b], a0[0], rtol=0, atol=0)
        assert rel(au[0], u[b]) <= 1e-9 and abs(aJ[0] - J[b]) <= 1e-9 * abs(J[b])


def run_trace(g, km, rh, hold, resident, Y=None, ys=None):
    cost, target, U = diamond_problem(g)
    N = int(g['mpc_N'])
    if resident:
        node = bmpc.KoopmanSolverNode(km, N, km.Ts, cost, target, U=U)
        c = KoopmanMPC(km, delay=2, u0=np.full(4, 300.), rollout_horizon=rh, input_hold=bool(hold), solver_node=node, Y=Y)
    else:
        node = bmpc.MPCSolverNode(km, N, km.Ts, cost, target, U=U)
        c = KoopmanMPC(km, delay=2, u0=np.full(4, 300.), rollout_horizon=rh, input_hold=bool(hold),
                       client=bmpc.MPCClient(node), Y=Y)
    c.set_sim_timestep(0.01)
    tag = 'tr_%d_%d_' % (rh, hold)
    ys = g['trace_y'] if ys is None else ys
    u_ref = g[tag + 'u']
    us = []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(ys.shape[0]):
            # the previous input of the REFERENCE's run: the lifted requests are then comparable to 1e-12
            u_prev = np.full(4, 300.) if k == 0 else u_ref[k - 1]
            us.append(c.evaluate(0.01 * k, ys[k], None, u_prev))
    return c, np.stack(us)


@pytest.mark.parametrize('rh', [1, 3])
@pytest.mark.parametrize('hold', [0, 1])
@pytest.mark.parametrize('resident', [True, False])
def test_evaluate_trace(g, rh, hold, resident):
    km = model_of(g)
    c, us = run_trace(g, km, rh, hold, resident)
    tag = 'tr_%d_%d_' % (rh, hold)
    req_t = np.array([r[0] for r in c.requests]); req_x = np.stack([r[1] for r in c.requests])
    np.testing.assert_array_equal(req_t, g[tag + 'req_t'])
    assert rel(req_x, g[tag + 'req_x0']) <= 1e-12
    assert np.abs(us - g[tag + 'u']).max() <= 1e-6 * np.abs(g[tag + 'u']).max()
    info = c.save_controller_info()
    for k in ('t_opt', 'u_opt', 'z_opt', 'zopt_full'):
        assert np.shape(info[k]) == g[tag + k].shape, k
    np.testing.assert_array_equal(info['t_opt'], g[tag + 't_opt'])
    assert np.abs(info['u_opt'] - g[tag + 'u_opt']).max() <= 1e-6 * np.abs(g[tag + 'u_opt']).max()
    assert np.stack(info['z_rollout']).shape == g[tag + 'z_rollout'].shape
    assert len(info['solve_times']) == int(g[tag + 'n_solves'])
    assert info['rollout_time'] == float(g[tag + 'rollout_time'])
    assert set(info) == {'t_opt', 'u_opt', 'z_opt', 'zopt_full', 'z_rollout', 't_rollout', 'solve_times', 'rollout_time'}


def test_Y_projection_path(g):
    """Trunk-style output box: measurements outside Y are projected before they enter the history (koopman.py:155-156)."""
    km = model_of(g)
    off = g['scale_y_offset'][0]
    lo, hi = off - np.array([1.0, 1.0, 0.2]), off + np.array([1.0, 1.0, 0.2])
    Y = Polyhedron(np.vstack([np.eye(3), -np.eye(3)]), np.concatenate([hi, -lo]), with_reproject=True)
    ys = g['trace_y'][:215]
    c_res, u_res = run_trace(g, km, 1, 0, True, Y=Y, ys=ys)
    c_host, u_host = run_trace(g, model_of(g), 1, 0, False, Y=Y, ys=ys)
    assert len(c_res.requests) == len(c_host.requests) == 3
    # the box projection of a point is the clip: the lifted requests equal the lift of the clipped history, up to the
    # tolerance of the projection QP (spoly_project is an interior point, not a clip)
    yc = np.clip(ys, lo, hi)
    yn = km.scaling.scale_down(y=yc); un = km.scaling.scale_down(u=g['tr_1_0_u'][:215])
    k = 200
    zeta = np.hstack([yn[k], yn[k - 1], un[k - 1]])
    assert rel(c_res.requests[0][1], km.lift_data(*zeta)) <= 1e-9
    assert rel(np.stack([r[1] for r in c_res.requests]), np.stack([r[1] for r in c_host.requests])) <= 1e-12
    assert np.abs(u_res - u_host).max() <= 1e-6 * np.abs(u_host).max()
