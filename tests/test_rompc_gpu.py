"""GPU: the ROMPC baseline -- sric_dare_wide against scipy, LinearROM / observer / ROMPC.evaluate against the golden vectors
of the imported reference (g23), and the resident step / replay kernels against a numpy statement of the recursion."""
import io
import os
import contextlib

import numpy as np
import pytest

from lq_cases import dare_modes_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rtol):
    np.testing.assert_allclose(a, b, rtol=0, atol=rtol * max(1.0, float(np.abs(b).max())))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(b).max()))


@pytest.fixture(scope='module')
def g(golden):
    return golden('g23_rompc')


# ------------------------------------------------------------------------------------------------ dare_wide
@pytest.mark.parametrize('n,m,rho,rank_q', [(8, 30, 0.98, 2), (12, 17, 0.9, 12), (20, 64, 0.9999, 20), (60, 30, 0.999, 2),
                                             (72, 30, 0.99, 3), (33, 48, 1.02, 6), (80, 64, 0.95, 5)])
def test_dare_wide_vs_scipy(n, m, rho, rank_q):
    import scipy.linalg as sl
    from sofacontrol_amd.lqr.lqr import dare_wide
    A, B, Q, R = dare_modes_case(n, m, rho, rank_q, 100 * n + m)
    K, P = dare_wide(A, B, Q, R)
    Ps = sl.solve_discrete_are(A, B, Q, R)
    Ks = -np.linalg.solve(R + B.T @ Ps @ B, B.T @ Ps @ A)
    print('dare_wide (%d, %d): P err %.3e of %.3e, K err %.3e of %.3e' % (n, m, np.abs(P - Ps).max(), np.abs(Ps).max(),
                                                                         np.abs(K - Ks).max(), np.abs(Ks).max()))
    close(P, Ps, 1e-9); close(K, Ks, 1e-8)
    assert np.abs(np.linalg.eigvals(A + B @ K)).max() < 1.0


def test_dare_wide_batched_and_failures():
    import scipy.linalg as sl
    from sofacontrol_amd.lqr.lqr import dare, dare_wide
    A, B, Q, R = dare_modes_case(12, 17, 0.9, 12, 1217)
    A2, B2, _, _ = dare_modes_case(12, 17, 0.8, 12, 7 * 12 + 17)
    K, P = dare_wide(A, B, Q, R)
    Kb, Pb = dare_wide(np.stack([A, A2]), np.stack([B, B2]), Q, R)
    assert Kb.shape == (2, 17, 12) and Pb.shape == (2, 12, 12)
    np.testing.assert_array_equal(Pb[0], P); np.testing.assert_array_equal(Kb[0], K)
    close(Pb[1], sl.solve_discrete_are(A2, B2, Q, R), 1e-9)
    Rbad = R.copy(); Rbad[5, 5] = -1.0
    with pytest.raises(Exception, match='not positive definite'):
        dare_wide(A, B, Q, Rbad)
    with pytest.raises(Exception):
        dare(A, B, Q, R)                         # sric_dare keeps its n_u <= 16


# ------------------------------------------------------------------------------------------------ LinearROM vs g23
def lin_rom(g, dt, with_H=True):
    import scipy.sparse as sp
    from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
    data = dict(A_c=g['model_A_c'][0], B_c=g['model_B_c'][0], d_c=g['model_d_c'][0],
                rom_info=dict(type='POD', U=g['U'], q_ref=g['q_ref'], v_ref=g['v_ref']))
    return LinearROM(data, dt, Cf=sp.csr_matrix(g['Cf']), Hf=sp.csr_matrix(g['Hf']) if with_H else None)


def test_linear_rom_against_golden(g):
    m = lin_rom(g, float(g['dt']))
    for k in ('A_d', 'B_d', 'd_d'):
        close(getattr(m, k), g['rom_' + k], 1e-10)
    for k in ('C', 'y_ref', 'H', 'z_ref'):
        close(getattr(m, k), g['rom_' + k], 1e-12)
    for k in ('state_dim', 'N', 'input_dim', 'meas_dim', 'output_dim'):
        assert getattr(m, k) == int(g['rom_' + k])
    assert (m.get_state_dim(), m.get_input_dim(), m.get_meas_dim(), m.get_output_dim()) == (8, 3, 30, 6)
    X = g['conv_x']
    close(m.x_to_zfyf(X, zf=True), g['conv_zf'], 1e-12)
    close(m.x_to_zfyf(X, yf=True), g['conv_yf'], 1e-12)
    close(m.x_to_zy(X, z=True), g['conv_z'], 1e-12)
    close(m.x_to_zfyf(X[0], zf=True), g['conv_x1_zf'], 1e-12)
    close(m.zfyf_to_zy(zf=g['conv_zf']), g['conv_zf_to_z'], 1e-12)
    close(m.zfyf_to_zy(yf=g['conv_yf']), g['conv_yf_to_y'], 1e-12)
    close(m.zy_to_zfyf(z=g['conv_z']), g['conv_z_to_zf'], 1e-12)
    close(m.zy_to_zfyf(y=g['conv_yf_to_y']), g['conv_y_to_yf'], 1e-12)
    # the two defects of the reference that are not kept: x_to_zy(y=True) maps the state, get_rom_info returns the basis
    close(m.x_to_zy(X, y=True), g['conv_yf'] - g['rom_y_ref'], 1e-12)
    assert m.get_rom_info()['type'] == 'POD'
    close(np.stack([m.update_state(x, np.array([100., 200., 300.])) for x in X]), g['conv_update_state'], 1e-10)
    A, B, d = m.get_jacobians(X[0], 0.3)
    assert A is m.A_d and B is m.B_d and d is m.d_d
    noH = lin_rom(g, float(g['dt']), with_H=False)
    assert noH.H is None and noH.z_ref is None and noH.output_dim is None
    close(noH.x_to_zfyf(X, yf=True), g['conv_noH_yf'], 1e-12)
    with pytest.raises(RuntimeError):
        noH.x_to_zfyf(X, zf=True)
    with pytest.raises(NotImplementedError):
        from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
        LinearROM(dict(A_c=g['model_A_c'][0], B_c=g['model_B_c'][0], d_c=g['model_d_c'][0], rom_info=dict(type='SSM')), 0.01)


# ------------------------------------------------------------------------------------------------ observer vs g23
def test_observer_gain_against_golden(g):
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    m = lin_rom(g, float(g['dt']))
    ob = DiscreteLuenbergerObserver(m, g['cost_Q'], g['costL_R'])
    print('observer gain: err %.3e of %.3e' % (np.abs(ob.L - g['L']).max(), np.abs(g['L']).max()))
    close(ob.L, g['L'], 1e-8)
    assert ob.C is m.C


@pytest.mark.parametrize('with_H', [True, False])
def test_observer_trace_against_golden(g, with_H):
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    m = lin_rom(g, float(g['dt']), with_H=with_H)
    ob = DiscreteLuenbergerObserver(m, g['cost_Q'], g['costL_R'])
    ob.L = g['L']
    tag = 'obs_H_' if with_H else 'obs_noH_'
    ob.initialize(g['obs_xf0'])
    assert ob.stats()['waits_last_step'] == 1
    xs, zs = [ob.x.copy()], [ob.z.copy()]
    for k in range(g['obs_u'].shape[0]):
        ob.update(g['obs_u'][k], g['obs_yf'][k])
        xs.append(ob.x.copy()); zs.append(ob.z.copy())
    xs, zs = np.stack(xs), np.stack(zs)
    assert xs.shape == g[tag + 'x'].shape and zs.shape == g[tag + 'z'].shape
    print('observer trace (H %s): x err %.3e, z err %.3e' % (with_H, np.abs(xs - g[tag + 'x']).max(), np.abs(zs - g[tag + 'z']).max()))
    close(xs, g[tag + 'x'], 1e-9); close(zs, g[tag + 'z'], 1e-9)
    ob.update_z()
    np.testing.assert_array_equal(ob.z, zs[-1])


# ------------------------------------------------------------------------------------------------ step / replay kernels
class _Sys:
    """The attributes of a LinearROM that the observer reads."""
    pass


_SYS = {}


def rand_sys(n, m, ny, nz, with_rom):
    key = (n, m, ny, nz, with_rom)
    if key in _SYS:
        return _SYS[key]
    rng = np.random.default_rng(1000 * n + 10 * ny + m)
    s = _Sys()
    s.A_d = 0.9 * np.linalg.qr(rng.standard_normal((n, n)))[0]
    s.B_d = rng.standard_normal((n, m)) / np.sqrt(m)
    s.d_d = 0.1 * rng.standard_normal(n)
    s.C = rng.standard_normal((ny, n)) / np.sqrt(n)
    s.y_ref = rng.standard_normal(ny)
    s.H = rng.standard_normal((nz, n)) / np.sqrt(n)
    s.z_ref = rng.standard_normal(nz)
    s.Lg = 0.3 * rng.standard_normal((n, ny)) / np.sqrt(ny)
    s.Kg = 0.3 * rng.standard_normal((m, n)) / np.sqrt(n)
    s.rom = None
    if with_rom:
        from sofacontrol_amd.mor.pod import POD
        r = n // 2
        n_f = 3 * (r // 3 + 5)
        U = np.linalg.qr(rng.standard_normal((n_f, r)))[0]
        s.rom = POD(dict(U=U, q_ref=rng.uniform(-100, 100, n_f), v_ref=0.01 * rng.standard_normal(n_f)))
    _SYS[key] = s
    return s


def np_step(s, x, y, u=None, ubar=None, xbar=None):
    """rompc.py:79 and observer.py:37-46 on rows of x."""
    if u is None:
        u = ubar + (x - xbar) @ s.Kg.T
    xn = x @ s.A_d.T + u @ s.B_d.T + s.d_d + ((y - s.y_ref) - x @ s.C.T) @ s.Lg.T
    return u, xn, xn @ s.H.T + s.z_ref


def make_observer(s, batch):
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    ob = DiscreteLuenbergerObserver(s, None, None, batch=batch, L=s.Lg)
    ob.K = s.Kg
    return ob


SHAPES = [(8, 3, 30, 6), (33, 4, 17, 6), (60, 4, 30, 6), (72, 8, 30, 6), (80, 16, 64, 16)]


@pytest.mark.parametrize('batch', [1, 16, 17, 64, 300])
@pytest.mark.parametrize('n,m,ny,nz', SHAPES)
def test_step_kernel_against_numpy(n, m, ny, nz, batch):
    with_rom = n % 2 == 0 and n <= 72
    s = rand_sys(n, m, ny, nz, with_rom)
    rng = np.random.default_rng(batch + n)
    ob = make_observer(s, batch)
    sh = (lambda a: a[0]) if batch == 1 else (lambda a: a)
    x = rng.standard_normal((batch, n))
    ob.set_state(sh(x))
    close(np.reshape(ob.z, (batch, nz)), x @ s.H.T + s.z_ref, 1e-9)
    worst = 0.0
    for k in range(3):                                       # u given, then the feedback, alternating
        y = rng.standard_normal((batch, ny))
        if k % 2 == 0:
            ug = rng.standard_normal((batch, m))
            u_ref, x_ref, z_ref = np_step(s, x, y, u=ug)
            u = ob.step(sh(y), u=sh(ug))
        else:
            ub, xb = rng.standard_normal((batch, m)), x + 0.1 * rng.standard_normal((batch, n))
            u_ref, x_ref, z_ref = np_step(s, x, y, ubar=ub, xbar=xb)
            u = ob.step(sh(y), ubar=sh(ub), xbar=sh(xb))
        assert ob.stats()['waits_last_step'] == 1
        got = [np.reshape(a, b.shape) for a, b in ((u, u_ref), (ob.x, x_ref), (ob.z, z_ref))]
        worst = max(worst, max(np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in zip(got, (u_ref, x_ref, z_ref))))
        close(got[0], u_ref, 1e-9); close(got[1], x_ref, 1e-9); close(got[2], z_ref, 1e-9)
        x = got[1]
    if with_rom:
        # the full-state path: initialize inside the step, then the same update
        nf2 = 2 * s.rom.U.shape[0]
        xf = s.rom.x_ref + rng.standard_normal((batch, nf2))
        x0 = (xf - s.rom.x_ref) @ s.rom.V
        y, ug = rng.standard_normal((batch, ny)), rng.standard_normal((batch, m))
        u_ref, x_ref, z_ref = np_step(s, x0, y, u=ug)
        ob.step(sh(y), u=sh(ug), xf=sh(xf))
        assert ob.stats()['waits_last_step'] == 1
        worst = max(worst, np.abs(np.reshape(ob.x, x_ref.shape) - x_ref).max() / max(1.0, np.abs(x_ref).max()))
        close(np.reshape(ob.x, x_ref.shape), x_ref, 1e-9); close(np.reshape(ob.z, z_ref.shape), z_ref, 1e-9)
        ob.initialize(sh(xf))
        assert ob.stats()['waits_last_step'] == 1
        close(np.reshape(ob.x, x0.shape), x0, 1e-9); close(np.reshape(ob.z, z_ref.shape), x0 @ s.H.T + s.z_ref, 1e-9)
    print('step (%d, %d, %d, %d) batch %d: worst scaled error %.3e' % (n, m, ny, nz, batch, worst))
    assert ob.stats()['steps'] == (4 if with_rom else 3)


@pytest.mark.parametrize('n,m,ny,nz', SHAPES)
def test_problem_of_a_batch_equals_the_problem_alone(n, m, ny, nz):
    s = rand_sys(n, m, ny, nz, False)
    rng = np.random.default_rng(n)
    B = 35
    x, y = rng.standard_normal((B, n)), rng.standard_normal((2, B, ny))
    ub, xb, ug = rng.standard_normal((B, m)), rng.standard_normal((B, n)), rng.standard_normal((B, m))
    ob = make_observer(s, B)
    ob.set_state(x)
    u1 = ob.step(y[0], u=ug); x1, z1 = ob.x.copy(), ob.z.copy()
    u2 = ob.step(y[1], ubar=ub, xbar=xb); x2, z2 = ob.x.copy(), ob.z.copy()
    one = make_observer(s, 1)
    for b in (0, 15, 16, 34):
        one.set_state(x[b])
        one.step(y[0, b], u=ug[b])
        assert rel(one.x, x1[b]) <= 1e-12 and rel(one.z, z1[b]) <= 1e-12
        v = one.step(y[1, b], ubar=ub[b], xbar=xb[b])
        assert rel(v, u2[b]) <= 1e-12 and rel(one.x, x2[b]) <= 1e-12 and rel(one.z, z2[b]) <= 1e-12


@pytest.mark.parametrize('batch', [17, 64])
def test_replay_equals_steps_and_numpy(batch):
    n, m, ny, nz = 72, 8, 30, 6
    T = 40
    s = rand_sys(n, m, ny, nz, False)
    rng = np.random.default_rng(7 + batch)
    x0 = rng.standard_normal((batch, n))
    Y = rng.standard_normal((T, batch, ny))
    Ub, Xb = rng.standard_normal((T, batch, m)), rng.standard_normal((T, batch, n))
    Ug = rng.standard_normal((T, batch, m))
    for feedback in (True, False):
        ob = make_observer(s, batch)
        ob.set_state(x0)
        U, X, Z = ob.replay(Y, ubar=Ub, xbar=Xb) if feedback else ob.replay(Y, U=Ug)
        assert ob.stats()['waits_last_step'] == 1 and ob.stats()['steps'] == T
        np.testing.assert_array_equal(ob.x, X[-1])
        st = make_observer(s, batch)
        st.set_state(x0)
        x = x0
        worst_np, worst_st = 0.0, 0.0
        for t in range(T):
            if feedback:
                u = st.step(Y[t], ubar=Ub[t], xbar=Xb[t]); u_ref, x, z_ref = np_step(s, x, Y[t], ubar=Ub[t], xbar=Xb[t])
            else:
                u = st.step(Y[t], u=Ug[t]); u_ref, x, z_ref = np_step(s, x, Y[t], u=Ug[t])
            worst_st = max(worst_st, rel(U[t], u), rel(X[t], st.x), rel(Z[t], st.z))
            worst_np = max(worst_np, max(np.abs(a - b).max() / max(1.0, np.abs(b).max())
                                         for a, b in ((U[t], u_ref), (X[t], x), (Z[t], z_ref))))
        print('replay batch %d feedback %s: vs steps %.3e, vs numpy %.3e' % (batch, feedback, worst_st, worst_np))
        assert worst_st <= 1e-12
        assert worst_np <= 1e-9


# ------------------------------------------------------------------------------------------------ ROMPC.evaluate vs g23
class ExactClient:
    """MPCClientNode protocol answered by the oracle's exact QP on the reference's MPC model: the maker's stub."""

    def __init__(self, g):
        self.g = g
        self.sol = None

    def send_request(self, t0, x0, wait=True):
        from scipy.interpolate import interp1d
        from oracle import locp as olocp
        g = self.g
        N, dt = int(g['qp_N']), float(g['qp_dt'])
        t = t0 + dt * np.arange(N + 1)
        z = interp1d(g['qp_t'], g['qp_z'], axis=0, bounds_error=False, fill_value=(g['qp_z'][0], g['qp_z'][-1]))(t)
        A, B, d = g['mpc_A_d'], g['mpc_B_d'], g['mpc_d_d']
        qp = olocp.build_qp(N, g['mpc_H'], g['qp_Q'], g['qp_R'], [A] * N, [B] * N, [d] * N, np.asarray(x0, float), None, 0.0, 0.0,
                            z=z, U=(g['qp_UA'], g['qp_Ub']), tr_active=False)
        w, _, _ = olocp.solve_exact(qp)
        x, u, _ = olocp.split(qp, w)
        self.sol = (t, u, x)

    def force_spin(self):
        pass

    def check_if_done(self):
        return True

    def force_wait(self):
        pass

    def get_solution(self, n_x, n_u):
        t, u, x = self.sol
        return t, u, x, 0.0


def solver_node(g):
    from sofacontrol_amd.baselines.mpc import MPCSolverNode
    from sofacontrol_amd.tpwl.tpwl_utils import Target
    from sofacontrol_amd.utils import QuadraticCost, Polyhedron
    target = Target()
    target.t, target.z = g['qp_t'], g['qp_z']
    cp = QuadraticCost(Q=g['qp_Q'], R=g['qp_R'])
    return MPCSolverNode(lin_rom(g, float(g['qp_dt'])), int(g['qp_N']), float(g['qp_dt']), cp, target,
                         U=Polyhedron(g['qp_UA'], g['qp_Ub']))


def run_trace(g, tag, mode, own_gains=False):
    import scipy.sparse as sp
    from sofacontrol_amd.baselines.rompc.rompc import ROMPC
    from sofacontrol_amd.utils import QuadraticCost
    dt = float(g[tag + 'dt'])
    model = lin_rom(g, dt)
    cost = QuadraticCost(Q=model.H.T @ g['Qz'] @ model.H, R=g['cost_R'])
    costL = QuadraticCost(Q=cost.Q, R=g['costL_R'])
    kw = dict(client=ExactClient(g)) if mode == 'client' else dict(solver_node=solver_node(g))
    with contextlib.redirect_stdout(io.StringIO()):
        c = ROMPC(model, cost, costL, dt, N_replan=int(g[tag + 'N_replan']), delay=float(g[tag + 'delay']), **kw)
    if not own_gains:
        c.K = g['K' if tag == 'tr_' else 'K_hw']
        c.observer.L = g['L' if tag == 'tr_' else 'L_hw']
    Cf = sp.csr_matrix(g['Cf'])
    xf = g[tag + 'xf']
    us, xs = [], []
    u_prev = np.zeros(model.input_dim)
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(int(g[tag + 'steps'])):
            u_prev = c.evaluate(dt * k, Cf @ xf[k], xf[k], u_prev)
            us.append(u_prev); xs.append(c.observer.x.copy())
            if k > 0:
                assert c.observer.stats()['waits_last_step'] == 1
    return c, np.stack(us), np.stack(xs)


def check_trace(g, tag, c, us, xs):
    req_t = np.array([r[0] for r in c.requests]); req_x = np.stack([r[1] for r in c.requests])
    n_start = int(round(float(g[tag + 'delay']) / float(g[tag + 'dt'])))
    info = c.save_controller_info()
    print('trace %s: request states rel %.3e, start-up estimates %.3e, all estimates %.3e, u %.3e of %.3e, u_opt %.3e of %.3e'
          % (tag, rel(req_x, g[tag + 'req_x0']), np.abs(xs[:n_start] - g[tag + 'xhat'][:n_start]).max(),
             np.abs(xs - g[tag + 'xhat']).max(), np.abs(us - g[tag + 'u']).max(), np.abs(g[tag + 'u']).max(),
             np.abs(info['u_opt'] - g[tag + 'u_opt']).max(), np.abs(g[tag + 'u_opt']).max()))
    np.testing.assert_array_equal(req_t, g[tag + 'req_t'])
    assert rel(req_x, g[tag + 'req_x0']) <= 1e-12
    close(xs[:n_start], g[tag + 'xhat'][:n_start], 1e-9)
    assert np.abs(us - g[tag + 'u']).max() <= 1e-6 * np.abs(g[tag + 'u']).max()
    assert np.abs(info['u_opt'] - g[tag + 'u_opt']).max() <= 1e-6 * np.abs(g[tag + 'u_opt']).max()
    np.testing.assert_array_equal(info['t_opt'], g[tag + 't_opt'])
    assert set(info) == {'t_opt', 'u_opt', 'z_opt', 'solve_times', 'rollout_time'}
    for k in ('t_opt', 'u_opt', 'z_opt'):
        assert np.shape(info[k]) == g[tag + k].shape, k
    assert len(info['solve_times']) == int(g[tag + 'n_solves'])
    assert info['rollout_time'] == float(g[tag + 'rollout_time'])


@pytest.mark.parametrize('mode', ['client', 'solver_node'])
@pytest.mark.parametrize('tag', ['tr_', 'hw_'])
def test_evaluate_trace(g, tag, mode):
    """Measured on an MI355X (scaled as the assertions are): see the figures printed by check_trace."""
    c, us, xs = run_trace(g, tag, mode)
    check_trace(g, tag, c, us, xs)


def test_evaluate_trace_with_device_gains(g):
    """K from sric_dare, L from sric_dare_wide (the controller's own): the inputs of the reference's run at 1e-6."""
    c, us, xs = run_trace(g, 'tr_', 'client', own_gains=True)
    close(c.K, g['K'], 1e-8)
    print('own gains: u err %.3e of %.3e' % (np.abs(us - g['tr_u']).max(), np.abs(g['tr_u']).max()))
    assert np.abs(us - g['tr_u']).max() <= 1e-6 * np.abs(g['tr_u']).max()
    np.testing.assert_array_equal(np.array([r[0] for r in c.requests]), g['tr_req_t'])


# ------------------------------------------------------------------------------------------------ refusals, example
def test_refusals(g):
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    from sofacontrol_amd.baselines.rompc.rompc import ROMPC
    from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
    from sofacontrol_amd.utils import QuadraticCost
    s = _Sys()
    rng = np.random.default_rng(3)
    n, m, ny, nz = 200, 4, 64, 6
    s.A_d, s.B_d, s.d_d = 0.5 * np.eye(n), rng.standard_normal((n, m)), np.zeros(n)
    s.C, s.y_ref, s.H, s.z_ref = rng.standard_normal((ny, n)), np.zeros(ny), rng.standard_normal((nz, n)), np.zeros(nz)
    s.rom = None
    with pytest.raises(RuntimeError, match='srompc_create'):
        DiscreteLuenbergerObserver(s, None, None, L=np.zeros((n, ny)))
    # 80 x 64 without an output model: C would have to stay in LDS as the output map, which does not fit
    t = rand_sys(80, 16, 64, 16, False)
    u = _Sys()
    u.__dict__.update(t.__dict__)
    u.H = u.z_ref = None
    with pytest.raises(RuntimeError, match='srompc_create'):
        DiscreteLuenbergerObserver(u, None, None, L=t.Lg)
    data = dict(A_c=g['model_A_c'][0], B_c=g['model_B_c'][0], d_c=g['model_d_c'][0],
                rom_info=dict(type='POD', U=g['U'], q_ref=g['q_ref'], v_ref=g['v_ref']))
    bare = LinearROM(data, 0.01)
    with pytest.raises(RuntimeError, match='meas. model'):
        DiscreteLuenbergerObserver(bare, np.eye(8), np.eye(30))
    model = lin_rom(g, 0.01)
    cost = QuadraticCost(Q=g['cost_Q'], R=g['cost_R'])
    with pytest.raises(RuntimeError, match='client'):
        ROMPC(model, cost, QuadraticCost(Q=g['cost_Q'], R=g['costL_R']), 0.01)


def test_closed_loop_example_runs():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'diamond_rompc_closed_loop.py'), '--steps', '60'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('rompc closed loop')]
    assert line and '60 steps, 6 solves' in line[0], r.stdout[-2000:]
