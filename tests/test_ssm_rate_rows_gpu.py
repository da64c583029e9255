"""GPU: input-rate rows dU.A (u_{k+1} - u_k) <= dU.b (locp.py:305-308) inside the one-launch SSM GuSTO solve (csrc/gusto_ssm.hip, rows of the
one-wave QP in the space of the inputs, csrc/locp_dense_u.h) against oracle.gusto.solve_generic, whose exact QP knows rate rows; the
hand-back of a rollout whose trust region binds (status SSM_NEEDS_HOST -> the host loop); device path against host loop.
Shape: the three-output problem of test_ssm_gpu.py (n_x = 6, n_u = 4, N = 3), the smallest at which the hardware loop's QP is posed."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ssm as ossm, gusto as ogusto
from test_ssm_gpu import product_ssm, close

pytestmark = pytest.mark.gpu

n, m, dt = 6, 4, 0.02
BOX = object()          # U = HyperRectangle([3] * 4, [-1] * 4)


@functools.lru_cache(maxsize=None)
def synthetic():
    return ossm.synthetic(n, m, 3, 2, seed=96)


def rate_box(r):
    return np.kron(np.eye(m), np.array([[1.0], [-1.0]])), np.full(2 * m, float(r))


RISE = (np.kron(np.eye(m), np.array([[1.0], [-1.0]])), np.tile([0.5, -0.1], m))      # 0.1 <= u_{k+1} - u_k <= 0.5


def setup(N):
    """Model, initial trajectory, cost and target of the three-output case for a horizon of N stages."""
    from sofacontrol_amd.utils import HyperRectangle
    model = synthetic()
    s = product_ssm(model, discr='be')
    x0 = 0.05 * np.random.default_rng(5).standard_normal(n)
    u_init = np.zeros((N, m))
    x_init, _ = s.rollout(x0, u_init, dt)
    Qz = np.zeros((n, n)); Qz[0, 0] = Qz[1, 1] = Qz[2, 2] = 100.0
    R = 1e-3 * np.eye(m)
    z = np.tile(ossm.observe(model, x0) + np.array([0.02, -0.01, 0.015, 0, 0, 0]), (N + 1, 1))
    return dict(model=model, s=s, x0=x0, u_init=u_init, x_init=x_init, Qz=Qz, R=R, z=z, U=HyperRectangle([3.0] * m, [-1.0] * m), N=N)


_oracle = {}


def oracle(key, P, U, dU, **kw):
    """oracle.gusto.solve_generic on the case, once per key."""
    if key not in _oracle:
        model, N = P['model'], P['N']
        _oracle[key] = ogusto.solve_generic(
            lambda x, u: ossm.jacobians(model, x, u, dt, 'be'),
            lambda x, u: (lambda A, B, d: (A @ x + B @ u + d, A, B))(*ossm.continuous_jacobians(model, x, u)),
            np.zeros((n, n)), N, dt, P['Qz'], P['R'], P['x0'], P['u_init'], P['x_init'], z=P['z'],
            U=None if U is None else (U.A, U.b), dU=dU, obs_lin=lambda x: ossm.observer_jacobians(model, x),
            convg_thresh=1e-5, max_gusto_iters=4, **kw)
    return _oracle[key]


def gusto(P, U, dU, **kw):
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    return GuSTO(SSMGuSTO(P['s']), P['N'], dt, P['Qz'], P['R'], P['x0'], P['u_init'], P['x_init'], z=P['z'], U=U,
                 dU=None if dU is None else Polyhedron(dU[0], dU[1]), verbose=0, max_gusto_iters=4, first_solve_cap=4, convg_thresh=1e-5, **kw)


def follows_oracle(g, ref):
    xo, uo, _, tr = ref
    print('SCP iterations %d (oracle %d); max |xopt - oracle| %.3e, max |uopt - oracle| %.3e, max |trace - oracle| %.3e' %
          (int(g.iters[0]), len(tr), np.abs(g.xopt - xo).max(), np.abs(g.uopt - uo).max(),
           np.abs(g.trace[0, :len(tr), :3] - np.asarray(tr, dtype=float)[:, :3]).max() if int(g.iters[0]) == len(tr) else np.nan))
    assert int(g.iters[0]) == len(tr)
    close(g.xopt, xo, 1e-6); close(g.uopt, uo, 1e-5)
    close(g.trace[0, :len(tr), :3], np.asarray(tr, dtype=float)[:, :3], 1e-6)


# (horizon, input set, rate polyhedron, SCP iterations of the oracle)
CASES = {
    'box_0p2': (3, BOX, rate_box(0.2), 3),
    'box_0p05': (3, BOX, rate_box(0.05), 4),
    'rise_negative_b': (3, BOX, RISE, 4),
    'rate_rows_only': (3, None, rate_box(0.2), 4),
    'full_tile_N4': (4, BOX, rate_box(0.2), 3),
}


@pytest.mark.parametrize('tag', sorted(CASES))
def test_rate_rows_in_the_one_launch_solve_follow_the_oracle(tag):
    """Rate rows binding (+-0.2: five active at the oracle's optimum; +-0.05: seven), a rate polyhedron that excludes the zero increment
    (0.1 <= du <= 0.5: the interior point starts infeasible), rate rows without an input box (nU = 0), and N = 4 (16 inputs, 32 + 24 = 56
    rows: the full tile).  Every SCP step of these stays inside the trust region: the whole solve is one launch, nothing goes to the host."""
    N, U, dU, its = CASES[tag]
    P = setup(N)
    U = P['U'] if U is BOX else None
    g = gusto(P, U, dU)
    assert g._ssm and g._fused
    assert g.kernel_info['rate_rows'] == 8
    assert g.kernel_info['handed_to_host'] == 0
    ref = oracle(tag, P, U, dU)
    assert len(ref[3]) == its                       # (what the oracle gave when the case was chosen)
    follows_oracle(g, ref)
    du = np.diff(g.uopt, axis=0)
    print('increments of uopt: min %.6f, max %.6f' % (du.min(), du.max()))
    if tag == 'rise_negative_b':
        assert du.min() >= 0.1 - 2e-5 and du.max() <= 0.5 + 2e-5
        assert du.min() <= 0.1 + 2e-5 and du.max() >= 0.5 - 2e-5          # both ends attained
    else:
        r = float(dU[1][0])
        assert np.abs(du).max() <= r + 2e-5
        assert np.abs(du).max() >= r - 2e-5         # rate rows are active at the optimum


def test_one_stage_horizon_has_no_rate_rows():
    """N = 1: no pair of stages, so dU adds no row and the kernel does the arithmetic of the dU = None solve."""
    P = setup(1)
    ga = gusto(P, P['U'], rate_box(0.2))
    gb = gusto(P, P['U'], None)
    assert ga._ssm and gb._ssm and ga.kernel_info['rate_rows'] == 8 and gb.kernel_info['rate_rows'] == 0
    assert ga.kernel_info['handed_to_host'] == 0
    np.testing.assert_array_equal(ga.iters, gb.iters)
    np.testing.assert_array_equal(ga.xopt, gb.xopt)
    np.testing.assert_array_equal(ga.uopt, gb.uopt)
    np.testing.assert_array_equal(ga.trace, gb.trace)


def test_trust_region_binding_goes_back_to_the_host_loop():
    """delta0 = 0.02: the first relaxed minimiser moves the state by 0.152 and leaves the trust region.  The kernel's full-row QP knows no rate
    rows, so the rollout comes back with SSM_NEEDS_HOST and the host loop solves it from the original arguments: the oracle's five QPs."""
    P = setup(3)
    g = gusto(P, P['U'], rate_box(0.2), delta0=0.02)
    assert g._ssm and g.kernel_info['rate_rows'] == 8
    assert g.kernel_info['handed_to_host'] == 1
    assert int(g.status[0]) in (0, 3)
    ref = oracle('hand_back', P, P['U'], rate_box(0.2), delta0=0.02)
    assert len(ref[3]) == 5
    follows_oracle(g, ref)
    assert np.abs(np.diff(g.uopt, axis=0)).max() <= 0.2 + 2e-5


def test_receding_horizon_device_equals_host_loop_with_rate_rows(monkeypatch):
    """The receding-horizon sequence of test_gusto_ssm_real_time_iteration_device_equals_host_loop (max_gusto_iters = 0: one QP per call) with
    dU = +-0.2: device path against the host loop around the state-augmented QP; a batch of four against four single solves; the kept
    solver state (the rate rows' multipliers are among the 64)."""
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import HyperRectangle
    N = 3
    model = synthetic()
    rng = np.random.default_rng(12)
    Qz = np.zeros((n, n)); Qz[0, 0] = Qz[1, 1] = 100.0
    R = 0.003 * np.eye(m)
    U = HyperRectangle([1500.0] * m, [0.0] * m)
    dU = HyperRectangle([0.2] * m, [-0.2] * m)
    x0s = 0.05 * rng.standard_normal((4, n))
    z = np.tile(np.array([0.02, -0.01, 0, 0, 0, 0.0]), (N + 1, 1))
    res = {}
    for path in ('device', 'host'):
        if path == 'host':
            monkeypatch.setenv('SRH_GUSTO_SSM_HOST_LOOP', '1')
        else:
            monkeypatch.delenv('SRH_GUSTO_SSM_HOST_LOOP', raising=False)
        s = product_ssm(model, discr='be')
        gm = SSMGuSTO(s)
        u0 = np.zeros((N, m))
        xi, _ = s.rollout(x0s[0], u0, dt)
        g = GuSTO(gm, N, dt, Qz, R, x0s[0], u0, xi, z=z, U=U, dU=dU, verbose=0, max_gusto_iters=0, convg_thresh=1e-3)
        assert g._ssm == (path == 'device')
        out = [(g.xopt.copy(), g.uopt.copy(), int(g.iters[0]))]
        for b in range(1, 4):
            xi, _ = s.rollout(x0s[b], out[-1][1], dt)
            g.solve(x0s[b], out[-1][1], xi, z, None, None)
            assert int(g.iters[0]) == 1
            out.append((g.xopt.copy(), g.uopt.copy(), 1))
        if path == 'device':
            print('rollouts handed to the host over the sequence: %d' % g.kernel_info['handed_to_host'])
        res[path] = out
    for a, b in zip(res['device'], res['host']):
        print('device - host loop: x %.3e, u %.3e; max |du| %.6f' % (np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(np.diff(a[1], axis=0)).max()))
    for a, b in zip(res['device'], res['host']):
        assert a[2] == b[2]
        close(a[0], b[0], 1e-7); close(a[1], b[1], 1e-6)
        assert np.abs(np.diff(a[1], axis=0)).max() <= 0.2 + 2e-5
    # a batch of four rollouts in one launch equals four single solves
    monkeypatch.delenv('SRH_GUSTO_SSM_HOST_LOOP', raising=False)
    s = product_ssm(model, discr='be')
    gm = SSMGuSTO(s)
    u0 = np.zeros((4, N, m))
    xi = np.stack([s.rollout(x0s[b], u0[b], dt)[0] for b in range(4)])
    zb = np.tile(z, (4, 1, 1))
    gb = GuSTO(gm, N, dt, Qz, R, x0s, u0, xi, z=zb, U=U, dU=dU, verbose=0, max_gusto_iters=3, convg_thresh=1e-3, batch=4, first_solve_cap=3)
    g1 = GuSTO(gm, N, dt, Qz, R, x0s[0], u0[0], xi[0], z=z, U=U, dU=dU, verbose=0, max_gusto_iters=3, convg_thresh=1e-3, first_solve_cap=3,
               keep_solver_state=True)
    assert gb._ssm and g1._ssm and gb.kernel_info['rate_rows'] == 8
    assert g1.solver_state_kept
    for b in range(4):
        g1.solve(x0s[b], u0[b], xi[b], z, None, None)
        assert int(g1.iters[0]) == int(gb.iters[b])
        close(gb.xopt[b], g1.xopt, 1e-7); close(gb.uopt[b], g1.uopt, 1e-6)
    # the same problem again, now from the minimiser and multipliers the solve before it left: the same plan
    first = (g1.xopt.copy(), g1.uopt.copy(), int(g1.iters[0]))
    g1.solve(x0s[3], u0[3], xi[3], z, None, None)
    assert int(g1.iters[0]) == first[2]
    close(g1.xopt, first[0], 1e-7); close(g1.uopt, first[1], 1e-6)


def test_too_many_inputs_for_the_tile_are_refused_and_run_on_the_host_loop():
    """N n_u = 20 > 16 with rate rows: sgusto_ssm_plan_create names the limit, GuSTO takes the host loop and still follows the oracle."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.locp import make_problem
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    P = setup(5)
    dU = rate_box(0.2)
    Ha = np.hstack((np.zeros((n, n)), np.eye(n)))
    prob, keep = make_problem(5, Ha, P['Qz'], P['R'], None, P['U'], None, None, Polyhedron(*dU), np.concatenate((np.ones(n), np.zeros(n))))
    assert prob.ndU == 8
    g0 = GuSTO.__new__(GuSTO)
    for k, v in dict(delta0=1e4, omega0=1, rho=0.1, beta_fail=0.5, gamma_fail=5, epsilon=0.01, omega_max=1e10, convg_thresh=1e-5).items():
        setattr(g0, k, v)
    par = GuSTO._params(g0, 4)
    plan = C.c_void_p()
    Hm = _lib.f64(np.zeros((n, n)))
    fc = _lib.f64(np.ones(n))
    rc = _lib.lib().sgusto_ssm_plan_create(C.byref(plan), P['s'].handle, C.byref(prob), C.byref(par), C.c_double(dt), C.c_int(P['s']._mode()),
                                           C.c_int64(1), _lib.dptr(fc), _lib.dptr(Hm), C.c_int(0), None, None, C.c_int(8))
    msg = _lib.lib().srh_last_error().decode()
    assert rc != 0 and not plan
    assert 'N n_u <= 16' in msg and 'rate rows' in msg, msg
    g = gusto(P, P['U'], dU)
    assert not g._ssm and not g._fused
    follows_oracle(g, oracle('refused_N5', P, P['U'], dU))
    assert np.abs(np.diff(g.uopt, axis=0)).max() <= 0.2 + 2e-5
