"""GPU: the Riccati and iLQR kernels of csrc/lqr.hip against exact linear-quadratic solutions in long double
(tests/lq_reference.py), on every backward-pass path and at the edges of the dispatch.

Tolerance rule (every comparison with the long-double reference): tol = max(100 e_oracle, 1e-13), e_oracle = the error of
the float64 statement in oracle/lqr.py against the same reference on the same inputs, computed here; the factor 100 covers
the kernels' different but equally legitimate float64 evaluation order (MFMA k-blocks of 4, Cholesky solves where the
oracle inverts, fma chains).  Input condition: e_oracle <= 1e-11 (asserted; tests/test_lq_reference_cpu.py asserts the same
without a GPU).  Error measure: max|a - b| / max(1, max|b|).  Every figure is printed before it is asserted (pytest -s)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import lq_cases as lc
import lq_reference as lr
from helpers import golden_problem, product_tpwl, ilqr_batch_equals_singles
from oracle import lqr as olqr, tpwl as otpwl

pytestmark = pytest.mark.gpu

E_ORACLE_MAX = 1e-11
LDS_MESSAGE = 'silqr_solve: state dimension too large for LDS'


def tolerance(e_oracle):
    assert e_oracle <= E_ORACLE_MAX, e_oracle
    return max(100.0 * e_oracle, 1e-13)


# ---------------------------------------------------------------------------------------------- iLQR: one exact Newton step
_CASES = {}


def prepared(shape):
    """The product model of a case and, per start (cold / warm), the long-double optimum and the oracle's error against
    it -- computed once per shape and shared by the default and the VALU runs."""
    if shape not in _CASES:
        c = lc.ilqr_case(*shape)
        tp = product_tpwl(c['model'], c['U'], c['q_ref'], c['v_ref'], c['Hf'])
        with contextlib.redirect_stdout(io.StringIO()):
            tp.pre_discretize(lc.DT)
        for A in tp.A_d[1:]:
            np.testing.assert_array_equal(A, tp.A_d[0])                # one affine map behind every point
        A, B, d, H, z_ref = tp.A_d[0], tp.B_d[0], tp.d_d[0], np.asarray(tp.H), np.asarray(tp.z_ref)
        assert H.shape == (c['nz'], 2 * c['r'])
        ref = lr.lq_tracking(A, B, d, H, z_ref, c['Q'], c['R'], c['Qf'], c['z_target'], c['x0'], c['N'])
        e_oracle = {}
        for start, uw in (('cold', None), ('warm', c['u_warm'])):
            o = lc.oracle_newton_step(A, B, d, H, z_ref, c, uw)
            e_oracle[start] = max(lr.err(a, b) for a, b in zip(o, ref))
        _CASES[shape] = (c, tp, ref, e_oracle)
    return _CASES[shape]


def newton_step(c, tp, switches, u_warm):
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    il = iLQR(lc.DT, tp, QuadraticCost(Q=c['Q'], R=c['R'], Qf=c['Qf']), c['N'])
    il.params.max_iter = 0                       # the kernel's loop is `it <= max_iter`: one backward and one forward pass
    il.params.include_input_var_constraint = False
    il.params.do_linesearch = il.params.regularize = il.params.state_regularization = switches
    assert il.params.rho0 == 0.0                 # the first backward pass is unregularised either way
    il.set_target(c['z_target'])
    x, u, K = il.ilqr_computation(c['x0'], u_warm)
    assert int(il.iters[0]) == 1
    return x, u, K, float(il.cost[0])


def check_exact_step(shape, index, no_mfma):
    c, tp, ref, e_oracle = prepared(shape)
    path = lc.ilqr_path(2 * c['r'], c['m'], no_mfma)
    assert path != 'refused'
    # half of the cases with every switch off, the other half with line search and (state) regularisation on: with
    # rho0 = 0 and an exact step (ratio 1, alpha = 1 accepted) both must land on the same optimum
    switches = index % 2 == 1
    worst = 0.0
    failures = []
    for start, uw in (('cold', None), ('warm', c['u_warm'])):
        tol = tolerance(e_oracle[start])
        got = newton_step(c, tp, switches, uw)
        errs = [lr.err(a, b) for a, b in zip(got, ref)]
        print('ilqr_exact shape (n_x %d, n_u %d, n_z %d, N %d) path %s switches %s start %s: err x %.2e u %.2e K %.2e cost %.2e '
              '| e_oracle %.2e tol %.2e' % (2 * c['r'], c['m'], c['nz'], c['N'], path, 'on' if switches else 'off', start,
                                            *errs, e_oracle[start], tol))
        worst = max(worst, *errs)
        if max(errs) > tol:
            failures.append((start, errs, tol))
    assert not failures, failures
    return worst


@pytest.mark.parametrize('index,shape', list(enumerate(lc.ILQR_SHAPES)), ids=lambda v: str(v).replace(' ', ''))
def test_ilqr_exact_newton_step(index, shape):
    """One iLQR iteration on an LQ problem is the exact Newton step: x, u, K and the cost equal the long-double optimum
    from a cold and from a random warm start (size ~1: K (x - x_prev) and alpha k are then non-trivial), on the MFMA
    panels in LDS (mfma1), on Jacobians read in place (mfma2) and -- (64, 16) fits neither -- on the VALU pass."""
    check_exact_step(shape, index, False)


@pytest.mark.parametrize('index,shape', list(enumerate(lc.VALU_SHAPES)), ids=lambda v: str(v).replace(' ', ''))
def test_ilqr_exact_newton_step_valu(index, shape, monkeypatch):
    """The VALU fallback (SRH_ILQR_NO_MFMA, read on every call): three shapes with [A|B] staged in LDS, and (74, 4), the
    largest n_x at n_u = 4 whose fallback fits only without staging (64 is the last staged, 76 is refused)."""
    monkeypatch.setenv('SRH_ILQR_NO_MFMA', '1')
    check_exact_step(shape, index, True)


@pytest.mark.parametrize('r,m,no_mfma', [(39, 4, False), (36, 8, False), (38, 4, True)])
def test_ilqr_refusal_sizes(r, m, no_mfma, monkeypatch):
    """The first sizes the paths refuse: n_x = 78 at n_u = 4 (76 runs on mfma2: it is in the exact-step list), n_u = 8 at
    n_x = 72 (7 runs), and n_x = 76 at n_u = 4 for the VALU fallback (74 runs): RuntimeError with the kernel's message."""
    if no_mfma:
        monkeypatch.setenv('SRH_ILQR_NO_MFMA', '1')
    assert lc.ilqr_path(2 * r, m, no_mfma) == 'refused'
    c = lc.ilqr_case(r, m, 6, 3)
    tp = product_tpwl(c['model'], c['U'], c['q_ref'], c['v_ref'], c['Hf'])
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(lc.DT)
    with pytest.raises(RuntimeError, match=LDS_MESSAGE):
        newton_step(c, tp, False, None)


# ------------------------------------------------------------------------------- iLQR: batch members against single solves
def golden_batch(golden, n_members=3):
    from test_lqr_gpu import setup
    g, tp = setup(golden)
    rng = np.random.default_rng(11)
    x0, zt, uw = g['c1_x0'], g['c1_z_target'], g['c1_uw']
    z_ref = np.asarray(tp.z_ref)
    scale = np.array([1.0, 0.6, 1.3])[:n_members]
    x0s = x0[None] * scale[:, None] * (1.0 + 0.1 * rng.standard_normal((n_members,) + x0.shape))
    zts = z_ref + (zt - z_ref)[None] * scale[:, None, None] * (1.0 + 0.1 * rng.standard_normal((n_members,) + zt.shape))
    uws = uw[None] * (1.0 + 0.2 * rng.standard_normal((n_members,) + uw.shape))
    uls = uw[0][None] * (1.0 + 0.2 * rng.standard_normal((n_members, uw.shape[1])))
    return g, tp, x0s, zts, uws, uls


@pytest.mark.parametrize('no_mfma', [False, True], ids=['mfma1', 'valu'])
def test_ilqr_batch_members_equal_single_solves(golden, no_mfma, monkeypatch):
    """Three DIFFERENT problems in one launch (x0, targets, warm start and u_last all differ): every member equals its
    single solve bit for bit -- a kernel reading problem 0's x0, target, u_last or work slice for every problem fails."""
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    if no_mfma:
        monkeypatch.setenv('SRH_ILQR_NO_MFMA', '1')
    g, tp, x0s, zts, uws, uls = golden_batch(golden)
    il = iLQR(0.05, tp, QuadraticCost(Q=g['Qz'], R=g['R'], Qf=g['Qf']), 10)
    ilqr_batch_equals_singles(il, x0s, zts, uws, uls)


def test_ilqr_batch_members_equal_single_solves_nx72():
    """The same on the MFMA-2 path (n_x = 72, n_u = 4: the problem of test_ilqr_diamond_sizes_vs_oracle)."""
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    r, m, N, dt = 36, 4, 15, 0.05
    model, U, q_ref, v_ref, Hf = golden_problem(r, m, 8, 40, 55, q_scale=0.2)
    tp = product_tpwl(model, U, q_ref, v_ref, Hf)
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(dt)
    assert lc.ilqr_path(2 * r, m) == 'mfma2'
    Qz = np.diag([0., 0., 0., 100., 100., 10.]); R = 1e-3 * np.eye(m)
    rng = np.random.default_rng(72)
    th = np.linspace(0, 1.0, N + 1)
    zts = np.zeros((3, N + 1, 6))
    for b, s in enumerate((1.0, 0.5, 1.5)):
        zts[b, :, 3] = -0.02 * s * np.sin(th); zts[b, :, 4] = 0.01 * s * np.sin(2 * th + 0.3 * b)
    zts = zts + np.asarray(tp.z_ref)
    x0s = 1e-3 * rng.standard_normal((3, 2 * r))
    uws = 5.0 * rng.standard_normal((3, N, m))
    uls = 5.0 * rng.standard_normal((3, m))
    il = iLQR(dt, tp, QuadraticCost(Q=Qz, R=R, Qf=10 * Qz), N)
    ilqr_batch_equals_singles(il, x0s, zts, uws, uls)


# ----------------------------------------------------------------------------------- iLQR over the SSM model: claimed forms
def c3_solve(members=2):
    import workloads as wl
    from test_ssm_gpu import product_ssm
    from oracle import ssm as ossm
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    c3 = wl.ssm_c3(256)
    n, m = c3['n'], c3['m']
    assert (n, m) == (10, 8)
    model = ossm.synthetic(n, m, 3, 2, seed=95)
    # the one-wave kernel is launched only on the MFMA-1 path with N <= 512 (ilqr_impl); anywhere else SRH_ILQR_THREADS=64
    # silently runs 512 threads and the comparison below would compare the default form with itself
    assert lc.ssm_ilqr_path(n, m, n, model['Er'], model['Es'].shape[0]) == 'mfma1' and c3['N'] <= 512
    s = product_ssm(model, discr=c3['discr'])
    s.H = model['W'][:, :n].copy()
    il = iLQR(c3['dt'], s, QuadraticCost(Q=c3['Qz'], R=c3['R'], Qf=c3['Qf']), c3['N'])
    il.set_target(c3['zt'][:members])
    x, u, K = il.ilqr_computation(c3['x0'][:members])
    return x, u, K, il.cost.copy(), il.iters.copy()


def test_ilqr_ssm_one_wave_form_is_bit_identical(monkeypatch):
    """The comment above ilqr_kernel claims that the one-wave form (SRH_ILQR_THREADS=64, C3 shape n_x = 10, n_u = 8) runs
    the same per-element arithmetic in the same order as the 512-thread form: x, u, K, cost and iters bit for bit."""
    base = c3_solve()
    monkeypatch.setenv('SRH_ILQR_THREADS', '64')
    one = c3_solve()
    for name, a, b in zip(('x', 'u', 'K', 'cost', 'iters'), one, base):
        print('ilqr_ssm one-wave vs 512 threads: max |d %s| = %.3e' % (name, float(np.abs(a - b).max())))
    for a, b in zip(one, base):
        np.testing.assert_array_equal(a, b)


def g11_solve(golden, tag):
    from test_ssm_gpu import product_ssm, ILQR_SSM_CASES
    from oracle import ssm as ossm
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    g = golden('g11_ilqr_ssm')
    meth, N, useH = ILQR_SSM_CASES[tag]
    model = ossm.synthetic(6, 4, 3, 3, seed=90)
    s = product_ssm(model, discr=meth)
    if useH:
        s.H = model['W'][:, :6].copy()
    Qz = g[tag + '_Qz']
    il = iLQR(0.01, s, QuadraticCost(Q=Qz, R=0.05 * np.eye(4), Qf=5 * Qz), N)
    il.set_target(g[tag + '_z_target'])
    x, u, K = il.ilqr_computation(g[tag + '_x0'], g[tag + '_uw'])
    return g, x, u, K, int(il.iters[0])


@pytest.mark.parametrize('env', ['SRH_SSM_DENSE_JACOBIAN', 'SRH_ILQR_NO_MFMA'])
@pytest.mark.parametrize('tag', ['fe', 'h0', 'hw'])
def test_ilqr_ssm_switched_forms_meet_g11(golden, tag, env, monkeypatch):
    """The dense derivative table and the VALU backward pass are other evaluation orders of the same solve: each meets the
    golden vectors g11 at the tolerances of test_ilqr_ssm_golden with the same iteration count (no bit identity is
    claimed for them; the difference from the default form is printed)."""
    from test_ssm_gpu import close
    _, x0, u0, K0, it0 = g11_solve(golden, tag)
    monkeypatch.setenv(env, '1')
    g, x, u, K, it = g11_solve(golden, tag)
    print('ilqr_ssm g11 %s with %s=1 vs default: max |dx| %.3e |du| %.3e |dK| %.3e, iters %d / %d'
          % (tag, env, np.abs(x - x0).max(), np.abs(u - u0).max(), np.abs(K - K0).max(), it, it0))
    assert it == int(g[tag + '_iters'])
    close(x, g[tag + '_x'], 1e-9); close(u, g[tag + '_u'], 1e-8); close(K, g[tag + '_K'], 1e-7)


# ------------------------------------------------------------------------------------------------------------ TV-LQR
@pytest.mark.parametrize('n,m', lc.RICCATI_SHAPES)
def test_tvlqr_against_long_double(n, m):
    """sric_tvlqr (explicit per-step A_i, B_i) against the long-double recursion: gains and all steps + 1 slices of P,
    the terminal P = Q included; the inner dimensions of `mm` sit below, on and past its unroll by 8."""
    from sofacontrol_amd.lqr.lqr import tvlqr
    failures = []
    for steps in (1, 3, 20):
        A, B, Q, R = lc.tvlqr_case(n, m, steps)
        Kr, Pr = lr.tvlqr(A, B, Q, R)
        Ko, Po = olqr.tvlqr(A, B, Q, R)
        tol = tolerance(max(lr.err(Ko, Kr), lr.err(Po, Pr)))
        K, P = tvlqr(A, B, Q, R)
        assert K.shape == (steps, m, n) and P.shape == (steps + 1, n, n)
        np.testing.assert_array_equal(P[-1], Q)
        eK, eP = lr.err(K, Kr), lr.err(P, Pr)
        print('tvlqr (n_x %d, n_u %d) steps %d: err K %.2e P %.2e | tol %.2e' % (n, m, steps, eK, eP, tol))
        if max(eK, eP) > tol:
            failures.append((steps, eK, eP, tol))
    assert not failures, failures


def test_tvlqr_accepts_no_P_and_refuses_nx79():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.lqr.lqr import tvlqr
    A, B, Q, R = lc.tvlqr_case(7, 3, 3)
    K, P = tvlqr(A, B, Q, R)
    K2 = np.empty_like(K)
    _lib.check(_lib.lib().sric_tvlqr(_lib.dptr(A), _lib.dptr(B), C.c_int(3), C.c_int(7), C.c_int(3), _lib.dptr(Q), _lib.dptr(R),
                                     _lib.dptr(K2), None), 'sric_tvlqr')
    np.testing.assert_array_equal(K2, K)
    A, B, Q, R = lc.tvlqr_case(79, 4, 1)                     # (78, 4) runs: test_tvlqr_against_long_double
    with pytest.raises(RuntimeError, match='sric_tvlqr: state dimension too large for LDS'):
        tvlqr(A, B, Q, R)


def test_tvlqr_tpwl_nx60_against_long_double():
    """sric_tvlqr_tpwl (the `idx` path: nearest TPWL point per nominal state, gathered on the device) at n_x = 60 through
    TrajTrackingLQR, against the long-double recursion over the tables the oracle's nearest-point rule selects."""
    from sofacontrol_amd.lqr.traj_tracking_lqr import TrajTrackingLQR
    from sofacontrol_amd.utils import QuadraticCost
    r, m, N, dt = 30, 4, 12, 0.05
    model, U, q_ref, v_ref, Hf = golden_problem(r, m, 8, 40, 55, q_scale=0.2)
    tp = product_tpwl(model, U, q_ref, v_ref, Hf)
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(dt)
    Ad, Bd = np.stack(tp.A_d), np.stack(tp.B_d)
    rng = np.random.default_rng(60)
    G = rng.standard_normal((2 * r, 2 * r))
    Q, R = G @ G.T + np.eye(2 * r), 0.5 * (np.eye(m) + 0.1 * np.ones((m, m)))
    # nominal states wandering between the table points, so that the gather makes real choices
    w = rng.dirichlet(np.ones(8) * 0.3, size=N + 1)
    xs = np.hstack([w @ model['v'], w @ model['q']])

    class Target:
        t, x, u = dt * np.arange(N + 1), xs, np.zeros((N + 1, m))
    tt = TrajTrackingLQR(dt, tp, QuadraticCost(Q=Q, R=R))
    K, P = tt.perform_dlqr_recursion(Target)
    steps = len(K)
    assert steps >= N - 1 and P.shape == (steps + 1, 2 * r, 2 * r)
    idx = otpwl.nearest_points(model, np.asarray(tt.x_bar))
    assert len(set(idx.tolist())) > 2
    Kr, Pr = lr.tvlqr(Ad[idx], Bd[idx], Q, R)
    Ko, Po = olqr.tvlqr(Ad[idx], Bd[idx], Q, R)
    tol = tolerance(max(lr.err(Ko, Kr), lr.err(Po, Pr)))
    eK, eP = lr.err(K, Kr), lr.err(P, Pr)
    print('tvlqr_tpwl n_x 60 steps %d, %d regions: err K %.2e P %.2e | tol %.2e' % (steps, len(set(idx.tolist())), eK, eP, tol))
    assert eK <= tol and eP <= tol


# --------------------------------------------------------------------------------------------------- fixed-point DARE
@pytest.mark.parametrize('n,m', lc.RICCATI_SHAPES)
def test_fixed_point_dare_against_long_double(n, m):
    """solve_riccati / sric_dare_fixed_point against the long-double iteration: same iteration count (the inputs stop at
    least 1 % away from tol on both sides: tests/test_lq_reference_cpu.py), L and P; and a stack of three DIFFERENT
    (A, B) in one launch, each member bit for bit its single solve."""
    from sofacontrol_amd.lqr.lqr import solve_riccati, _fixed_point
    tol_fp = 1e-4
    As, Bs, Q, R = lc.dare_case(n, m)
    Lb, Pb, itb = _fixed_point(As, Bs, Q, R, tol_fp, 1000000)
    failures = []
    for k in range(3):
        L1, P1, it1 = _fixed_point(As[k], Bs[k], Q, R, tol_fp, 1000000)
        np.testing.assert_array_equal(Lb[k], L1[0]); np.testing.assert_array_equal(Pb[k], P1[0])
        assert int(itb[k]) == int(it1[0])
        Lr, Pr, itr, (d_prev, d_last) = lr.fixed_point_dare(As[k], Bs[k], Q, R, tol_fp)
        assert d_last <= 0.99 * tol_fp and d_prev >= 1.01 * tol_fp
        Lo, Po, ito = olqr.solve_riccati(As[k], Bs[k], Q, R, tol_fp)
        tol = tolerance(max(lr.err(Lo, Lr), lr.err(Po, Pr)))
        eL, eP = lr.err(Lb[k], Lr), lr.err(Pb[k], Pr)
        print('dare_fp (n_x %d, n_u %d) member %d: %d iterations (reference %d), err L %.2e P %.2e | tol %.2e'
              % (n, m, k, int(itb[k]), itr, eL, eP, tol))
        if int(itb[k]) != itr or max(eL, eP) > tol:
            failures.append((k, int(itb[k]), itr, eL, eP, tol))
    assert not failures, failures
    L, P = solve_riccati(As[0], Bs[0], Q, R)
    np.testing.assert_array_equal(L, Lb[0]); np.testing.assert_array_equal(P, Pb[0])


def test_fixed_point_dare_max_iter_is_not_an_error():
    from sofacontrol_amd.lqr.lqr import _fixed_point
    As, Bs, Q, R = lc.dare_case(9, 1)
    L, P, it = _fixed_point(As[0], Bs[0], Q, R, 1e-4, 3)
    Lr, Pr, itr, _ = lr.fixed_point_dare(As[0], Bs[0], Q, R, 1e-4, 3)
    Lo, Po, ito = olqr.solve_riccati(As[0], Bs[0], Q, R, 1e-4, 3)
    assert int(it[0]) == itr == ito == 3
    tol = tolerance(max(lr.err(Lo, Lr), lr.err(Po, Pr)))
    assert lr.err(L[0], Lr) <= tol and lr.err(P[0], Pr) <= tol


def test_indefinite_R_is_reported():
    """A factorisation that fails is an error on every Riccati entry point (the fixed-point iteration used to return
    whatever its work arrays held, with SRH_OK)."""
    from sofacontrol_amd.lqr.lqr import tvlqr, solve_riccati, _fixed_point
    A, B, Q, _ = lc.tvlqr_case(7, 2, 3)
    R = np.diag([1.0, -1e6])
    with pytest.raises(RuntimeError, match=r"sric_tvlqr: R \+ B'PB is not positive definite"):
        tvlqr(A, B, Q, R)
    message = r'sric_dare_fixed_point: problem 0: R \+ B\^T P B is not positive definite'
    with pytest.raises(RuntimeError, match=message):
        solve_riccati(A[0], B[0], Q, R)
    with pytest.raises(RuntimeError, match=message):
        _fixed_point(A, B, Q, R, 1e-4, 100)
    # a definite R on the same inputs goes through
    L, P = solve_riccati(A[0], B[0], Q, np.eye(2))
    assert np.isfinite(L).all() and np.isfinite(P).all()
