"""CPU: keeps the long-double reference of tests/lq_reference.py honest, and enforces the input conditions under which
tests/test_lqr_exact_gpu.py may hold the kernels of csrc/lqr.hip to a tolerance near round-off: on every test problem the
float64 oracle must agree with the long-double solution to 1e-11, and the fixed-point DARE iteration must stop at a safe
distance from its threshold."""
import numpy as np
import pytest

import lq_cases as lc
import lq_reference as lr
from oracle import lqr as olqr, tpwl as otpwl

E_ORACLE_MAX = 1e-11


def test_chol_solve_against_float64():
    rng = np.random.default_rng(0)
    for m in (1, 2, 5, 16):
        G = rng.standard_normal((m, m))
        S = G @ G.T + m * np.eye(m)
        B = rng.standard_normal((m, 3))
        X = lr.chol_solve(S, B)
        assert X.dtype == np.longdouble
        assert lr.err(np.linalg.solve(S, B), X) <= 1e-13
        assert float(np.abs(lr.ld(S) @ X - B).max()) <= 1e-16 * m * float(np.abs(S).max())      # residual at 80-bit level
        assert lr.chol_solve(S, B[:, 0]).shape == (m,)
    with pytest.raises(np.linalg.LinAlgError):
        lr.chol_solve(np.diag([1.0, -1.0]), np.ones(2))


@pytest.mark.parametrize('n,m,nz,N', [(1, 1, 1, 1), (2, 1, 1, 4), (4, 2, 3, 3), (6, 3, 6, 4)])
def test_lq_tracking_against_dense_kkt(n, m, nz, N):
    """The Riccati solution is the minimiser: the same problem as one dense float64 KKT system."""
    rng = np.random.default_rng(10 * n + m)
    A = 0.98 * lc.orthogonal(n, rng)
    B = rng.standard_normal((n, m))
    d = 0.1 * rng.standard_normal(n)
    H = rng.standard_normal((nz, n))
    z_ref = rng.standard_normal(nz)
    Q, R, Qf = lc.costs(m, nz, rng)
    zt = z_ref + 0.05 * rng.standard_normal((N + 1, nz))
    x0 = rng.standard_normal(n)
    x, u, K, cost = lr.lq_tracking(A, B, d, H, z_ref, Q, R, Qf, zt, x0, N)
    xk, uk = lr.kkt_tracking(A, B, d, H, z_ref, Q, R, Qf, zt, x0, N)
    assert lr.err(xk, x) <= 1e-12 and lr.err(uk, u) <= 1e-12, (lr.err(xk, x), lr.err(uk, u))
    # u_t = K_t x_t + k_t: moving x0 moves u_0 by K_0 dx
    x2, u2, _, _ = lr.lq_tracking(A, B, d, H, z_ref, Q, R, Qf, zt, x0 + 1.0, N)
    assert float(np.abs(u2[0] - u[0] - K[0] @ np.ones(n)).max()) <= 1e-16 * max(1.0, float(np.abs(K[0]).max())) * n


@pytest.mark.parametrize('shape', lc.ILQR_SHAPES + lc.VALU_SHAPES[-1:], ids=str)
def test_oracle_newton_step_is_the_exact_minimiser(shape):
    """One iteration of oracle.lqr.ILQRGeneric (max_iter = 0, switches off) lands on lq_tracking's optimum from a cold
    and from a random warm start, on every shape of the GPU test, to 1e-11: the input condition of that test."""
    c = lc.ilqr_case(*shape)
    Ad, Bd, dd = otpwl.pre_discretize(c['model'], lc.DT, 'zoh')
    A, B, d = Ad[0], Bd[0], dd[0]
    xr, ur, Kr, cr = lr.lq_tracking(A, B, d, c['H'], c['z_ref'], c['Q'], c['R'], c['Qf'], c['z_target'], c['x0'], c['N'])
    # the nearest-point search makes real choices along the optimum (the tables carry different q)
    picks = {otpwl.nearest_point(c['model'], np.asarray(xi, dtype=np.float64)) for xi in xr[:c['N']]}
    assert len(picks) > 1 or c['N'] == 1
    for uw in (None, c['u_warm']):
        x, u, K, cost = lc.oracle_newton_step(A, B, d, c['H'], c['z_ref'], c, uw)
        e = max(lr.err(x, xr), lr.err(u, ur), lr.err(K, Kr), lr.err(cost, cr))
        print('%s %s e_oracle %.2e' % (shape, 'cold' if uw is None else 'warm', e))
        assert e <= E_ORACLE_MAX, (shape, e)


def test_ilqr_paths_and_refusal_sizes():
    """The shapes reach the paths their comments claim (dispatch restated from the LDS formulas of ilqr_impl)."""
    path = {s: lc.ilqr_path(2 * s[0], s[1]) for s in lc.ILQR_SHAPES}
    assert path[(5, 4, 6, 10)] == path[(30, 4, 6, 15)] == path[(24, 16, 16, 5)] == path[(31, 2, 6, 5)] == 'mfma1'
    assert path[(30, 8, 6, 15)] == path[(31, 9, 6, 5)] == path[(36, 4, 6, 15)] == path[(36, 7, 6, 3)] == 'mfma2'
    assert path[(32, 16, 16, 5)] == 'valu_unstaged'
    assert lc.ilqr_path(64, 2) == 'mfma2' and lc.ilqr_path(50, 16) == 'mfma2'          # successors of the largest MFMA-1 shapes
    assert lc.ilqr_path(62, 16) == 'valu_unstaged' and lc.ilqr_path(72, 7) == 'mfma2' and lc.ilqr_path(72, 8) == 'refused'
    assert [lc.ilqr_path(2 * r, m, True) for r, m, _, _ in lc.VALU_SHAPES] == ['valu_staged'] * 3 + ['valu_unstaged']
    assert lc.ilqr_path(64, 4, True) == 'valu_staged' and lc.ilqr_path(66, 4, True) == 'valu_unstaged'
    assert lc.ilqr_path(76, 4, True) == 'refused' and lc.ilqr_path(76, 4) == 'mfma2' and lc.ilqr_path(78, 4) == 'refused'
    assert lc.ilqr_path(72, 16) == 'refused'
    assert lc.lqr_lds_doubles(78, 4) * 8 <= lc.LDS_LIMIT < lc.lqr_lds_doubles(79, 4) * 8
    # the C3 SSM shape sits on MFMA-1 with either derivative table: the only place the one-wave kernel is launched
    from oracle import ssm as ossm
    c3 = ossm.synthetic(10, 8, 3, 2, seed=95)
    assert lc.ssm_ilqr_path(10, 8, 10, c3['Er'], c3['Es'].shape[0]) == 'mfma1'
    assert lc.ssm_ilqr_path(10, 8, 10, c3['Er'], c3['Es'].shape[0], no_mfma=True) == 'valu_staged'


@pytest.mark.parametrize('n,m', lc.RICCATI_SHAPES)
def test_tvlqr_oracle_against_long_double(n, m):
    for steps in (1, 3, 20):
        A, B, Q, R = lc.tvlqr_case(n, m, steps)
        K, P = olqr.tvlqr(A, B, Q, R)
        Kr, Pr = lr.tvlqr(A, B, Q, R)
        assert Kr.shape == (steps, m, n) and Pr.shape == (steps + 1, n, n)
        np.testing.assert_array_equal(np.asarray(Pr[-1], dtype=np.float64), Q)
        e = max(lr.err(K, Kr), lr.err(P, Pr))
        print('tvlqr (%d, %d) steps %d e_oracle %.2e' % (n, m, steps, e))
        assert e <= E_ORACLE_MAX, (n, m, steps, e)


@pytest.mark.parametrize('n,m', lc.RICCATI_SHAPES)
def test_fixed_point_dare_oracle_and_stopping_margin(n, m):
    """oracle.solve_riccati against the long-double iteration: same count, L and P to 1e-11; and the reference's last two
    ||L - L_old||_F are each at least 1 % away from tol, so that no float64 evaluation order can flip the count."""
    tol = 1e-4
    As, Bs, Q, R = lc.dare_case(n, m)
    for k in range(3):                                         # the single solve (member 0) and the members of the batched test
        A, B = As[k], Bs[k]
        Lr, Pr, itr, (d_prev, d_last) = lr.fixed_point_dare(A, B, Q, R, tol)
        assert itr >= 2 and d_last <= tol < d_prev
        assert d_last <= 0.99 * tol and d_prev >= 1.01 * tol, (n, m, k, d_prev, d_last)
        L, P, it = olqr.solve_riccati(A, B, Q, R, tol)
        e = max(lr.err(L, Lr), lr.err(P, Pr))
        print('dare (%d, %d) member %d: %d iterations, steps %.3e %.3e, e_oracle %.2e' % (n, m, k, itr, d_prev, d_last, e))
        assert it == itr and e <= E_ORACLE_MAX, (n, m, k, it, itr, e)
