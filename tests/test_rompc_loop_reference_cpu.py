"""CPU: the input conditions of tests/rompc_loop_cases.py that tests/test_rompc_loop_gpu.py relies on -- the float64 statement of every
advance case is within E_ORACLE_MAX of the long-double reference, every nearest-point pick has a margin of at least MARGIN in both
precisions, the seeded observer systems are stable -- and the chain statement of tests/rompc_loop_reference.py against a direct
scipy.interpolate.interp1d stitching of two plans (rompc.py:109-141 restated here)."""
import numpy as np
import pytest

import cl_reference as cr
import rompc_loop_cases as rc
import rompc_loop_reference as rr


@pytest.mark.parametrize('case', rc.ADVANCE, ids=[c[0] for c in rc.ADVANCE])
def test_advance_cases_meet_the_input_conditions(case):
    name, mname, B, ny, dt_sim, nk, dist, noise, with_H, mode, seed = case
    c = rc.advance_case(case)
    rho_obs, rho_ctl = rc.spectral_radii(c['ctrl'])
    e, ref, f64 = rc.e_oracle(case)
    print('%s: rho(A - L C) %.4f, rho(A + B K) %.4f, e_oracle %.3e, least margin %.3e / %.3e, plant points %s'
          % (name, rho_obs, rho_ctl, e, ref['margin'], f64['margin'], sorted(set(ref['picks'].ravel().tolist()))))
    assert rho_obs < 1.0 and rho_ctl < 1.0
    assert e <= cr.E_ORACLE_MAX
    assert ref['margin'] >= cr.MARGIN and f64['margin'] >= cr.MARGIN
    np.testing.assert_array_equal(ref['picks'], f64['picks'])
    assert c['ctrl']['C'].shape[0] == ny and ref['Y'].shape == (B, nk, ny) and ref['Xbar'].shape == ref['X'].shape
    if mode == 'replay':
        np.testing.assert_array_equal(ref['X'], c['X_plant'][:, 1:].astype(cr.LD))
    if mode == 'sim' and nk >= 10 and B <= 3:
        assert len(set(ref['picks'].ravel().tolist())) >= 2         # the panel is reloaded on the way
    # the law reads the estimate before the update, the measurement is that of the state before the step
    b, ct = 0, c['ctrl']
    y0 = ct['C'] @ c['x'][b] + ct['y_ref'] + (0 if c['V'] is None else c['V'][0, b])
    assert cr.err(f64['Y'][b, 0], y0) <= 1e-14
    u0 = f64['Ubar'][b, 0] + ct['K'] @ (c['x_hat'][b] - f64['Xbar'][b, 0])
    assert cr.err(f64['U'][b, 0], u0) <= 1e-14
    xh1 = ct['A'] @ c['x_hat'][b] + ct['B'] @ u0 + ct['d'] + ct['L'] @ ((y0 - ct['y_ref']) - ct['C'] @ c['x_hat'][b])        # observer.py:39, unfolded
    assert cr.err(f64['XH'][b, 0], xh1) <= 1e-12


def test_the_ranges_are_covered():
    A = rc.ADVANCE
    assert {c[3] for c in A} == {3, 30, 64}
    assert {(c[4], c[5]) for c in A} >= {(0.05, 1), (0.05, rc.N), (0.01, 10), (0.01, 5 * rc.N), (0.03, 10)}
    assert {c[2] for c in A} == {1, 3, 260}
    assert {c[6] for c in A} == {c[7] for c in A} == {c[8] for c in A} == {True, False}
    assert {c[9] for c in A} == {'sim', 'replay', 'one'}
    assert {c[1] for c in A} == {'g6', 'r36', 'm8'}
    j, th = rr.end_point(rc.N, rc.DT, 0.05, rc.N)
    assert j == rc.N - 1 and abs(th - 1.0) <= 4e-15                                    # theta == 1 (to rounding) at the largest n_replan
    assert rr.end_point(rc.N, rc.DT, 0.05, 1) == (1, 0.0)
    j, th = rr.end_point(rc.N, rc.DT, 0.03, 10)
    assert j == 5 and 0.0 < th < 1.0


@pytest.mark.parametrize('dt_sim,nk', [(0.05, 1), (0.05, rc.N), (0.01, 10), (0.01, 5 * rc.N), (0.03, 10)])
def test_chain_equals_the_stitched_tape(dt_sim, nk):
    """Two plans stitched as rompc.py:109-141 does (interp1d over the plans' own times, the tape sampled every dt_sim), against the
    statement: the second request starts where the tape ends, the tape's rows are the x_bar / u_bar of the sub-steps, and the row the
    reference keeps from the old plan where the new one starts is the row-0 overwrite."""
    from scipy.interpolate import interp1d
    N, dt = rc.N, rc.DT
    n, m = 8, 3
    c = rc.chain_case(4, N, n, m, 17)
    j_end, th_end = rr.end_point(N, dt, dt_sim, nk)
    import cl_cases as cc
    _, _, j, theta = cc.direct_schedule(N, dt, dt_sim, nk, 0.0, 0)
    grid = dt_sim * np.arange(nk + 1)
    worst = 0.0
    for b in range(4):
        # period 0: the plan of the first request (from the estimate x0)
        x_p, u_p = c['xprev'][b].copy(), c['uprev'][b]
        x_p[0] = c['x0'][b]                                     # the QP's x_0 = x0 constraint
        t_p = dt * np.arange(N + 1)
        u_of_t, x_of_t = interp1d(t_p, np.vstack((u_p, u_p[-1])), axis=0), interp1d(t_p, x_p, axis=0)
        t_opt, u_opt, x_opt = grid, u_of_t(np.minimum(grid, t_p[-1])), x_of_t(np.minimum(grid, t_p[-1]))
        for dtype in (cr.LD, np.float64):
            xo, uo, x_next = rr.chain(c['xprev'][b], c['uprev'][b], c['x0'][b], 0, None, None, True, j_end, th_end, dtype)
            e_req = cr.err(x_next, x_opt[-1])
            tape_x = np.stack([rr.request_state(xo, int(j[s]), theta[s], dtype) for s in range(nk)])
            ue = np.vstack((uo, uo[-1:]))
            tape_u = np.stack([ue[int(j[s])] + dtype(theta[s]) * (ue[int(j[s]) + 1] - ue[int(j[s])]) for s in range(nk)])
            e_tape = max(cr.err(tape_x, x_opt[:-1]), cr.err(tape_u, u_opt[:-1]))
            worst = max(worst, e_req, e_tape)
            assert e_req <= cr.tolerance(0.0) and e_tape <= cr.tolerance(0.0), (b, dtype, e_req, e_tape)
        # period 1: the second request starts at the tape's end; its plan has that state in row 0 (the QP's constraint), the tape keeps
        # the old plan's last row there
        x_q, u_q = c['xsol'][b].copy(), c['usol'][b]
        xo1, uo1, x_next1 = rr.chain(x_q, u_q, x_opt[-1], 0, xo, uo, False, j_end, th_end, np.float64)
        np.testing.assert_array_equal(xo1[0], x_opt[-1])
        np.testing.assert_array_equal(xo1[1:], x_q[1:]); np.testing.assert_array_equal(uo1, u_q)
        x_q[0] = x_opt[-1]
        t_q = t_opt[-1] + dt * np.arange(N + 1)
        g1 = np.minimum(t_opt[-1] + grid, t_q[-1])
        x_new = interp1d(t_q, x_q, axis=0)(g1)
        tape = np.concatenate((x_opt, x_new[1:]))
        assert cr.err(x_next1, tape[-1]) <= cr.tolerance(0.0)
        np.testing.assert_array_equal(tape[nk], x_opt[-1])
        # a failed second solve: the previous plan moved up one row, its last row held, row 0 the request
        xf, uf, _ = rr.chain(x_q, u_q, x_opt[-1], 5, xo, uo, False, j_end, th_end, np.float64)
        np.testing.assert_array_equal(xf[1:-1], xo[2:]); np.testing.assert_array_equal(xf[-1], xo[-1]); np.testing.assert_array_equal(xf[0], x_opt[-1])
        np.testing.assert_array_equal(uf[:-1], uo[1:]); np.testing.assert_array_equal(uf[-1], uo[-1])
        # a failed first solve: the request in every row, zero inputs
        x00, u00, xn0 = rr.chain(x_q, u_q, c['x0'][b], 5, None, None, True, j_end, th_end, np.float64)
        assert (x00 == c['x0'][b]).all() and not u00.any()
        np.testing.assert_array_equal(xn0, c['x0'][b])
    print('chain (%g, %d): worst distance from the interp1d tape %.3e' % (dt_sim, nk, worst))
