"""CPU: input conditions of the seeded cases of the batched closed-loop Koopman MPC (tests/koopman_loop_cases.py), and the numpy
restatement (tests/koopman_loop_reference.py) against the reference's own KoopmanMPC.evaluate traces (tests/golden/g22_koopman.npz).

The float64 restatement agrees with the long-double one within E_ORACLE_MAX; every plant sub-step of every case has a nearest-point gap
above MARGIN (no case is dropped for a near tie: the seeds are chosen so, and every case is asserted); the table of cases is covered;
the observables' order is the golden file's; and the restatement, replayed on the recorded measurements and applied inputs with the exact
QP of oracle/locp.py, reproduces the reference's requests."""
import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import koopman_loop_cases as kc
import koopman_loop_reference as kr


def test_the_rules_are_the_shared_ones():
    assert kr.err is cr.err and kr.tolerance is cr.tolerance and kr.nearest_with_margin is cr.nearest_with_margin and kr.window is cr.window
    assert kr.LD is cr.LD


def test_the_table_of_cases_is_covered():
    rows = kc.ADVANCE
    assert len({c[0] for c in rows}) == len(rows)
    kind = lambda key: key.split('-')[0]
    pairs = {(c[1], kind(c[2])) for c in rows}
    # every (plant, model kind) that exists: the shipped model has four inputs, as r36 alone has
    assert pairs == {('r36', 'ship')} | {(p, k) for p in ('g6', 'r36', 'm8') for k in ('syn2', 'w', 'dmd')}
    sim = [c for c in rows if c[8] == 'sim']
    for plant in ('g6', 'r36', 'm8'):
        mine = [c for c in sim if c[1] == plant]
        assert {c[3] for c in mine} == {1, 5}, plant                                  # r
        assert {c[4] for c in mine} == {1, 3, kc.N}, plant                            # rollout_horizon
        assert {c[6] for c in mine} == {True, False} and {c[7] for c in mine} == {True, False}, plant      # W, V
    assert {c[5] for c in rows} == {1, 3, 260}
    assert {c[8] for c in rows} == {'sim', 'replay', 'replay-u'}
    # the models: two delays, a W truncation (mandatory for m8: 14 zeta entries at degree 2 give 120 observables), dmd
    for key in kc.SPECS:
        s = kc.spec(key)
        assert s['n_lift'] <= 96 and s['m'] <= 16, key
        assert s['B'].shape == (s['n_lift'], s['m']) and s['H'].shape == (s['n_y'], s['n_lift']), key
        assert (s['W'] is None) == (s['n_lift'] == s['n_psi']), key
    assert kc.spec('w-m8')['nzeta'] == 14 and kc.spec('w-m8')['n_psi'] == 120 and kc.spec('w-m8')['n_lift'] == 24
    assert all(kc.spec(k)['delays'] == 2 for k in kc.SPECS if k.startswith('syn2'))
    assert all(kc.spec(k)['dmd'] for k in kc.SPECS if k.startswith('dmd'))
    assert kc.spec('ship')['n_lift'] == 66 and 2 * cc.MODELS['r36'][0] == 72


@pytest.mark.parametrize('key', ['10_2_0', '10_2_1', '3_3_0', '3_3_1', '4_4_0', '4_4_1'])
def test_observable_order_is_the_golden_one(key):
    nzeta, degree, dmd = (int(v) for v in key.split('_'))
    np.testing.assert_array_equal(kr.exponents(nzeta, degree, dmd), kc.golden()['order_' + key])


def test_lift_reproduces_the_golden_lift():
    g = kc.golden()
    for dmd, want in ((False, g['lift']), (True, g['lift_dmd'])):
        s = dict(kc.spec('ship'), dmd=dmd)
        for row, zeta in enumerate(g['zeta_offline_1']):
            # zeta = [y_t, y_{t-1}, u_{t-1}]: histories of two samples that give it back
            hy, hu = [zeta[3:6], zeta[0:3]], [zeta[6:10], np.zeros(4)]
            got = kr.lift(s, hy, hu, np.float64)
            assert kr.err(got, want[row]) <= 1e-13, (dmd, row)


@pytest.mark.parametrize('case', kc.ADVANCE, ids=lambda c: c[0])
def test_advance_cases_are_well_conditioned(case):
    name, mname, key, r, rh, B, dist, noise, mode, seed = case
    c = kc.advance_case(case)
    e, ref, f64 = kc.e_oracle(case)
    print('%s: e_oracle %.3e, nearest-point margin %.3e' % (name, e, ref['margin']))
    assert e <= cr.E_ORACLE_MAX
    assert c['n_keep'] == rh * r and abs(kc.TS - r * c['dt_sim']) <= 1e-15
    if mode == 'sim':
        assert ref['margin'] > cr.MARGIN and f64['margin'] > cr.MARGIN
        np.testing.assert_array_equal(ref['picks'], f64['picks'])
        assert (ref['picks'] >= 0).all()
        if rh * r >= 15 and B <= 3:
            assert len(np.unique(ref['picks'])) >= 2, 'a long case should change region'
        assert np.isfinite(np.asarray(ref['X'], dtype=np.float64)).all()
    else:
        assert ref['X'] is None and (ref['picks'] == -1).all()
        np.testing.assert_array_equal(f64['Y'], c['Y_plant'][:, 1:])
    # the input of a sub-step is the plan row of the controller step that has fired
    s = c['spec']
    for k in range(c['n_keep']):
        np.testing.assert_array_equal(f64['U'][:, k], c['uopt'][:, k // r] * s['u_factor'] + s['u_offset'])
    if c['U_applied'] is not None:
        np.testing.assert_array_equal(f64['ring'][:, :, s['n_y']:], (c['U_applied'] - s['u_offset']) / s['u_factor'])


def test_fixup_statement():
    c = kc.fixup_case(4, 6, 3, 1)
    u0s = (c['u0'] - 1.0) / 2.0
    for first in (True, False):
        for b in range(4):
            xo, uo = kr.fixup(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, u0s, np.float64)
            if c['status'][b] == 0:
                np.testing.assert_array_equal(xo, c['xsol'][b]); np.testing.assert_array_equal(uo, c['usol'][b])
            elif first:
                assert (xo == c['x0'][b]).all() and (uo == u0s).all()
            else:
                np.testing.assert_array_equal(xo[:-1], c['xprev'][b, 1:]); np.testing.assert_array_equal(xo[-1], c['xprev'][b, -1])
                np.testing.assert_array_equal(uo[:-1], c['uprev'][b, 1:]); np.testing.assert_array_equal(uo[-1], c['uprev'][b, -1])


def exact_solver(g, s, N):
    """solve(p, t_p, x0) on the exact QP of oracle/locp.py with the driver's cost, box and target (tests/test_koopman_gpu.py)."""
    from oracle import locp as olocp

    def solve(p, t_p, x0):
        z = kr.window(g['cost_t'], g['cost_z'], round(t_p, 4), kc.TS, N + 1, np.float64)
        qp = olocp.build_qp(N, s['H'], g['cost_Q'], g['cost_R'], [s['A']] * N, [s['B']] * N, [np.zeros(s['n_lift'])] * N, np.asarray(x0), None,
                            0.0, 0.0, z=z, u_des=np.tile(g['cost_u'], (N, 1)), U=(g['cost_UA'], g['cost_Ub']), tr_active=False)
        w, _, _ = olocp.solve_exact(qp)
        x, u, _ = olocp.split(qp, w)
        return x, u, 0
    return solve


@pytest.mark.parametrize('rh,periods', [(1, 11), (3, 3)])
def test_replay_reproduces_the_reference_trace(rh, periods):
    """Y_plant = trace_y[200:], U_applied = tr_<rh>_0_u, history from rows 199 / 198: the requests of the reference's own evaluate.  The
    reference rounds its request times to four decimals (koopman.py:76); the restatement's t_p are compared after the same rounding
    (exactly) and as they are (1e-9)."""
    g = kc.golden()
    s = kc.spec('ship')
    tag = 'tr_%d_0_' % rh
    r, N = 5, int(g['mpc_N'])
    S = periods * rh * r
    y, u = g['trace_y'], g[tag + 'u']
    u0s = kr.scale_down(np.full(4, 300.0), s['u_offset'], s['u_factor'], np.float64)
    out = kr.replay(s, y[199:200], u[198:199], y[200], u[199], y[200:200 + S + 1], u[200:200 + S], r, rh, periods, 0.0, 0.01,
                    exact_solver(g, s, N), u0s)
    req_t, req_x = g[tag + 'req_t'], g[tag + 'req_x0']
    assert len(req_t) >= periods
    np.testing.assert_array_equal(np.round(out['t'][:periods], 4), req_t[:periods])
    np.testing.assert_allclose(out['t'][:periods], req_t[:periods], rtol=0, atol=1e-9)
    e = np.abs(out['x_lift'] - req_x[:periods]).max() / np.abs(req_x[:periods]).max()
    e_u = np.abs(out['u'] - u[200:200 + S]).max() / np.abs(u).max()
    print('rh %d: %d periods, requests %.3e relative, inputs of the exact QP %.3e of max|u|' % (rh, periods, e, e_u))
    assert e <= 1e-12
    assert e_u <= 1e-6
    np.testing.assert_array_equal(out['y'], y[200:200 + S + 1])
