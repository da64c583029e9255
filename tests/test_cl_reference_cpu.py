"""CPU: the input conditions of the closed-loop cases (tests/cl_cases.py) and the float64 statement of the reference
(tests/cl_reference.py) against the code it restates.  For every advance case: e_oracle -- the worst error of the float64 statement
against the long-double one, max|a - b| / max(1, max|b|) -- is at most 1e-11, every nearest-point lookup has a relative margin of at
least 1e-6 (so rounding cannot flip a region: the float64 picks equal the long-double ones), and over the case set the plant and the
gain lookup both change region inside a period.  The float64 shift is GuSTOSolverNode._warm_start bit for bit; the float64 target
window is scipy's interp1d as scp/standalone.py:29 configures it."""
import types

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr


@pytest.fixture(scope='module')
def advance_refs():
    return {c[0]: (cc.advance_reference(c, cr.LD), cc.advance_reference(c, np.float64)) for c in cc.ADVANCE}


@pytest.mark.parametrize('case', cc.ADVANCE, ids=[c[0] for c in cc.ADVANCE])
def test_advance_case_conditions(advance_refs, case):
    ref, f64 = advance_refs[case[0]]
    e_oracle = max(cr.err(f64[i], ref[i]) for i in range(3))
    print('%s: e_oracle %.3e, least margin %.3e, tolerance %.3e' % (case[0], e_oracle, ref[5], cr.tolerance(e_oracle)))
    assert e_oracle <= cr.E_ORACLE_MAX
    assert ref[5] >= cr.MARGIN and f64[5] >= cr.MARGIN
    np.testing.assert_array_equal(f64[3], ref[3])
    np.testing.assert_array_equal(f64[4], ref[4])
    assert np.isfinite(np.asarray(ref[0], dtype=np.float64)).all()


def test_case_set_switches_regions_and_members_differ(advance_refs):
    plant = sum(int((np.diff(r[0][3], axis=1) != 0).sum()) for r in advance_refs.values())
    gain = sum(int((np.diff(r[0][4], axis=1) != 0).sum()) for n, r in advance_refs.items() if r[0][4].min() >= 0)
    print('region switches inside a period over the case set: plant %d, gain lookup %d' % (plant, gain))
    assert plant >= 1 and gain >= 1
    for case in cc.ADVANCE:
        c = cc.advance_case(case)
        for b in range(1, min(case[2], 3)):
            assert not np.array_equal(c['xopt'][0], c['xopt'][b]) and not np.array_equal(c['x'][0], c['x'][b])
    # the largest n_keep samples the held last input interval, the fractional ratio varies theta
    assert cc.advance_case(cc.ADVANCE[1])['j'][-1] == cc.N - 1 and cc.advance_case(cc.ADVANCE[3])['j'][-1] == cc.N - 1
    assert len(np.unique(cc.advance_case(cc.ADVANCE[4])['theta'])) > 3


@pytest.mark.parametrize('dt_sim,n_keep', [(0.05, 1), (0.05, 12), (0.01, 10), (0.03, 1), (0.03, 7), (0.03, 10), (0.03, 20)])
def test_shift_is_warm_start(dt_sim, n_keep):
    from sofacontrol_amd.scp.standalone import GuSTOSolverNode
    rng = np.random.default_rng(4)
    N = cc.N
    seen = set()
    for k in range(1, 30):
        xopt, uopt = rng.standard_normal((N + 1, 8)), rng.standard_normal((N, 3))
        _, idx0, _, _ = cc.direct_schedule(N, cc.DT, dt_sim, n_keep, 0.1, k)
        seen.add(idx0)
        # (the host's idx0: a stand-in whose times are the row numbers finds exactly that row)
        node = types.SimpleNamespace(topt=np.arange(N + 1.0), xopt=xopt, uopt=uopt, N=N)
        u_ws, x_ws = GuSTOSolverNode._warm_start(node, float(idx0))
        u_sh, x_sh = cr.shift(xopt, uopt, idx0)
        np.testing.assert_array_equal(u_sh, u_ws)
        np.testing.assert_array_equal(x_sh, x_ws)
        if idx0 < N:          # the reference's own search on the period's times, where it finds a row
            t_prev = (0.1 + (k - 1) * (n_keep * dt_sim)) + cc.DT * np.arange(N + 1)
            node.topt = t_prev
            u_ws, x_ws = GuSTOSolverNode._warm_start(node, 0.1 + k * (n_keep * dt_sim))
            np.testing.assert_array_equal(u_sh, u_ws)
            np.testing.assert_array_equal(x_sh, x_ws)
    print('dt_sim %g, n_keep %d: idx0 values %s' % (dt_sim, n_keep, sorted(seen)))
    if (dt_sim, n_keep) == (0.03, 7):
        assert seen == {5}          # 0.21 lies between rows 4 and 5 of the previous plan: idx0 lands mid-grid


def test_window_is_interp1d():
    from scipy.interpolate import interp1d
    g = cc.g6()
    t, z = g['t'], g['zt']
    zi = interp1d(t, z, axis=0, bounds_error=False, fill_value=(z[0, :], z[-1, :]))
    worst, clamped = 0.0, [0, 0]
    for t0 in (-0.2, 0.0, 0.37, 1.3 + 0.03 * 7, float(t[-1]) - 0.8 + 0.9, float(t[5]), 3.5):
        tq = t0 + cc.DT * np.arange(cc.N + 1)
        clamped[0] += int((tq < t[0]).sum()); clamped[1] += int((tq > t[-1]).sum())
        ref, f64 = cr.window(t, z, t0, cc.DT, cc.N + 1, cr.LD), cr.window(t, z, t0, cc.DT, cc.N + 1, np.float64)
        e_oracle = cr.err(f64, ref)
        e_scipy = cr.err(f64, zi(tq))
        print('t0 %.4f: e_oracle %.3e, float64 window against interp1d %.3e, tolerance %.3e' % (t0, e_oracle, e_scipy, cr.tolerance(e_oracle)))
        assert e_oracle <= cr.E_ORACLE_MAX
        assert e_scipy <= cr.tolerance(e_oracle)
        worst = max(worst, e_scipy)
    assert clamped[0] > 0 and clamped[1] > 0


def test_loop_members_differ_and_reach_both_ends_of_the_target_table():
    g = cc.g6()
    a, big, one = cc.loop_inputs(3, 10), cc.loop_inputs(260, 10), cc.loop_inputs(1, 10)
    for f in ('x0', 'phase'):
        np.testing.assert_array_equal(big[f][:3], a[f]); np.testing.assert_array_equal(one[f], a[f][:1])
        assert len({a[f][b].tobytes() for b in range(3)}) == 3
    np.testing.assert_array_equal(big['W'][:, :, :3], a['W'])
    t0 = 0.1 + a['phase']
    assert t0[0] < g['t'][0] < t0[0] + cc.DT * cc.N and t0[2] < g['t'][-1] < t0[2] + cc.DT * cc.N
