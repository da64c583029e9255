"""CPU: the input conditions under which tests/test_gusto_loop_observer_gpu.py may hold the observed loop to a tolerance near round-off,
on the reference statement alone (tests/clobs_reference.py on tests/clobs_cases.py):
  - every one of the three lookups of every sub-step (plant at x, gain at x_bar, filter at x_hat) keeps a relative margin >=
    ekf_cases.MARGIN, and the float64 statement picks the points the long-double one picks;
  - e_oracle, the float64 statement against long double over all sub-steps and fields, is <= ekf_cases.E_ORACLE_MAX;
  - the statement composes what it claims to: with x_hat = x its first sub-step is cl_reference.advance's, and its filter step is
    ekf_reference's predict + update at the point nearest to x_hat;
  - the exact-model case has a vanishing innovation: x_hat stays on x."""
import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import clobs_cases as oc
import clobs_reference as cor
import ekf_cases as ec
import ekf_reference as er


def test_the_cases_cover_what_they_claim():
    names = {c[1] for c in oc.CASES}
    assert {2 * cc.MODELS[m][0] for m in names} == {8, 60, 72}
    assert {c[4] for c in oc.CASES} == {1, 3} and {c[3] for c in oc.CASES} == {0.05, 0.03}
    for flag in (2, 5, 6, 7):            # filter model, gains, disturbance, noise: both ways
        assert {c[flag] for c in oc.CASES} == {True, False}
    from sofacontrol_amd import _lib
    assert [_lib.ekf_plan(2 * cc.MODELS[m][0], oc.N_Y[m])['kernel'] for m in ('g6', 'r30', 'r36')] == ['valu', 'mfma_60', 'wide']
    assert cr.MARGIN == ec.MARGIN and cr.E_ORACLE_MAX == ec.E_ORACLE_MAX and cr.tolerance(3e-15) == ec.tolerance(3e-15)


@pytest.mark.parametrize('cs', oc.CASES, ids=oc.IDS)
def test_margins_and_oracle_error(cs):
    ref, e_oracle = oc.measured(cs)
    print('%s: e_oracle %.3e, least margin %.3e, plant points %s, filter points %s' %
          (cs[0], e_oracle, ref['margin'], sorted(set(ref['idx_plant'].ravel())), sorted(set(ref['idx_filter'].ravel()))))
    assert ref['margin'] >= ec.MARGIN, (cs[0], ref['margin'])
    assert e_oracle <= ec.E_ORACLE_MAX, (cs[0], e_oracle)
    assert ref['Xhat'].shape == (oc.B, cs[4], 2 * cc.MODELS[cs[1]][0]) and ref['Y'].shape == (oc.B, cs[4], oc.N_Y[cs[1]])
    assert (ref['idx_gain'] >= 0).all() == bool(cs[5])


@pytest.mark.parametrize('cs', [oc.CASES[1], oc.CASES[3]], ids=[oc.IDS[1], oc.IDS[3]])
def test_composition_of_the_two_references(cs):
    name, mname, same, dt_sim, n_keep, gains, dist, noise, seed = cs
    c, ms = oc.case(cs), oc.measurement(mname)
    planner, plant, filt = cc.table_dict(mname), cc.table_dict(mname, dt_sim), oc.filter_tables(mname, same, dt_sim)
    H = cc.model(mname)['H']
    b = 1
    Wn = None if c['W'] is None else c['W'][:, b]
    Vn = None if c['V'] is None else c['V'][:, b]
    # x_hat = x: the law, the plant step and z of the first sub-step are cl_reference.advance's, bit for bit in long double
    o = cor.observed_advance(planner, plant, filt, H, ms['C'], ms['y_ref'], ms['W'], ms['V'], c['K'], c['xopt'][b], c['uopt'][b], c['x'][b],
                             c['x'][b], ms['Sigma0'], c['j'][:1], c['theta'][:1], None if Wn is None else Wn[:1], None if Vn is None else Vn[:1],
                             cr.LD)
    X, U, Z, ip, ig, _ = cr.advance(planner, plant, H, c['K'], c['xopt'][b], c['uopt'][b], c['x'][b], c['j'][:1], c['theta'][:1],
                                    None if Wn is None else Wn[:1], cr.LD)
    for got, want in ((o['X'], X), (o['U'], U), (o['Z'], Z), (o['idx_plant'], ip), (o['idx_gain'], ig)):
        np.testing.assert_array_equal(got, want)
    # the filter step is ekf_reference's at the point nearest to the estimate
    f, _ = er.nearest_with_margin(filt['q'], filt['v'], filt['w_q'], filt['w_v'], c['x'][b])
    assert f == o['idx_filter'][0]
    xp, Sp = er.predict(filt['A_d'][f], filt['B_d'][f], filt['d_d'][f], c['x'][b], ms['Sigma0'], o['U'][0], ms['W'])
    xn, Sn = er.update(ms['C'], ms['y_ref'], xp, Sp, o['Y'][0], ms['V'])
    np.testing.assert_array_equal(o['Xhat'][0], xn)
    np.testing.assert_array_equal(o['Sigma'], Sn)
    y = er.ld(ms['C']) @ o['X'][0] + er.ld(ms['y_ref']) + (0 if Vn is None else er.ld(Vn[0]))
    np.testing.assert_array_equal(o['Y'][0], y)


def test_exact_model_keeps_the_estimate_on_the_state():
    cs = [c for c in oc.CASES if c[0].endswith('exact')][0]
    assert cs[2] and not cs[6] and not cs[7]
    ref, e_oracle = oc.measured(cs)
    e = cor.err(ref['Xhat'], ref['X'])
    print('%s: x_hat against x in long double %.3e' % (cs[0], e))
    assert e <= 1e-16
