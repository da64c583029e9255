"""CPU: the reference of the TPWL horizon error stands on its own -- a float64 numpy restatement of TPWL's formulas lies inside every
bound of tpwl_horizon_reference on every case, every case's least search margin is at least 1e-6 (the figure the fit tests use), so no
decision of a chain is a matter of rounding, and the windows formula equals a brute-force enumeration."""
import numpy as np
import pytest

import tpwl_horizon_cases as hc
import tpwl_horizon_reference as hr

MARGIN = 1e-6


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_float64_restatement_lies_inside_every_bound(name):
    c = hc.case(name)
    mdl, H = c['model'], c['H']
    tabs = hr.fe_tables(mdl, mdl['Ts'])
    ld = hr.predict(tabs, mdl['q'], mdl['v'], mdl['w'], c['X'], c['U'], H, c['stride'], c['every'], hr.LD)
    f8 = hr.predict(tabs, mdl['q'], mdl['v'], mdl['w'], c['X'], c['U'], H, c['stride'], c['every'], np.float64)
    assert ld['margin'] >= MARGIN and f8['margin'] >= MARGIN, (name, ld['margin'], f8['margin'])
    np.testing.assert_array_equal(ld['regions'], f8['regions'])
    assert (ld['status'] == 0).all() and (f8['status'] == 0).all()
    if name in ('n12', 'n12v', 'p65'):
        assert ld['switches'] > 0, name                           # windows cross regions
    n_x, n_z, W = 2 * mdl['r'], mdl['n_z'], ld['windows'].shape[0]
    # the restatement's own sums (numpy's pairwise order: the bounds hold for any order) against the long-double evaluation of ITS predictions
    cv = hr.curves(f8['x_pred'], f8['Xw'], c['Hm'], f8['status'])
    e = f8['x_pred'] - f8['Xw']
    ez = e @ c['Hm'].T
    sq_x, sq_z = (e * e).sum(axis=2), (ez * ez).sum(axis=2)
    assert (np.abs(sq_x.sum(axis=0) - cv['sse_x']) <= hr.sse_x_bound(cv, n_x)).all()
    assert (np.abs(sq_z.sum(axis=0) - cv['sse_z']) <= hr.sse_z_bound(cv, n_x, n_z)).all()
    assert (np.abs(sq_x - cv['sq_x']) <= hr.sq_x_bound(cv, n_x)).all() and (np.abs(sq_z - cv['sq_z']) <= hr.sq_z_bound(cv, n_x, n_z)).all()
    assert hr.norm_sq_check(np.sqrt(sq_x), cv['sq_x'], hr.sq_x_bound(cv, n_x)).all()
    assert hr.norm_sq_check(np.sqrt(sq_z), cv['sq_z'], hr.sq_z_bound(cv, n_x, n_z)).all()
    assert (cv['sse_x'][0] == 0) and (cv['sse_z'][0] == 0) and (cv['sse_x'][1:] > 0).all()
    # the maxima are decided by more than rounding
    if W > 1:
        assert (hr.top_gap(cv['sq_x'], cv['ok'])[1:] > 1e-9).all() and (hr.top_gap(cv['sq_z'], cv['ok'])[1:] > 1e-9).all()
    # the restatement against the chain: e_np, the yardstick of the end-to-end test
    e_np = float(np.abs(f8['x_pred'].astype(hr.LD) - ld['x_pred']).max() / np.abs(ld['x_pred']).max())
    print('%s: W = %d, %d switches, margin %.2e, e_np %.2e' % (name, W, ld['switches'], ld['margin'], e_np))
    assert e_np <= 1e-12


def test_windows_formula_equals_the_enumeration():
    for E in (1, 3):
        for T in (1, 2, 7, 13, 38):
            for H in (1, 2, 6, 12, 37):
                for stride in (1, 2, 3):
                    for every in (1, 2, 5, 50):
                        a, b = hr.windows(E, T, H, stride, every), hr.windows_brute(E, T, H, stride, every)
                        assert a.shape == b.shape and np.array_equal(a, b), (E, T, H, stride, every)
    assert hr.windows(2, 6, 6, 1, 1).shape[0] == 0 and hr.windows(2, 7, 6, 1, 1).shape[0] == 2


def test_status_of_the_reference():
    c = hc.case('n12')
    mdl = c['model']
    X, U = c['X'].copy(), c['U'].copy()
    X[1, 12, 3] = np.nan
    U[2, 20, 1] = np.inf
    tabs = hr.fe_tables(mdl, mdl['Ts'])
    out = hr.predict(tabs, mdl['q'], mdl['v'], mdl['w'], X, U, c['H'], 1, c['every'], hr.LD)
    w = out['windows']
    reads_x = (w[:, 0] == 1) & (w[:, 1] <= 12) & (12 <= w[:, 1] + c['H'])
    reads_u = (w[:, 0] == 2) & (w[:, 1] <= 20) & (20 <= w[:, 1] + c['H'] - 1)
    assert reads_x.sum() > 0 and reads_u.sum() > 0
    np.testing.assert_array_equal(out['status'], np.where(reads_x | reads_u, 2, 0))
