"""CPU: the reference of the SSM horizon error (tests/ssm_horizon_reference.py) and the cases the GPU tests run (tests/ssm_horizon_cases.py)
hold what those tests lean on: the float64 restatement lies inside every bound and within the project's cap of the long-double chain on
every case, the windows formula is the brute-force enumeration, the status rules, and maxima that are decided by more than rounding."""
import numpy as np
import pytest

import ssm_cases as sc
import ssm_horizon_cases as shc
import ssm_horizon_reference as shr


@pytest.mark.parametrize('name,label', shc.case_modes())
def test_float64_restatement_within_the_cap_and_the_bounds(name, label):
    ld, f8 = shc.reference(name, label)
    c = shc.case(name)
    assert (ld['status'] == 0).all() and (f8['status'] == 0).all()
    e, _ = shc.e_np(ld, f8)
    print('%s %s: e_np %s' % (name, label, ', '.join('%s %.1e' % kv for kv in sorted(e.items()))))
    assert max(e.values()) <= sc.E_ORACLE_MAX, (name, label, e)             # no case is skipped to meet the cap
    # the float64 sums of the restatement's own predictions lie inside the bounds stated for any order of summation
    n, W = c['d']['n'], len(ld['status'])
    cv = shr.curves(f8['x_pred'], f8['z_pred'], f8['Xow'], f8['Yw'], f8['status'])
    for key, a, b in (('x', f8['x_pred'], f8['Xow']), ('z', f8['z_pred'], f8['Yw'])):
        d = a - b
        got = (d * d).sum(axis=2).sum(axis=0)
        assert (np.abs(got.astype(shr.LD) - cv['sse_' + key]) <= shr.sse_bound(cv['sse_' + key], n, W)).all(), (name, label, key)
    # without x_start the first row of ex is exactly zero, the first row of ez is not
    assert cv['sse_x'][0] == 0 and cv['sse_z'][0] > 0
    # every maximum is decided by more than rounding -- but the all-zero row 0 of x, and row 0 of z under a linear chart (there
    # C_map(W_map(y)) = y: ez_0 is rounding alone, ssm_horizon_cases.linear_chart)
    if W > 1:
        z0 = 1 if shc.linear_chart(name) else 0
        assert (shr.top_gap(cv['sq_x'], cv['ok'])[1:] > 1e-9).all() and (shr.top_gap(cv['sq_z'], cv['ok'])[z0:] > 1e-9).all(), (name, label)


@pytest.mark.parametrize('E,T,H,stride,every', [(1, 18, 3, 1, 1), (3, 20, 3, 1, 1), (3, 4, 3, 1, 1), (2, 38, 4, 3, 1), (1, 30, 4, 1, 2), (1, 30, 4, 1, 5),
                                               (2, 6, 1, 1, 1), (2, 3, 3, 1, 1), (2, 12, 4, 3, 1), (4, 1002, 20, 1, 49), (2, 50, 12, 2, 7)])
def test_windows_formula_is_the_enumeration(E, T, H, stride, every):
    np.testing.assert_array_equal(shr.windows(E, T, H, stride, every), shr.windows_brute(E, T, H, stride, every))
    if (E, T, H) == (2, 3, 3):
        assert len(shr.windows(E, T, H, stride, every)) == 0                # T' = H: no window
    if (E, T, H, stride) == (2, 12, 4, 3):
        assert len(shr.windows(E, T, H, stride, every)) == 0                # T' = 4 = H under the stride


def test_status_of_the_reference():
    c = shc.case('e3-b17')
    M = sc.oracle_model(c['d'])
    Y, U = c['Y'].copy(), c['U'].copy()
    Y[0, 5, 1], U[1, 7, 0] = np.nan, np.inf
    p = shr.predict(M, 'be', 0.01, Y, U, c['H'], dtype=np.float64)
    wins, H = p['windows'], c['H']
    want = np.zeros(len(wins), dtype=np.int32)
    want[(wins[:, 0] == 0) & (wins[:, 1] <= 5) & (5 <= wins[:, 1] + H)] = 2          # y rows j0 .. j0 + H
    want[(wins[:, 0] == 1) & (wins[:, 1] <= 7) & (7 <= wins[:, 1] + H - 1)] = 2      # u rows j0 .. j0 + H - 1
    np.testing.assert_array_equal(p['status'], want)
    assert np.isnan(p['x_pred'][want == 2]).all() and np.isfinite(p['x_pred'][want == 0]).all()
    # 2 wins over 1: a model whose map overflows at the second step, on records with a bad row
    d = dict(c['d'])
    d['Rd'] = np.hstack([1e200 * np.eye(d['n']), np.zeros((d['n'], d['Rd'].shape[1] - d['n']))])
    q = shr.predict(sc.oracle_model(d), 'map', 0.01, Y, U, c['H'], dtype=np.float64)
    np.testing.assert_array_equal(q['status'], np.where(want == 2, 2, 1))
    cv = shr.curves(q['x_pred'], q['z_pred'], q['Xow'], q['Yw'], q['status'])
    assert np.isnan(cv['worst_x']).all() and (cv['wx'] == -1).all()
