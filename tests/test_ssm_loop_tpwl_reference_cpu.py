"""CPU: the input conditions of the cases of tests/ssm_loop_tpwl_cases.py, on the reference alone (no GPU, nothing under test): every
nearest-point lookup of the gain-free chains is decided by more than cl_reference.MARGIN, every member of every multi-sub-step case
changes region inside the window -- but for the two members that ssm_loop_tpwl_cases.STAYING names, which are asserted to stay --, the
float64 chain stays within E_ORACLE_MAX of the long-double chain on every field and picks the long-double regions.

Measured: least margin 7.4e-5 (g6-5-max), 1.3e-4 at g6-260, at least 1.9e-3 elsewhere; 2-5 regions per member except g6-knots-1 (one
sub-step) and members 1, 2 of r36-5-10 (one region); e_oracle at most 1.2e-15; max |y - z_ref| at most 6.8."""
import numpy as np
import pytest

import cl_reference as cr
import ssm_loop_tpwl_cases as stc


@pytest.mark.parametrize('pair', stc.PAIRS, ids=[stc.case_id(p) for p in stc.PAIRS])
def test_input_conditions(pair):
    i, r = stc.inputs(pair), stc.reference(pair)
    regions = [len(set(row.tolist())) for row in r['picks']]
    yd = float(np.abs(np.asarray(r['ref']['Y'], dtype=np.float64) - stc.observer_model(pair[1])['z_ref']).max())
    print('%s: B %d, n_keep %d, n_p %d, n_o %d; least margin %.3e; regions per member %d..%d; max |y - z_ref| %.3g; e_oracle %s' %
          (stc.case_id(pair), i['B'], i['n_keep'], i['x'].shape[1], i['C'].shape[0], r['margin'], min(regions), max(regions), yd,
           ', '.join('%s %.2e' % (f, e) for f, e in r['e_oracle'].items())))
    assert r['margin'] > cr.MARGIN
    if i['n_keep'] > 1:
        staying = [b for b, k in enumerate(regions) if k < 2]
        assert staying == stc.STAYING.get(pair[0], []), regions
        assert max(regions) >= 2
    for f, e in r['e_oracle'].items():
        assert e <= cr.E_ORACLE_MAX, (f, e)
    np.testing.assert_array_equal(r['picks64'], r['picks'])
    assert abs(float(np.abs(i['x'] @ i['C'].T).max()) - 0.3) < 1e-12
    for f in stc.FIELDS:
        assert np.isfinite(np.asarray(r['ref'][f], dtype=np.float64)).all(), f
