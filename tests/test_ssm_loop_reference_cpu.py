"""CPU: the reference statement of the SSM closed loop's sub-step chain (tests/ssm_loop_reference.py) on the seeded cases of
tests/ssm_loop_cases.py.  The float64 chain (oracle/ssm.py) is measured against the long-double chain (tests/ssm_reference.py): that
error, e_oracle, sets the tolerance of the device comparison in tests/test_gusto_ssm_loop_gpu.py, and the rule's cap e_oracle <= 1e-11
is asserted here where no GPU is needed.  Measured on these seeds: e_oracle <= 1.9e-15 for X, Z, U, Y and x_hat on all nine cases, states
below 0.91.  The float64 chain's plant step is tied to the oracle's own rollout on a constant-input plan, bit for bit."""
import numpy as np
import pytest

import ssm_cases as sc
import ssm_loop_cases as slc
import ssm_loop_reference as slr
from oracle import ssm as ossm


@pytest.mark.parametrize('case', slc.ADVANCE, ids=[slc.case_id(c) for c in slc.ADVANCE])
def test_float64_chain_against_the_long_double_chain(case):
    ref, e_oracle = slc.reference(case)
    nk = case[5]
    for f in slc.FIELDS:
        assert ref[f].dtype == slr.LD and ref[f].shape[:2] == (slc.B, nk)
    print('%s: e_oracle %s, max |x| %.3f' % (slc.case_id(case), ' '.join('%s %.2e' % (f, e_oracle[f]) for f in slc.FIELDS),
                                            float(np.abs(ref['X']).max())))
    for f in slc.FIELDS:
        assert e_oracle[f] <= sc.E_ORACLE_MAX, (f, e_oracle[f])
    assert np.isfinite(ref['X'].astype(np.float64)).all() and float(np.abs(ref['X']).max()) < 1.0      # the states stay of order one
    # the plant differs from the planner, and the noise is felt
    assert not np.array_equal(slc.plant_model(case[0])['W'], sc.model(case[0])['W'])
    i = slc.inputs(case)
    np.testing.assert_array_equal(ref['Y'].astype(np.float64),
                                  ((ref['Z'] + slr.LD(1) * slc.plant_model(case[0])['z_ref']) + i['V'].transpose(1, 0, 2)).astype(np.float64))


@pytest.mark.parametrize('case', slc.ADVANCE, ids=[slc.case_id(c) for c in slc.ADVANCE])
def test_plant_step_of_the_float64_chain_is_the_oracles_rollout(case):
    s, method, dt_sim, dt, N, nk = case
    plant, planner = sc.oracle_model(slc.plant_model(s)), sc.oracle_model(sc.model(s))
    i = slc.inputs(case)
    u = i['uopt'][0, 0]
    X, Z, U, Y, Xh = slr.advance(plant, planner, method, dt_sim, np.tile(u, (N, 1)), i['x'][0], i['j'], i['theta'], None, None, np.float64)
    xr, zr = ossm.rollout(plant, i['x'][0], np.tile(u, (nk, 1)), dt_sim, 'fe' if method == 'map' else method, discrete=method == 'map')
    np.testing.assert_array_equal(U, np.tile(u, (nk, 1)))
    np.testing.assert_array_equal(X, xr[1:])
    np.testing.assert_array_equal(Y, zr[1:])               # the oracle's z carries z_ref: the measurement without noise
    np.testing.assert_array_equal(Xh, np.stack([ossm.reduce(planner, y) for y in Y]))
