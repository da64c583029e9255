"""Koopman baseline, host side: the observable order of the device table (skoop_exponents, host-only), KoopmanScaling,
KoopmanData.get_zeta and the KoopmanModel constructor against the reference's golden outputs (g22_koopman.npz)."""
import os

import numpy as np
import pytest

from sofacontrol_amd.baselines.koopman import koopman_utils as ku

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_koopman.npz')


@pytest.fixture(scope='module')
def g():
    return dict(np.load(GOLDEN))


def struct_inputs(g):
    """The loadmat layout of the reference's model file: every field a (1, 1) object array around its value."""
    def wrap(v):
        o = np.empty((1, 1), dtype=object)
        o[0, 0] = v
        return o

    def struct(d):
        names = list(d)
        s = np.zeros((1, 1), dtype=[(k, object) for k in names])
        for k in names:
            s[k][0, 0] = d[k]
        return s
    model = struct({k: g['model_' + k] for k in ('A', 'B', 'C', 'M', 'K')})
    scale = struct({k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')})
    ot = np.empty((1, 1), dtype=object)
    ot[0, 0] = np.array(['poly'])
    params = struct({'n': wrap(np.array([[int(g['param_n'])]], dtype=np.uint8)),
                     'm': wrap(np.array([[int(g['param_m'])]], dtype=np.uint8)),
                     'N': wrap(np.array([[int(g['param_N'])]], dtype=np.uint8)),
                     'nzeta': wrap(np.array([[int(g['param_nzeta'])]], dtype=np.uint8)),
                     'delays': wrap(np.array([[int(g['param_delays'])]], dtype=np.uint8)),
                     'obs_degree': wrap(np.array([[int(g['param_obs_degree'])]], dtype=np.uint8)),
                     'obs_type': wrap(ot), 'Ts': wrap(np.array([[float(g['param_Ts'])]])), 'scale': scale})
    # loadmat hands the reference `raw['model']` (1, 1) and reads fields as model_in['A'][0, 0]
    for k in ('A', 'B', 'C', 'M', 'K'):
        model[k][0, 0] = g['model_' + k]
    return model, params


def dict_inputs(g):
    model = {k: g['model_' + k] for k in ('A', 'B', 'C', 'M', 'K')}
    params = {'n': 3, 'm': 4, 'N': 66, 'nzeta': 10, 'delays': 1, 'obs_degree': 2, 'obs_type': 'poly', 'Ts': 0.05,
              'scale': {k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}}
    return model, params


@pytest.mark.parametrize('nz,deg', [(10, 2), (3, 3), (4, 4)])
@pytest.mark.parametrize('dmd', [0, 1])
def test_observable_order_matches_sympy(g, nz, deg, dmd):
    want = g['order_%d_%d_%d' % (nz, deg, dmd)]
    assert ku.num_observables(nz, deg, bool(dmd)) == want.shape[0]
    np.testing.assert_array_equal(ku.observable_exponents(nz, deg, bool(dmd)), want)


def test_order_is_not_the_ssm_order():
    # within degree 2 of 3 variables: z1^2, z1 z2, z2^2, z1 z3, z2 z3, z3^2 (the issue's check of the sympy call)
    e = ku.observable_exponents(3, 2, True)
    np.testing.assert_array_equal(e[3:], [[2, 0, 0], [1, 1, 0], [0, 2, 0], [1, 0, 1], [0, 1, 1], [0, 0, 2]])


def test_observable_limits():
    assert ku.num_observables(66, 2) == 67 * 68 // 2
    with pytest.raises(RuntimeError):
        ku.observable_exponents(65, 1)
    with pytest.raises(RuntimeError):
        ku.observable_exponents(4, 5)
    with pytest.raises(RuntimeError):
        ku.observable_exponents(64, 2)      # 2145 observables > 1024


@pytest.mark.parametrize('form', ['struct', 'dict'])
def test_scaling(g, form):
    model, params = (struct_inputs if form == 'struct' else dict_inputs)(g)
    s = ku.KoopmanScaling(params['scale'][0, 0] if form == 'struct' else params['scale'])
    assert s.y_offset.shape == (1, 3) and s.u_factor.shape == (1, 4)
    np.testing.assert_array_equal(s.scale_down(y=g['scal_y']), g['scal_y_down'])
    np.testing.assert_array_equal(s.scale_down(u=g['scal_u']), g['scal_u_down'])
    np.testing.assert_array_equal(s.scale_up(y=g['scal_y']), g['scal_y_up'])
    np.testing.assert_array_equal(s.scale_up(u=g['scal_u']), g['scal_u_up'])
    one = s.scale_down(y=g['scal_y'][0])
    assert one.shape == (1, 3)
    np.testing.assert_array_equal(one, g['scal_y1_down'])


@pytest.mark.parametrize('d', [1, 2, 3])
def test_get_zeta_online(g, d):
    _, params = dict_inputs(g)
    kd = ku.KoopmanData(params['scale'], d)
    for i in range(g['rec_y'].shape[0]):
        kd.add_measurement(g['rec_y'][i], g['rec_u'][i])
        z = kd.get_zeta()
        if not g['zeta_online_ok_%d' % d][i]:
            assert z is None
        else:
            np.testing.assert_array_equal(z, g['zeta_online_%d' % d][i])
    assert kd.y_norm.shape == tuple(g['ynorm_shape_%d' % d])


@pytest.mark.parametrize('form', ['struct', 'dict'])
def test_model_constructor(g, form):
    model, params = (struct_inputs if form == 'struct' else dict_inputs)(g)
    km = ku.KoopmanModel(model, params)
    np.testing.assert_array_equal(km.A_d, g['model_A'])
    np.testing.assert_array_equal(km.H, g['model_C'])
    assert (km.n, km.m, km.N, km.state_dim, km.delays, km.obs_degree, km.obs_type, km.Ts) == (3, 4, 66, 10, 1, 2, 'poly', 0.05)
    np.testing.assert_array_equal(km.W, np.eye(66))
    np.testing.assert_array_equal(km.V, np.eye(66))
    assert km.DMD is False and km.n_psi == 66
    assert km.scaling.y_factor.shape == (1, 3)
    for attr in ('A_d', 'B_d', 'C', 'H', 'M', 'K', 'V', 'W', 'n', 'm', 'N', 'state_dim', 'delays', 'obs_degree', 'obs_type',
                 'Ts', 'scale', 'DMD'):
        assert hasattr(km, attr)


def test_model_dimension_checks(g):
    model, params = dict_inputs(g)
    bad = dict(model, B=model['B'][:, :3])
    with pytest.raises(AssertionError):
        ku.KoopmanModel(bad, params)
    bad = dict(model, C=model['C'][:2])
    with pytest.raises(AssertionError):
        ku.KoopmanModel(bad, params)
    with pytest.raises(AssertionError):
        ku.KoopmanModel(model, dict(params, N=65))
