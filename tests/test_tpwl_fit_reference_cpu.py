"""CPU: the inputs the GPU tests of the TPWL fit rely on hold for the seeded cases -- the float64 statement of the fit sits within the
sums bound of the long-double one, every point search is decided by a margin that rounding cannot close, the equilibrated blocks are
well conditioned, every point has the samples to solve, the long-double fit returns the generating tables, and at least one case
changes region inside its episodes.  The bound's constant is derived in tpwl_fit_reference.sums_constant."""
import numpy as np
import pytest

import tpwl_fit_cases as fc
import tpwl_fit_reference as fr

_switches = {}


@pytest.mark.parametrize('name', list(fc.CASES))
def test_case_is_fit_for_the_gpu_tests(name):
    from sofacontrol_amd.tpwl import sysid  # noqa: F401  (the cases belong to the feature: without it nothing here is stated)
    mdl = fc.known_model(name)
    X, U, _switches[name] = fc.records(name)
    n = 2 * mdl['r'] + mdl['m'] + 1
    ref, f64 = fc.reference(name), fc.reference(name, dtype=np.float64)
    np.testing.assert_array_equal(f64['region'], ref['region'])
    use = max(fr.sums_use(f64['G'][p], f64['R'][p], ref, p) for p in range(mdl['P']))
    tb = fr.tables(ref, mdl['q'], mdl['v'], mdl['m'], range(mdl['P']))
    errs = [float(np.abs(np.asarray(tb[k][p]) - mdl[k][p]).max()) for p in range(mdl['P']) for k in ('A_c', 'B_c', 'd_c')]
    scale = max(np.abs(mdl['A_c']).max(), np.abs(X).max() / mdl['Ts'])
    print('%s: n = %d, S_p = %r, switches %d, least margin %.3g, kappa %.3g, float64 sums use %.3g of the bound, long-double recovery %.3g'
          % (name, n, ref['S'], _switches[name], ref['margin'], tb['kappa'], use, max(errs)))
    assert use <= 1.0
    assert ref['margin'] >= 1e-6
    assert tb['kappa'] <= 1e8
    assert min(ref['S']) >= 2 * n
    # the records carry float64 rounding of |x| eps, the target that over Ts
    assert max(errs) <= 64 * tb['kappa'] * fr.EPS * scale
    for p in range(mdl['P']):
        assert float(np.abs(tb['u'][p] - U[:, :-1].reshape(-1, mdl['m'])[ref['region'] == p].mean(axis=0)).max()) <= 1e-12


def test_some_case_switches_region_inside_its_episodes():
    sw = {name: fc.records(name)[2] for name in fc.CASES}
    print(sw)
    assert max(sw.values()) > 0 and sw['n77'] > 0


def test_nearest_is_the_first_minimum_and_copies_carry_no_margin():
    q = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 2.0]])
    v = np.zeros((4, 2))
    x = np.array([[0.0, 0.0, 0.1, 0.0], [0.0, 0.0, 0.5, 0.0], [0.0, 0.0, 0.9, 0.1]])
    idx, mg = fr.nearest(x, q, v, {'q': 1.0, 'v': 0.0})
    np.testing.assert_array_equal(idx, [0, 0, 1])              # the tie at (0.5, 0) and the copy (point 2) go to the smaller index
    assert mg[1] == 0.0 and mg[0] > 0.5
    idx, mg = fr.nearest(x, q[:1], v[:1], {'q': 1.0, 'v': 0.0})
    assert np.all(idx == 0) and np.all(np.isinf(mg))


def test_sums_constant_is_derived():
    assert fr.sums_constant(100) == 104 * 2.0 ** -53
    for word in ('rounded once', 'carries 2', 'S + 1 additions', 'granule'):
        assert word in fr.sums_constant.__doc__, word
