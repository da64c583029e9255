"""CPU: the input conditions of tests/test_koopman_fit_gpu.py.  The float64 statement of the fit (tests/koopman_fit_reference.py) against
its long-double statement on every case of tests/koopman_fit_cases.py: e_oracle is printed and stays <= 1e-11 (the project's rule), and
the float64 statement alone passes both bounds the device is held to -- the elementwise sums bound (S + 2 degree + 2) eps sum |terms|
and the solve's certificate |X (G + ridge I) - R|_F <= 4 n^2 eps |X|_F |G + ridge I|_F.  The table of cases is checked for coverage."""
import numpy as np
import pytest

import koopman_fit_cases as kc
import koopman_fit_reference as kr

SOLVE = [c for c in kc.CASES if c[1] == 'solve']


def test_observable_order_is_the_products():
    from sofacontrol_amd.baselines.koopman.koopman_utils import observable_exponents
    for ny, m, d, degree, dmd in list(kc.SHAPES) + [(3, 4, 1, 3, False), (2, 3, 2, 2, True)]:
        nz = ny * (d + 1) + m * d
        np.testing.assert_array_equal(kr.exponents(nz, degree, dmd), observable_exponents(nz, degree, dmd))
    for shape, n in kc.SHAPES.items():
        ny, m, d, degree, dmd = shape
        assert len(kr.exponents(ny * (d + 1) + m * d, degree, dmd)) + m == n, shape
    ny, m, d, degree, dmd = kc.REFUSED
    assert len(kr.exponents(ny * (d + 1) + m * d, degree, dmd)) + m == 129


def test_the_table_of_cases_is_covered():
    assert sorted(kc.SHAPES.values()) == [2, 15, 16, 17, 21, 38, 70, 128]
    names = {name for _, name in kc.CASES}
    assert names == {'one-pair', 'TR-1', 'TR', 'TR+1', '2TR+1', 'E3-aligned', 'E3-unaligned', 'empty-between', 'stride3-lag1', 'stride3-lag0',
                     'two-adds', 'one-add', 'solve'}
    for shape in kc.SHAPES:
        d = shape[2]
        want = {'one-pair': 1, 'TR-1': kc.TR - 1, 'TR': kc.TR, 'TR+1': kc.TR + 1, '2TR+1': 2 * kc.TR + 1, 'E3-aligned': 3 * kc.TR,
                'E3-unaligned': 3 * (kc.TR + 5), 'empty-between': 50, 'stride3-lag1': 40, 'stride3-lag0': 9, 'two-adds': 120, 'one-add': 120,
                'solve': 6 * kc.SHAPES[shape]}
        for name, pairs in want.items():
            assert kc.expected_pairs((shape, name)) == pairs == kc.reference((shape, name), np.float64)['pairs'], (shape, name)
        assert {kc.records((shape, k))['u_lag'] for k in want} == {0, 1}
        assert {kc.records((shape, k))['stride'] for k in want} == {1, 3}
        # T is no multiple of the stride where the stride is 3
        for name, rest in (('stride3-lag1', 2), ('stride3-lag0', 1)):
            c = kc.records((shape, name))
            assert c['stride'] == 3 and c['adds'][0][0].shape[1] % 3 == rest
        # the empty episodes are there
        Ts = [Y.shape[1] for Y, _ in kc.records((shape, 'empty-between'))['adds']]
        assert d + 1 in Ts and (d in Ts or d == 0)
        # 'one-add' holds the episodes of 'two-adds'
        two, one = kc.records((shape, 'two-adds'))['adds'], kc.records((shape, 'one-add'))['adds']
        np.testing.assert_array_equal(np.concatenate([a[0] for a in two]), one[0][0])
        np.testing.assert_array_equal(np.concatenate([a[1] for a in two]), one[0][1])


@pytest.mark.parametrize('case', kc.CASES, ids=kc.case_id)
def test_float64_sums_stay_inside_the_sums_bound(case):
    """The oracle alone passes the bound the device is held to.  The bound counts S + 2 degree + 2 roundings on a term, and a term of G
    or R is a product of two observables, i.e. of up to 2 degree scaled samples: with a sample rounded once (scale_down) it carries
    2 degree + 2 (degree - 1) + 1 roundings at first order (one per sample, one per product of the recurrence, one for the product
    of the two observables), which the bound covers up to degree 2 for any S; at degree 3 the worst case is 11 eps against the 9 eps
    of one pair.  With the scaling's subtraction and division rounded separately a sample brings 2 eps per occurrence, a degree-2
    term 11 eps against 7, and z^3 z^3 of shape (1, 1, 1, 3, False) with one pair measured 1.005 of the bound: that is why the fit
    rounds a scaled sample once.  As it stands the one-pair cases use 0.17 to 0.71 of the bound (0.31 at degree 3), every case with
    more pairs at most 0.30."""
    c = kc.records(case)
    ref, f64 = kc.reference(case, kr.LD), kc.reference(case, np.float64)
    use = kr.sums_use(f64['G'], f64['R'], ref, c['degree'])
    print('%s: pairs %d, float64 uses %.3g of the sums bound' % (kc.case_id(case), ref['pairs'], use))
    assert f64['pairs'] == ref['pairs'] == kc.expected_pairs(case)
    assert use <= 1.0


@pytest.mark.parametrize('case', SOLVE, ids=kc.case_id)
def test_float64_model_against_long_double(case):
    e = kc.e_oracle(case)
    f64 = kc.reference(case, np.float64)
    A, B = kc.model_reference(case, np.float64)
    res, bound = kr.certificate(np.hstack([A, B]), f64['G'], f64['R'], 0.0)
    print('%s: e_oracle %.3e (tolerance %.3e); float64 certificate %.3e of %.3e (%.2g of it)' % (kc.case_id(case), e, kr.tolerance(e), res, bound,
                                                                                             res / bound))
    assert e <= kr.E_ORACLE_MAX
    assert res <= bound


def test_float64_certificate_on_the_smooth_trajectory():
    c = kc.smooth_case()
    scale = kr.scale_from(c['adds'], 1)
    s = kr.sums(c['adds'], scale, c['delays'], c['degree'], c['dmd'], 1, 0, np.float64)
    X = kr.solve(s['G'], s['R'], 0.0, np.float64)
    res, bound = kr.certificate(X, s['G'], s['R'], 0.0)
    print('smooth: cond(G) %.2e, float64 certificate %.3e of %.3e' % (np.linalg.cond(s['G']), res, bound))
    assert s['pairs'] == 600 and np.linalg.cond(s['G']) > 1e5
    assert res <= bound
