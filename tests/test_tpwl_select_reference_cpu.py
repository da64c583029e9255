"""CPU: the reference of the TPWL point selection (tests/tpwl_select_reference.py) and its cases (tests/tpwl_select_cases.py) are sound
before the kernels are held to them: every comparison of every case's scan is decided (the certificate -- checked here so that a case
cannot hide a failure), every case shows what it was built to show, the long-double scan agrees with the float64 numpy restatement of
tpwl_utils.py:171-196, and the streaming identity holds for the reference itself."""
import numpy as np
import pytest

import tpwl_select_cases as sc
import tpwl_select_reference as sr

NAMES = sorted(sc.build())


@pytest.mark.parametrize('name', NAMES)
def test_every_comparison_of_the_case_is_decided_and_the_case_shows_its_point(name):
    c, ref = sc.build()[name], sc.reference(name)
    ok, bad = sr.certified(ref, c['thr'], c['X'].shape[2] // 2, c['exact'])
    assert ok, (name, bad[:5])
    sc.check_expect(c, ref)
    assert len(ref['q']) == ref['P0'] + len(ref['index']) <= c['max_points']
    if name.startswith('dim_') or name.startswith('edge_n'):
        assert 8 <= len(ref['q']) <= 400, len(ref['q'])             # a scan with decisions of both kinds, not a degenerate one


@pytest.mark.parametrize('name', NAMES)
def test_long_double_scan_agrees_with_the_float64_restatement(name):
    c, ref = sc.build()[name], sc.reference(name)
    f64 = sc.run(sr.scan_f64, c)
    assert np.array_equal(f64['index'], ref['index']) and f64['complete'] == ref['complete'] and f64['stopped_at'] == ref['stopped_at']
    assert np.array_equal(f64['q'], ref['q']) and np.array_equal(f64['v'], ref['v'])
    r = c['X'].shape[2] // 2
    got, want = np.asarray(f64['dmin'], dtype=np.longdouble), ref['dmin']
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert np.all(np.abs(got[fin] - want[fin]) <= sr.bound(r) * np.abs(want[fin]))


def test_wild_velocities_change_nothing_without_a_velocity_weight():
    assert np.array_equal(sc.reference('wv0_wild')['index'], sc.reference('wv0_calm')['index'])
    assert len(sc.reference('wv0_wild')['index']) > 8


def test_the_certificate_refuses_what_it_should():
    assert sr.decided(5.0, 5.0, 2, exact=True) and not sr.decided(5.0, 5.0, 2)
    assert sr.decided(5.0, float(np.nextafter(5.0, np.inf)), 2, exact=True)
    assert not sr.decided(np.nextafter(5.0, 0.0), 5.0, 2, exact=True)        # not an integer: only the margin could decide it
    assert sr.decided(np.inf, 5.0, 2) and not sr.decided(np.nan, 5.0, 2)
    assert sr.decided(5.0 * (1 + 2 * sr.bound(30)), 5.0, 30) and not sr.decided(5.0 * (1 + 0.5 * sr.bound(30)), 5.0, 30)


@pytest.mark.parametrize('name,split', [('two_episodes', 'episode'), ('edge_n3', 1000), ('sep_walk', 'episode'), ('line_65', 100)])
def test_streaming_identity_of_the_reference(name, split):
    """X1 then X2 with the first result as the seed == the concatenation."""
    c, ref = sc.build()[name], sc.reference(name)
    X = c['X']
    X1, X2 = (X[:1], X[1:]) if split == 'episode' else (X[:, :split], X[:, split:])
    a = sc.run(sr.scan, c, X=X1)
    b = sc.run(sr.scan, c, X=X2, q0=a['q'], v0=a['v'])
    assert np.array_equal(b['q'], ref['q']) and np.array_equal(b['v'], ref['v'])
    assert len(a['index']) + len(b['index']) == len(ref['index'])
    assert np.array_equal(np.concatenate([a['dmin'], b['dmin']]), ref['dmin'])
    off = (1, 0) if split == 'episode' else (0, split)
    assert np.array_equal(np.vstack([a['index'], b['index'] + np.array(off)]), ref['index'])
