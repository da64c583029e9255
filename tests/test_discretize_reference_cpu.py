"""CPU: the fixture of the discretisation kernel's exact tests (tests/golden/g24_discretize.npz) checked against what it must
equal -- its own regeneration (under mpmath), closed forms, exact rational arithmetic -- the paths that the cases are listed for
(squaring counts and their parities, pivot rows, exactness of the dyadic elimination, the LDS limit), and the yardsticks from which
the device bounds of tests/test_discretize_exact_gpu.py are set: the error of float64 codes of the same kind against the fixture."""
from fractions import Fraction

import numpy as np
import pytest

import discretize_cases as dc
import discretize_reference as dr

ZOH = [c for c in dc.fixture_cases() if c[1] == 'zoh']
SOLVE = [c for c in dc.fixture_cases() if c[1] in ('be', 'bil')]


# -------------------------------------------------------------------------------------------------------- regeneration
def test_fixture_holds_every_case_and_stays_small():
    import os
    g = dc.load_fixture()
    for key, method, dt, A, B, d in dc.fixture_cases():
        assert g[key + '/Ad'].shape == A.shape and g[key + '/Bd'].shape == B.shape and g[key + '/dd'].shape == d.shape, key
        assert all(np.isfinite(g[key + '/' + o]).all() for o in ('Ad', 'Bd', 'dd')), key
        assert (key + '/s' in g) == (method == 'zoh')
    assert os.path.getsize(dc.GOLDEN) < 300 * 1024


@pytest.mark.parametrize('key', dc.REGENERATED)
def test_fixture_regenerates_bit_for_bit(key):
    pytest.importorskip('mpmath')
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('make_golden_discretize',
                                                  os.path.join(os.path.dirname(dc.GOLDEN), 'make_golden_discretize.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = dc.load_fixture()
    new = gen.entries(*dc.case(key))
    assert sorted(new) == sorted(k for k in g if k.startswith(key + '/'))
    for k, v in new.items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k


# -------------------------------------------------------------------------------------------------------- closed forms
def _within_one_ulp(key, closed):
    for got, ref, o in zip(dc.expected(key), closed, ('Ad', 'Bd', 'dd')):
        worst = float(dr.ulps(got[0], ref).max())
        print('%s %s: %.2f ulp from the closed form' % (key, o, worst))
        assert worst <= 1.0, (key, o, worst)


def test_closed_form_scalar():
    """exp(a dt), b (exp(a dt) - 1) / a, d (exp(a dt) - 1) / a, in long double through expm1."""
    _, _, dt, A, B, d = dc.case('z_one')
    L = np.longdouble
    a = L(A[0, 0, 0])
    g = np.expm1(a * L(dt)) / a
    _within_one_ulp('z_one', (np.array([[np.exp(a * L(dt))]], dtype=np.float64), np.array([[L(B[0, 0, 0]) * g]], dtype=np.float64),
                              np.array([L(d[0, 0]) * g], dtype=np.float64)))


def test_closed_form_zero_A():
    """M^2 = 0: exp(M) = I + M, and the rounded products dt B, dt d are what float64 gives."""
    _, _, dt, A, B, d = dc.case('z_zero_A')
    Ad, Bd, dd = dc.expected('z_zero_A')
    assert np.array_equal(Ad[0], np.eye(6)) and np.array_equal(Bd[0], dt * B[0]) and np.array_equal(dd[0], dt * d[0])


def test_closed_form_nilpotent():
    """The finite sum of M^k / k! in fractions.Fraction, rounded once."""
    _, _, dt, A, B, d = dc.case('z_nilpotent')
    M = dr.augmented(A[0], B[0], d[0], dt)
    assert np.array_equal(M, np.triu(M, 1)) and np.array_equal(M * 4, np.round(M * 4))             # strictly upper, dyadic
    E = dr.expm_nilpotent_fraction([[Fraction(float(v)) for v in row] for row in M])
    E = np.array([[float(v) for v in row] for row in E])
    n, m = B.shape[1:]
    Ad, Bd, dd = dc.expected('z_nilpotent')
    assert np.array_equal(Ad[0], E[:n, :n]) and np.array_equal(Bd[0], E[:n, n:n + m]) and np.array_equal(dd[0], E[:n, n + m])
    assert np.abs(E - np.eye(13) - M).max() > 0.1                                             # the higher terms are not negligible


def test_closed_form_rotation():
    _within_one_ulp('z_rotation', dc.rotation_closed_form())
    assert dc.load_fixture()['z_rotation/nrm'][0] >= 40.0


# ------------------------------------------------------------------------------------------------------- path coverage
def test_squaring_counts_reach_every_path():
    g = dc.load_fixture()
    for key, method, dt, A, B, d in ZOH:
        for b in range(A.shape[0]):
            M = dr.augmented(A[b], B[b], d[b], dt)
            assert g[key + '/s'][b] == dr.squarings(M) and g[key + '/nrm'][b] == dr.norm1(M)
            # no case sits at a threshold of the rule: the device's own summation order cannot change its s
            frac = np.log2(max(dr.norm1(M), 1e-300) / dr.THETA_13)
            assert dr.norm1(M) < 0.995 * dr.THETA_13 or abs(frac - round(frac)) > 0.01, (key, b, frac)
    s_all = sorted({int(s) for key, *_ in ZOH for s in g[key + '/s']})
    print('squaring counts of the zoh cases:', {key: g[key + '/s'].tolist() for key, *_ in ZOH})
    assert 0 in s_all and 1 in s_all and any(s > 1 and s % 2 for s in s_all) and any(s > 1 and s % 2 == 0 for s in s_all)
    assert [int(g['z_threshold[%d]/s' % k][0]) for k in range(4)] == list(dc.THRESHOLD_S)
    for k, t in enumerate(dc.THRESHOLD_TARGETS):
        assert abs(g['z_threshold[%d]/nrm' % k][0] / t - 1) < 1e-12
    assert g['z_mixed_batch/s'].tolist() == list(dc.MIXED_S)
    assert g['z_tile_plus_one@2dt/s'][0] == g['z_tile_plus_one@dt/s'][0] + 1                 # both parities at ne = NP + 1
    assert g['z_stiff/s'][0] >= 17 and g['z_one/s'][0] == 0 and g['z_zero_A/s'][0] == 0
    assert float(np.abs(g['z_unstable/Ad']).max()) > np.exp(7.0)


def test_shapes_sit_at_the_tile_edges():
    shapes = {key: dc.ne_np(A.shape[1], B.shape[2]) for key, _, _, A, B, _ in ZOH}
    assert shapes['z_one'] == (3, 16) and shapes['z_full_tile'] == (16, 16) and shapes['z_tile_plus_one@dt'] == (17, 32)
    assert shapes['z_two_tiles[28,3]'] == (32, 32) and shapes['z_two_tiles[30,2]'] == (33, 48) and shapes['z_wide'] == (66, 80)
    assert shapes['z_mixed_batch'] == (17, 32)


@pytest.mark.parametrize('method', ['be', 'bil'])
def test_far_pivot_rows(method):
    """The float64 elimination finds its pivots where the case says: rows 69 and 68 (>= p + 64) for columns 0 and 3, the diagonal
    elsewhere; a search that stops after its first 64 rows takes another pivot there and its result misses the device bound."""
    _, _, dt, A, B, d = dc.case('b_far_pivot/' + method)
    Ad, Bd, dd, piv = dr.eliminate(A[0], B[0], d[0], dt, method)
    assert piv == [dc.FAR_PIVOT_ROWS.get(p, p) for p in range(70)]
    T = dr.tableau(A[0], B[0], d[0], dt, method)
    assert int(np.argmax(np.abs([row[0] for row in T]))) == 69
    key = 'b_far_pivot/' + method
    exp = [x[0] for x in dc.expected(key)]
    assert dc.max_err((Ad, Bd, dd), exp) <= dc.solve_bound(key, 70)
    Ad1, Bd1, dd1, piv1 = dr.eliminate(A[0], B[0], d[0], dt, method, search=lambda p: range(p, min(70, p + 64)))
    print('%s: first-pass-only search pivots %r at columns 0 and 3, error / bound %.1f' %
          (key, (piv1[0], piv1[3]), dc.max_err((Ad1, Bd1, dd1), exp) / dc.solve_bound(key, 70)))
    assert piv1[0] < 64 and dc.max_err((Ad1, Bd1, dd1), exp) > dc.solve_bound(key, 70)


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('method', ['be', 'bil'])
def test_dyadic_elimination_is_exact(method, shifted):
    A, B, d = dc.dyadic(method, shifted)
    Ad, Bd, dd, piv = dc.dyadic_expected(method, shifted)
    got = dr.eliminate(A, B, d, dc.DYADIC_DT, method)
    assert np.array_equal(got[0], Ad) and np.array_equal(got[1], Bd) and np.array_equal(got[2], dd) and got[3] == piv
    n = 8
    assert piv == ([n - 1] * n if shifted else list(range(n)))       # a swap in every column that has a row to swap with
    # the same numbers from the formulas: A_d (I - c A) = R, exactly
    c = dc.DYADIC_DT if method == 'be' else dc.DYADIC_DT / 2
    R = np.eye(n) if method == 'be' else np.eye(n) + c * A
    assert np.array_equal((np.eye(n) - c * A) @ Ad, R) and np.array_equal((np.eye(n) - c * A) @ Bd, dc.DYADIC_DT * B)
    assert np.abs(Ad).max() > 2.0                             # (the entries of T are at most 2)


def test_fe_fixture_is_the_rounded_elementwise_form():
    _, _, dt, A, B, d = dc.case('f_small')
    Ad, Bd, dd = dc.expected('f_small')
    off = ~np.eye(5, dtype=bool)
    assert np.array_equal(Ad[0][off], (dt * A[0])[off]) and np.array_equal(Bd[0], dt * B[0]) and np.array_equal(dd[0], dt * d[0])
    # the diagonal is 1 + dt a rounded once; float64's two roundings stay inside the device bound, taken against the unrounded value
    for i in range(5):
        assert Ad[0, i, i] == float(dc.fe_diagonal_exact(dt, A[0, i, i]))
        assert dc.fe_diagonal_ok(1.0 + dt * A[0, i, i], dt, A[0, i, i])


def test_lds_limit_numbers_follow_from_the_formula():
    for method, (ok, refused) in dc.LDS_LIMIT.items():
        assert refused == ok + 1 and dc.lds_bytes(ok, 1, method) <= dc.LDS_MAX < dc.lds_bytes(refused, 1, method), method
    assert dc.lds_bytes(100, 1, 'be') == 163328 and dc.lds_bytes(98, 1, 'zoh') == 161888


def test_singular_and_nonfinite_cases_are_what_they_say():
    for method in ('be', 'bil'):
        A, B, d = dc.singular_batch(method)
        c = dc.SINGULAR_DT if method == 'be' else dc.SINGULAR_DT / 2
        for b in range(4):
            W = np.eye(4) - c * A[b]
            assert np.array_equal(W, np.zeros((4, 4))) if b in (1, 3) else np.linalg.cond(W) < 10
    for place in dc.NONFINITE_PLACES:
        A, B, d = dc.nonfinite_batch(place)
        bad = [not (np.isfinite(A[b]).all() and np.isfinite(B[b]).all() and np.isfinite(d[b]).all()) for b in range(3)]
        assert bad == [False, True, False]
        assert sum(int((~np.isfinite(x)).sum()) for x in (A, B, d)) == 1


# ---------------------------------------------------------------------------------------------------------- yardsticks
def _zoh_ratio(key, A, B, d, dt, expm):
    """err / (ne 2^s 2^-53 max |expected|) per member: the device bound without its constant."""
    n, m = B.shape[1:]
    out = []
    for b in range(A.shape[0]):
        got = dr.f64_discretize(A[b], B[b], d[b], dt, 'zoh', expm=expm)
        exp = [x[b] for x in dc.expected(key)]
        out.append(dc.max_err(got, exp) / (dc.zoh_bound(key, n, m, b) / dc.C_Z))
    return out


def test_yardsticks_zoh():
    """Measures, prints, and holds C_Z to its rule: four times the largest ratio of the float64 restatement of Alg. 2.3, rounded up to a
    power of two, and never above 1 (the cap is what holds here: 4 x 0.45 at z_one, 4 x 0.31 at z_unstable)."""
    from scipy.linalg import expm as scipy_expm
    worst = 0.0
    for key, _, dt, A, B, d in ZOH:
        rp, rs = _zoh_ratio(key, A, B, d, dt, dr.expm_pade13), _zoh_ratio(key, A, B, d, dt, scipy_expm)
        print('%-22s s %-22s Alg. 2.3 %s   scipy %s' % (key, dc.load_fixture()[key + '/s'].tolist(), ' '.join('%.4f' % r for r in rp),
                                                     ' '.join('%.4f' % r for r in rs)))
        worst = max(worst, max(rp))
    print('largest ratio of the restatement %.4f -> C_Z = %g' % (worst, dc.C_Z))
    assert dc.C_Z == min(1.0, 2.0 ** np.ceil(np.log2(4.0 * worst)))


def test_yardsticks_be_bil():
    """Measures and prints e_np, the error of np.linalg.solve relative to max |expected|; the stored values are these rounded up."""
    for key, method, dt, A, B, d in SOLVE:
        n = A.shape[1]
        got = dr.f64_discretize(A[0], B[0], d[0], dt, method)
        exp = [x[0] for x in dc.expected(key)]
        big = max(float(np.abs(x).max()) for x in exp)
        e_np = dc.max_err(got, exp) / big
        c = dt if method == 'be' else dt / 2
        print('%-18s e_np %.2e (stored %.2e), n 2^-53 %.2e, cond_inf %.1e' %
              (key, e_np, dc.E_NP[key], n * dc.U, np.linalg.cond(np.eye(n) - c * A[0], np.inf)))
        assert e_np <= dc.E_NP[key] <= 1e-14
