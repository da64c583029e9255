"""GPU: csrc/discretize.hip (stpwl_discretize_dev) on every method, path and edge, against the multiprecision fixture
tests/golden/g24_discretize.npz (tests/discretize_cases.py lists the cases and where the constants of the bounds come from;
tests/test_discretize_reference_cpu.py checks the fixture and measures those constants without a GPU).

  fe        off-diagonal A_d, B_d, d_d bit for bit; the diagonal of A_d within 2^-53 (|dt a| + |1 + dt a|) of 1 + dt a
  be / bil  the dyadic cases bit for bit; the others within 16 max(e_np, n 2^-53) max |expected|
  zoh       within C_Z ne 2^s 2^-53 max |expected| over the three outputs, s from the fixture

Every output of every call sits between sentinel guards that are checked after the call; a member of a batch equals the same model
solved alone bit for bit; a failed member leaves the others' results as they are."""
import ctypes as C

import numpy as np
import pytest

import discretize_cases as dc
import discretize_reference as dr
from test_pod_build_exact_gpu import Guarded, SENTINEL, _dev

pytestmark = pytest.mark.gpu

ZOH = [c[0] for c in dc.fixture_cases() if c[1] == 'zoh']
SOLVE = [c[0] for c in dc.fixture_cases() if c[1] in ('be', 'bil')]


def discretize(method, A, B, d, dt):
    """(rc, message, A_d, B_d, d_d) of one stpwl_discretize_dev call on a batch; the three outputs guarded."""
    from sofacontrol_amd import _lib
    L = _lib.lib()
    batch, n, m = B.shape
    dA, dB, dd_in = _dev(A), _dev(B), _dev(d)
    oA, oB, oD = Guarded(batch * n * n), Guarded(batch * n * m), Guarded(batch * n)
    rc = L.stpwl_discretize_dev(C.c_int(dc.CODE[method]), C.c_int(n), C.c_int(m), C.c_int64(batch), dA.ptr, dB.ptr, dd_in.ptr,
                                C.c_double(dt), oA.ptr, oB.ptr, oD.ptr, None)
    msg = L.srh_last_error().decode(errors='replace') if rc != 0 else ''
    _lib.sync()
    return rc, msg, oA.get((batch, n, n)), oB.get((batch, n, m)), oD.get((batch, n))


def solved(method, A, B, d, dt):
    rc, msg, Ad, Bd, dd = discretize(method, A, B, d, dt)
    assert rc == 0, msg
    return Ad, Bd, dd


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def untouched(x):
    return np.array_equal(x, np.full(x.shape, SENTINEL))


# ------------------------------------------------------------------------------------------------------------------ fe
def test_fe_elementwise():
    key, method, dt, A, B, d = dc.case('f_small')
    Ad, Bd, dd = solved('fe', A, B, d, dt)
    eAd, eBd, edd = dc.expected(key)
    off = ~np.eye(5, dtype=bool)
    assert np.array_equal(Ad[0][off], eAd[0][off]) and np.array_equal(Ad[0][off], (dt * A[0])[off])
    assert np.array_equal(Bd, eBd) and np.array_equal(Bd, dt * B) and np.array_equal(dd, edd) and np.array_equal(dd, dt * d)
    for i in range(5):
        print('fe diagonal %d: %.17g, fixture %.17g' % (i, Ad[0, i, i], eAd[0, i, i]))
        assert dc.fe_diagonal_ok(Ad[0, i, i], dt, A[0, i, i])


# ----------------------------------------------------------------------------------------------------------------- zoh
@pytest.mark.parametrize('key', ZOH)
def test_zoh_against_the_fixture(key):
    _, _, dt, A, B, d = dc.case(key)
    batch, n, m = B.shape
    got = solved('zoh', A, B, d, dt)
    exp = dc.expected(key)
    s = dc.load_fixture()[key + '/s']
    for b in range(batch):
        err, bound = dc.max_err([x[b] for x in got], [x[b] for x in exp]), dc.zoh_bound(key, n, m, b)
        print('%s[%d]: s %d, error %.3e, bound %.3e, ratio %.3f' % (key, b, s[b], err, bound, err / bound))
    for b in range(batch):
        assert dc.max_err([x[b] for x in got], [x[b] for x in exp]) <= dc.zoh_bound(key, n, m, b), (key, b)


def test_zoh_mixed_batch_members_are_independent_and_the_host_entry_agrees():
    """Six workgroups with s = 0, 1, 4, 9, 10, 0: each with its own parity and workspace slice."""
    from sofacontrol_amd import _lib
    _, _, dt, A, B, d = dc.case('z_mixed_batch')
    got = solved('zoh', A, B, d, dt)
    for b in range(A.shape[0]):
        alone = solved('zoh', A[b:b + 1], B[b:b + 1], d[b:b + 1], dt)
        assert same([x[b] for x in got], [x[0] for x in alone]), b
    Ad, Bd, dd = np.empty_like(A), np.empty_like(B), np.empty_like(d)
    _lib.check(_lib.lib().stpwl_discretize(C.c_int(3), C.c_int(A.shape[1]), C.c_int(B.shape[2]), C.c_int64(A.shape[0]), _lib.dptr(A),
                                           _lib.dptr(B), _lib.dptr(d), C.c_double(dt), _lib.dptr(Ad), _lib.dptr(Bd), _lib.dptr(dd)),
               'stpwl_discretize')
    assert same(got, (Ad, Bd, dd))


# ------------------------------------------------------------------------------------------------------------ be / bil
@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('method', ['be', 'bil'])
def test_dyadic_elimination_bit_exact(method, shifted):
    A, B, d = dc.dyadic(method, shifted)
    eAd, eBd, edd, _ = dc.dyadic_expected(method, shifted)
    Ad, Bd, dd = solved(method, A[None], B[None], d[None], dc.DYADIC_DT)
    assert np.array_equal(Ad[0], eAd) and np.array_equal(Bd[0], eBd) and np.array_equal(dd[0], edd)


@pytest.mark.parametrize('key', SOLVE)
def test_be_bil_against_the_fixture(key):
    _, method, dt, A, B, d = dc.case(key)
    n = A.shape[1]
    got = solved(method, A, B, d, dt)
    err, bound = dc.max_err([x[0] for x in got], [x[0] for x in dc.expected(key)]), dc.solve_bound(key, n)
    print('%s: error %.3e, bound %.3e, ratio %.3f' % (key, err, bound, err / bound))
    assert err <= bound


@pytest.mark.parametrize('method', ['be', 'bil'])
def test_be_bil_batch_members_are_independent(method):
    A, B, d = dc.fem_batch3(12, method)
    got = solved(method, A, B, d, 0.05)
    for b in range(3):
        alone = solved(method, A[b:b + 1], B[b:b + 1], d[b:b + 1], 0.05)
        assert same([x[b] for x in got], [x[0] for x in alone]), b
    key = 'b_fem[12,3]/' + method
    assert dc.max_err([x[0] for x in got], [x[0] for x in dc.expected(key)]) <= dc.solve_bound(key, 12)


@pytest.mark.parametrize('method', ['be', 'bil'])
def test_singular_members_are_reported_by_the_first_index(method):
    A, B, d = dc.singular_batch(method)
    rc, msg, Ad, Bd, dd = discretize(method, A, B, d, dc.SINGULAR_DT)
    assert rc == -4 and 'singular' in msg and '(model 1)' in msg, (rc, msg)
    for b in (0, 2):                          # the members that did not fail are as if solved alone, the failed ones' slices untouched
        alone = solved(method, A[b:b + 1], B[b:b + 1], d[b:b + 1], dc.SINGULAR_DT)
        assert same((Ad[b], Bd[b], dd[b]), [x[0] for x in alone])
    for b in (1, 3):
        assert untouched(Ad[b]) and untouched(Bd[b]) and untouched(dd[b])


# ------------------------------------------------------------------------------------------------------- the LDS limit
@pytest.mark.parametrize('method', ['be', 'bil', 'zoh'])
def test_lds_limit_runs_and_the_next_size_is_refused(method):
    """The largest model whose tableau fits 160 KB of LDS (m = 1), against the float64 restatement at the 1e-10 of
    tests/test_tpwl_gpu.py (the point is addressing), and the refusal of the next size, which names n_x."""
    n_ok, n_refused = dc.LDS_LIMIT[method]
    A, B, d = dc.lds_model(n_ok)
    got = solved(method, A[None], B[None], d[None], dc.LDS_DT)
    ref = dr.f64_discretize(A, B, d, dc.LDS_DT, method)
    big = max(1.0, max(float(np.abs(x).max()) for x in ref))
    err = dc.max_err([x[0] for x in got], ref)
    print('%s at n = %d (%d bytes of LDS): error %.2e' % (method, n_ok, dc.lds_bytes(n_ok, 1, method), err / big))
    assert err <= 1e-10 * big
    A, B, d = dc.lds_model(n_refused)
    rc, msg, Ad, Bd, dd = discretize(method, A[None], B[None], d[None], dc.LDS_DT)
    assert rc == -1 and 'n_x %d' % n_refused in msg and 'LDS' in msg, (rc, msg)
    assert untouched(Ad) and untouched(Bd) and untouched(dd)


# ---------------------------------------------------------------------------------------------------- non-finite models
@pytest.mark.parametrize('place', dc.NONFINITE_PLACES)
@pytest.mark.parametrize('method', ['be', 'bil', 'zoh'])
def test_nonfinite_model_is_reported(method, place):
    """A NaN or Inf anywhere in A, B or d of member 1 of 3: SRH_ENUMERIC, "non-finite model (model 1)"; members 0 and 2 as if
    solved alone, member 1's outputs untouched."""
    A, B, d = dc.nonfinite_batch(place)
    rc, msg, Ad, Bd, dd = discretize(method, A, B, d, dc.NONFINITE_DT)
    assert rc == -4 and 'non-finite model (model 1)' in msg, (rc, msg)
    for b in (0, 2):
        alone = solved(method, A[b:b + 1], B[b:b + 1], d[b:b + 1], dc.NONFINITE_DT)
        assert same((Ad[b], Bd[b], dd[b]), [x[0] for x in alone])
        assert np.isfinite(Ad[b]).all() and np.isfinite(Bd[b]).all() and np.isfinite(dd[b]).all()
    assert untouched(Ad[1]) and untouched(Bd[1]) and untouched(dd[1])


@pytest.mark.parametrize('method', ['be', 'bil'])
def test_nonfinite_takes_precedence_over_singular_and_the_lowest_index_is_named(method):
    A, B, d = dc.singular_batch(method)
    d[1, 2] = np.nan                                            # member 1: I - c A = 0 and a NaN in d
    rc, msg, *_ = discretize(method, A, B, d, dc.SINGULAR_DT)
    assert rc == -4 and 'non-finite model (model 1)' in msg, (rc, msg)
    A, B, d = dc.singular_batch(method)
    B[3, 0, 0] = np.inf                                         # member 1 singular, member 3 non-finite: the lower index is named
    rc, msg, *_ = discretize(method, A, B, d, dc.SINGULAR_DT)
    assert rc == -4 and 'singular' in msg and '(model 1)' in msg, (rc, msg)


@pytest.mark.parametrize('place', dc.NONFINITE_PLACES)
def test_fe_passes_nonfinite_entries_through(place):
    A, B, d = dc.nonfinite_batch(place)
    dt = dc.NONFINITE_DT
    Ad, Bd, dd = solved('fe', A, B, d, dt)
    with np.errstate(invalid='ignore'):
        eAd = dt * A
    off = ~np.eye(6, dtype=bool)
    for b in range(3):
        assert np.array_equal(Ad[b][off], eAd[b][off], equal_nan=True)
        assert np.array_equal(np.isfinite(np.diag(Ad[b])), np.isfinite(np.diag(A[b])))
    assert np.array_equal(Bd, dt * B, equal_nan=True) and np.array_equal(dd, dt * d, equal_nan=True)
