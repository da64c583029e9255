"""GPU: the filter kernels of csrc/observer.hip -- ekf_kernel (VALU), ekf_mfma_kernel<0>, ekf_mfma_kernel<60> and
ekf_wide_kernel -- against the long-double filter of tests/ekf_reference.py on the seeded cases of tests/ekf_cases.py.

Tolerance rule (every comparison with the long-double reference): tol = max(100 e_oracle, 1e-13), e_oracle = the worst error
of the float64 oracle (oracle/observer.py) against the same reference over the same schedule; input condition e_oracle <=
1e-11 (asserted here; tests/test_ekf_reference_cpu.py asserts it without a GPU, with the nearest-point margins).  Error
measure: max|a - b| / max(1, max|b|), on x and on Sigma separately, after every call of the schedule.  Every case asserts
that the live handle runs the kernel its label names.  Every figure is printed before it is asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import ekf_cases as ec
import ekf_reference as er

pytestmark = pytest.mark.gpu

NOT_PD = 'innovation covariance S is not positive definite'
WORST = {}                          # path label -> [worst err x, worst err Sigma, cases]


@pytest.fixture(scope='module', autouse=True)
def worst_errors_per_path():
    yield
    for path, (ex, eS, count) in sorted(WORST.items()):
        print('\nekf_exact worst over %2d runs on path %-11s: err x %.2e Sigma %.2e' % (count, path, ex, eS), end='')
    print()


class DeviceFilter:
    """The product's DiscreteEKFObserver on a case; the explicit form and the state resets go through the C ABI."""

    def __init__(self, c):
        from sofacontrol_amd import _lib
        self.lib, self.c = _lib, c
        self.tp, self.ekf = ec.product_filter(c)

    def plan(self):
        return self.ekf.kernel_plan()

    def set_x(self, x):
        x = self.lib.f64(x)
        self.lib.check(self.lib.lib().sekf_set_state(self.ekf._h, self.lib.dptr(x), None), 'sekf_set_state')
        self.ekf.x = x.copy()

    def step(self, u, y, explicit):
        if explicit is None:
            if u is not None and y is not None:
                self.ekf.update(u, y, ec.DT)
            elif u is not None:
                self.ekf.predict_state(u, ec.DT)
            else:
                self.ekf.update_state(y)
            return
        L, f = self.lib, self.lib.f64
        A, B, d = (f(a) for a in explicit)
        u, y, x = f(u), f(y), np.empty(self.c['n'])
        L.check(L.lib().sekf_step(self.ekf._h, L.dptr(u), L.dptr(y), L.dptr(A), L.dptr(B), L.dptr(d), L.dptr(x)), 'sekf_step')
        self.ekf.x = x

    def state(self):
        n = self.c['n']
        x, S = np.empty(n), np.empty((n, n))
        self.lib.check(self.lib.lib().sekf_get_state(self.ekf._h, self.lib.dptr(x), self.lib.dptr(S)), 'sekf_get_state')
        np.testing.assert_array_equal(x, self.ekf.x)              # the estimate a step hands back is the resident one
        return x, S


def check_plan(flt, label):
    """The live handle runs the kernel the case names, with the plan sekf_plan states for its shape."""
    from sofacontrol_amd import _lib
    c, got = flt.c, flt.plan()
    want = _lib.ekf_plan(c['n'], c['ny'])
    assert got['path'] == want['path'] == ec.PATH_CODE[label], (label, got, want)
    assert got['gain_form'] == want['gain_form'] == (1 if label == 'valu' else 0)
    assert 0 < got['lds_bytes'] <= want['lds_bytes']                      # sekf_plan sizes for the largest n_u (16)


def check_case(s, label):
    c = ec.case(s)
    ref, _, e_oracle = ec.reference(s)
    tol = ec.tolerance(e_oracle)
    flt = DeviceFilter(c)
    check_plan(flt, label)
    got = ec.run(c, flt)
    check_plan(flt, label)                                        # the first predictor re-creates the filter on the dt handle
    errs = ec.errors(got, ref)
    ex, eS = max(e[0] for e in errs), max(e[1] for e in errs)
    print('ekf_exact %-32s kernel %-6s: worst err x %.2e Sigma %.2e over %d calls | e_oracle %.2e tol %.2e'
          % (ec.spec_id(s), label, ex, eS, len(errs), e_oracle, tol))
    w = WORST.setdefault(label if label == c['path'] else label + ' (no mfma)', [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], ex), max(w[1], eS), w[2] + 1
    bad = [(k, e) for k, e in zip(ec.call_steps(c), errs) if max(e) > tol]
    assert not bad, (ec.spec_id(s), tol, bad[:4])
    return got, tol


@pytest.mark.parametrize('s', ec.SPECS, ids=ec.spec_id)
def test_ekf_against_long_double(s, monkeypatch):
    """12 steps (fused, predict-only, update-only; state resets that walk over the table points) on every path, at both
    scalings of (W, V, Sigma0); one case per path on the explicit (A_d, B_d, d_d) form; (4, 3) with n_u = 8 > n_x."""
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    check_case(s, s[0])


@pytest.mark.parametrize('s', ec.NO_MFMA_SPECS, ids=ec.spec_id)
def test_ekf_valu_kernel_at_mfma_shapes(s, monkeypatch):
    """SRH_EKF_NO_MFMA=1 (read when a filter is created): the shapes of the MFMA and wide kernels on ekf_kernel, same
    tolerance -- the VALU kernel at the sizes the product uses."""
    monkeypatch.setenv('SRH_EKF_NO_MFMA', '1')
    check_case(s, 'valu')


@pytest.mark.parametrize('s', ec.LONG_SPECS, ids=ec.spec_id)
def test_ekf_200_steps_and_symmetry(s, monkeypatch):
    """200 steps: the error does not compound past the tolerance, and the device covariance -- which every MFMA path reads
    as its own transpose -- stays symmetric to the same tolerance."""
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    got, tol = check_case(s, s[0])
    steps = ec.call_steps(ec.case(s))
    worst = 0.0
    for i, (k, (x, S)) in enumerate(zip(steps, got)):
        a = er.asymmetry(S)
        worst = max(worst, a)
        last_call_of_step = i + 1 == len(steps) or steps[i + 1] != k
        if last_call_of_step and (k + 1) % 50 == 0:
            print('ekf_exact %-32s step %3d: max|Sigma - Sigma^T| / max|Sigma| = %.2e (worst so far %.2e) | tol %.2e'
                  % (ec.spec_id(s), k + 1, a, worst, tol))
    assert worst <= tol, (worst, tol)


def test_failed_step_through_the_abi_leaves_x_out_unwritten(monkeypatch):
    """sekf_step on a failed update: SRH_ENUMERIC with its message, and the caller's x_out is not written (the batched step fills it
    either way: tests/test_ekf_batch_gpu.py).  The smallest VALU shape with more than one pivot."""
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    c = ec.case(ec.spec(('valu', 4, 3, 8)))
    flt = DeviceFilter(c)
    L = flt.lib
    flt.set_x(c['resets'][0])
    flt.ekf.Sigma = ec.indefinite_sigmas(c)[0][1]
    y, x_out = L.f64(c['y'][0]), np.full(c['n'], -7.25)
    rc = L.lib().sekf_step(flt.ekf._h, None, L.dptr(y), None, None, None, L.dptr(x_out))
    msg = L.lib().srh_last_error().decode()
    print('ekf_exact failed sekf_step: rc %d, message %r, x_out %s' % (rc, msg, x_out))
    assert rc == -4 and msg == 'sekf_step: ' + NOT_PD
    np.testing.assert_array_equal(x_out, np.full(c['n'], -7.25))
    np.testing.assert_array_equal(flt.state()[0], c['resets'][0])


@pytest.mark.parametrize('shape', ec.INDEFINITE, ids=str)
def test_ekf_failure_exit_leaves_the_state_untouched(shape, monkeypatch):
    """An update whose innovation covariance is not positive definite -- at the first pivot (Sigma = -1e3 I) and at the
    last one (the long-double Cholesky fails there: tests/test_ekf_reference_cpu.py) -- is reported, leaves x and Sigma
    bit for bit as they were, and the filter goes on to the usual accuracy once a good Sigma is back."""
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    s = ec.spec(shape)
    c = ec.case(s)
    flt = DeviceFilter(c)
    check_plan(flt, shape[0])
    x0, u0, y0 = c['resets'][0], c['u'][0], c['y'][0]
    flt.set_x(x0)
    for name, Sigma, pivot in ec.indefinite_sigmas(c):
        with pytest.raises(np.linalg.LinAlgError) as info:
            er.update(c['C'], c['y_ref'], x0, Sigma, y0, c['V'])
        assert info.value.pivot == pivot and (pivot == 0 or pivot >= c['ny'] / 2)
        flt.ekf.Sigma = Sigma
        with pytest.raises(RuntimeError, match=NOT_PD):
            flt.ekf.update_state(y0)
        x, S = flt.state()
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(S, Sigma)
        print('ekf_exact %s failure exit %s (pivot %d): reported, state untouched' % (shape, name, pivot))
    flt.ekf.Sigma = c['Sigma0']
    ref, orc = ec.LongDoubleFilter(c), ec.OracleFilter(c)
    for f in (ref, orc, flt):
        f.set_x(x0)
        f.step(u0, y0, None)
    check_plan(flt, shape[0])
    (e_oracle,), (e_dev,) = ec.errors([orc.state()], [ref.state()]), ec.errors([flt.state()], [ref.state()])
    tol = ec.tolerance(max(e_oracle))
    print('ekf_exact %s fused step after the failures: err x %.2e Sigma %.2e | e_oracle %.2e tol %.2e'
          % (shape, e_dev[0], e_dev[1], max(e_oracle), tol))
    assert max(e_dev) <= tol
