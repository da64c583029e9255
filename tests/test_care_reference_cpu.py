"""CPU: the long-double CARE reference of tests/care_reference.py is a reference on every case the GPU tests use
(tests/care_cases.py) -- per member: its certificate (a relative residual at least 30 times below that of
scipy.linalg.solve_continuous_are, a closed loop in the open left half plane) and the input condition of the tolerance rule
(e_yardstick <= 1e-11).  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import care_cases as cc
import care_reference as cr


@pytest.mark.parametrize('case', cc.ALL_CASES, ids=cc.case_id)
def test_reference_holds_its_certificate_and_the_input_condition(case):
    A, B, Q, R, members = cc.prepared(case)
    assert A.shape[0] == len(members) == (1 if case == cc.CONTROLLER else cc.MEMBERS)
    failures = []
    for k, mem in enumerate(members):
        ratio = mem['res_scipy'] / mem['res'] if mem['res'] > 0 else np.inf
        print('%s member %d: %d doubling steps, residual %.2e (scipy %.2e: %.0fx), max Re eig(A + B K) %+.3e, e_yardstick %.2e'
              % (cc.case_id(case), k, mem['steps'], mem['res'], mem['res_scipy'], ratio, mem['re_max'], mem['e_yardstick']))
        if not (cr.CERTIFICATE_RATIO * mem['res'] <= mem['res_scipy'] and mem['re_max'] < 0.0 and
                mem['e_yardstick'] <= cc.E_YARDSTICK_MAX):
            failures.append((k, mem['res'], mem['res_scipy'], mem['re_max'], mem['e_yardstick']))
        # the gain of the reference is the gain of its X, and X is symmetric
        np.testing.assert_array_equal(mem['X'], mem['X'].T)
        assert cr.err(cr.ld(B[k]) @ mem['K'], -cr.input_weight(B[k], R) @ mem['X']) <= 1e-16
    assert not failures, failures


def test_unstable_family_has_an_unstable_open_loop():
    for n, m in cc.UNSTABLE_SHAPES:
        A = cc.unstable_case(n, m)[0]
        for k in range(A.shape[0]):
            assert np.linalg.eigvals(A[k]).real.max() > 0.0


def test_fem_family_is_lightly_damped_and_stable():
    for r, m in cc.FEM_SHAPES:
        A = cc.fem_case(r, m)[0]
        for k in range(A.shape[0]):
            re = np.linalg.eigvals(A[k]).real
            assert re.max() < 0.0 and re.max() > -0.2


def test_reference_refuses_what_cannot_be_stabilised():
    """A = diag(1, -1), B = [0; 1]: the unstable mode is not controllable; the long-double recursion overflows."""
    with np.errstate(all='ignore'), pytest.raises(np.linalg.LinAlgError):
        cr.care(np.diag([1.0, -1.0]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1))
