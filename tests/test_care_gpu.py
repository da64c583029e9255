"""GPU: the continuous-time Riccati kernel (csrc/care.hip, `sric_care`) and the CLQR / StateCLQR classes on top of it, against the
long-double CARE solution of tests/care_reference.py on the cases of tests/care_cases.py.

Tolerance rule (tests/test_lqr_exact_gpu.py): tol = max(100 e_yardstick, 1e-13), e_yardstick = the error of
scipy.linalg.solve_continuous_are against the same reference on the same inputs, computed here; input condition
e_yardstick <= 1e-11 (asserted; tests/test_care_reference_cpu.py asserts the same without a GPU).  A reference is compared against
only after its certificate has been asserted (residual 30 times below scipy's, stable closed loop).  Error measure:
max|a - b| / max(1, max|b|).  Every figure is printed before it is asserted (pytest -s).

`control` / slycot, which the reference's CLQR rests on, are not installed where the golden vectors are recorded, so there is no
golden from the reference here: the pin is the stabilising CARE solution itself."""
import contextlib
import io

import numpy as np
import pytest

import care_cases as cc
import care_reference as cr
from helpers import product_tpwl

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def solve(A, B, Q, R, tol=1e-14, max_iter=100):
    """(K, P, doubling steps), stacked, straight from the entry point (care / care_batch drop the steps)."""
    from sofacontrol_amd.lqr.lqr import _dare_call
    return _dare_call('sric_care', A, B, Q, R, tol, max_iter)


def assert_certified(case, k, mem):
    assert cr.CERTIFICATE_RATIO * mem['res'] <= mem['res_scipy'] and mem['re_max'] < 0.0, (cc.case_id(case), k, mem['res'],
                                                                                          mem['res_scipy'], mem['re_max'])


_SOLVED = {}


def solved(case):
    """The batched solve of a case and the single solve of each member, once per case."""
    if case not in _SOLVED:
        A, B, Q, R, _ = cc.prepared(case)
        _SOLVED[case] = (solve(A, B, Q, R), [solve(A[k], B[k], Q, R) for k in range(A.shape[0])])
    return _SOLVED[case]


def check_against_reference(case):
    A, B, Q, R, members = cc.prepared(case)
    (Kb, Pb, itb), singles = solved(case)
    assert Kb.shape == B.transpose(0, 2, 1).shape and Pb.shape == A.shape and itb.shape == (A.shape[0],)
    failures = []
    # member 0 as a single solve, then the stack of three
    for label, k, K, P, it in [('single', 0, *(v[0] for v in singles[0]))] + [('stack', k, Kb[k], Pb[k], itb[k]) for k in range(len(members))]:
        mem = members[k]
        assert_certified(case, k, mem)
        tol = cc.tolerance(mem['e_yardstick'])
        eP, eK, eS = cr.err(P, mem['X']), cr.err(K, mem['K']), cr.err(P, P.T)
        print('care %s %s member %d: %d doubling steps (reference %d), err P %.2e K %.2e symmetry %.2e | e_yardstick %.2e tol %.2e'
              % (cc.case_id(case), label, k, int(it), mem['steps'], eP, eK, eS, mem['e_yardstick'], tol))
        if not (max(eP, eK, eS) <= tol and 1 <= int(it) <= 100):
            failures.append((label, k, int(it), eP, eK, eS, tol))
    assert not failures, failures


@pytest.mark.parametrize('case', [c for c in cc.CASES if c[0] == 'rand'], ids=cc.case_id)
def test_care_rand_against_long_double(case):
    check_against_reference(case)


@pytest.mark.parametrize('case', [c for c in cc.CASES if c[0] != 'rand'], ids=cc.case_id)
def test_care_fem_and_unstable_against_long_double(case):
    check_against_reference(case)


@pytest.mark.parametrize('case', cc.CASES, ids=cc.case_id)
def test_care_batch_members_equal_single_solves(case):
    (Kb, Pb, itb), singles = solved(case)
    for k, (K1, P1, it1) in enumerate(singles):
        assert np.array_equal(Kb[k], K1[0]) and np.array_equal(Pb[k], P1[0]) and int(itb[k]) == int(it1[0]), (cc.case_id(case), k)


def test_care_public_functions_return_the_entry_points_results():
    from sofacontrol_amd.lqr.lqr import care, care_batch
    case = ('rand', 7, 3)
    A, B, Q, R, _ = cc.prepared(case)
    (Kb, Pb, _), singles = solved(case)
    K, P = care(A[0], B[0], Q, R)
    assert K.shape == (3, 7) and P.shape == (7, 7)
    assert np.array_equal(K, singles[0][0][0]) and np.array_equal(P, singles[0][1][0])
    K2, P2 = care_batch(A, B, Q, R)
    assert np.array_equal(K2, Kb) and np.array_equal(P2, Pb)


def test_care_slot_placement_lds_against_hbm(monkeypatch):
    """(17, 9) fits the LDS slots; SRH_DARE_HBM_SLOTS=1 (read per call) moves them to the HBM workspace: same arithmetic."""
    case = ('rand', 17, 9)
    A, B, Q, R, members = cc.prepared(case)
    (Kl, Pl, itl), _ = solved(case)
    monkeypatch.setenv('SRH_DARE_HBM_SLOTS', '1')
    Kh, Ph, ith = solve(A, B, Q, R)
    monkeypatch.delenv('SRH_DARE_HBM_SLOTS')
    print('care (17, 9) LDS slots vs HBM slots: bit-identical P %s K %s steps %s' % (np.array_equal(Pl, Ph), np.array_equal(Kl, Kh),
                                                                                    np.array_equal(itl, ith)))
    for k, mem in enumerate(members):
        assert_certified(case, k, mem)
        tol = cc.tolerance(mem['e_yardstick'])
        eP, eK, ePr, eKr = cr.err(Ph[k], Pl[k]), cr.err(Kh[k], Kl[k]), cr.err(Ph[k], mem['X']), cr.err(Kh[k], mem['K'])
        print('  member %d: HBM vs LDS err P %.2e K %.2e, HBM vs reference err P %.2e K %.2e | tol %.2e' % (k, eP, eK, ePr, eKr, tol))
        assert max(eP, eK, ePr, eKr) <= tol


# ------------------------------------------------------------------------------------- refusals and numeric failures
def test_care_refuses_a_wide_input():
    with pytest.raises(RuntimeError, match='sric_care: bad dimensions'):
        solve(np.eye(2), np.ones((2, 17)), np.eye(2), np.eye(17))


def test_care_reports_an_indefinite_R():
    from sofacontrol_amd import _lib
    A, B, Q, R, _ = cc.prepared(('rand', 7, 3))
    Rbad = R.copy()
    Rbad[1, 1] = -1.0
    with pytest.raises(_lib.HipError, match=r'sric_care failed \(code -4\): sric_care: problem 0: R is not positive definite'):
        solve(A[0], B[0], Q, Rbad)


def test_care_reports_a_pair_that_cannot_be_stabilised():
    """A = diag(1, -1), B = [0; 1]: the unstable mode is not controllable -- an ordinary status return within max_iter."""
    from sofacontrol_amd import _lib
    with pytest.raises(_lib.HipError, match=r'sric_care failed \(code -4\): sric_care: problem 0: ') as info:
        solve(np.diag([1.0, -1.0]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1))
    print('unstabilisable pair:', info.value)


def test_care_reports_an_uncontrollable_mode_on_the_axis():
    """A = 0, B = [0; 1]: the mode at the origin can be moved by no gain; E_k keeps an eigenvalue of modulus 1."""
    from sofacontrol_amd import _lib
    with pytest.raises(_lib.HipError, match=r'sric_care failed \(code -4\): sric_care: problem 0: ') as info:
        solve(np.zeros((2, 2)), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1))
    print('uncontrollable mode on the axis:', info.value)


def test_care_names_the_first_failing_member_of_a_stack():
    from sofacontrol_amd import _lib
    A, B, Q, R, _ = cc.prepared(('rand', 2, 2))
    A, B = A.copy(), B.copy()
    A[1], B[1] = np.diag([1.0, -1.0]), np.array([[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(_lib.HipError, match=r'sric_care: problem 1: '):
        solve(A, B, Q, R)


# ------------------------------------------------------------------------------------- CLQR / StateCLQR
def test_clqr_and_state_clqr_on_a_product_tpwl_model():
    """StateCLQR about one point's continuous pair (as tests/test_controllers_gpu.py builds its StateDLQR): K is care's gain, A + B K
    is stable, compute_input applies u_bar + K (x - x_bar); StateDLQR on the same target keeps its own gain."""
    from sofacontrol_amd.lqr.lqr import care, CLQR, DLQR
    from sofacontrol_amd.tpwl import controllers as ctl
    from sofacontrol_amd.tpwl.tpwl_utils import DynamicsTarget
    from sofacontrol_amd.utils import QuadraticCost
    (model, U, q_ref, v_ref, Hf), point, Q, R = cc.controller_case()
    tp = product_tpwl(model, U, q_ref, v_ref, Hf)
    cost = QuadraticCost(Q=Q, R=R)
    tgt = DynamicsTarget()
    tgt.A, tgt.B = model['A_c'][point], model['B_c'][point]
    tgt.x = np.concatenate((model['v'][point], model['q'][point]))
    tgt.u = model['u'][point]
    dt = 0.02
    c = quiet(ctl.StateCLQR, tp, cost, tgt, dt=dt, delay=0.0)
    assert isinstance(c.policy, CLQR)
    K, P = care(tgt.A, tgt.B, cost.Q, cost.R)
    assert np.array_equal(np.asarray(c.K), K)
    np.testing.assert_array_equal(c.x_bar, tgt.x)
    np.testing.assert_array_equal(c.u_bar, tgt.u)
    # the gain is the stabilising one of the continuous pair, against the long-double reference and by its closed loop
    A, B, _, _, (mem,) = cc.prepared(cc.CONTROLLER)
    assert np.array_equal(A[0], tgt.A) and np.array_equal(B[0], tgt.B)
    assert_certified(cc.CONTROLLER, 0, mem)
    tol = cc.tolerance(mem['e_yardstick'])
    eP, eK = cr.err(P, mem['X']), cr.err(K, mem['K'])
    re_max = float(np.linalg.eigvals(tgt.A + tgt.B @ K).real.max())
    print('StateCLQR: err P %.2e K %.2e | tol %.2e; max Re eig(A + B K) %+.3e (open loop %+.3e)'
          % (eP, eK, tol, re_max, float(np.linalg.eigvals(tgt.A).real.max())))
    assert eP <= tol and eK <= tol and re_max < 0.0
    x = tgt.x + 1e-2 * np.random.default_rng(6).standard_normal(8)
    u = c.compute_input(0.0, x)
    np.testing.assert_array_equal(u, tgt.u + K @ (x - tgt.x))
    # StateDLQR on the same target is untouched: its policy is the discrete one, its gain that of solve_riccati on the discretised pair
    from sofacontrol_amd.lqr.lqr import solve_riccati
    d = quiet(ctl.StateDLQR, tp, cost, tgt, dt=dt, delay=0.0)
    assert type(d.policy) is DLQR
    Ad, Bd, _ = tp.discretize_dynamics(A_c=tgt.A, B_c=tgt.B, d_c=np.zeros(8), dt=dt)
    assert np.array_equal(np.asarray(d.K), solve_riccati(Ad, Bd, cost.Q, cost.R)[0])
    assert not np.array_equal(np.asarray(d.K), K)
