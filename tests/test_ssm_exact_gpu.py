"""GPU: the SSM model kernels of csrc/ssm.hip / csrc/ssm_dev.h -- basis, analytic Jacobians, the in-kernel inverses of `be` and
`bil` on all four elimination paths of ssm::inverse_wave, observer map, reduce, rollout, and the staged LDS evaluator of the iLQR
forward pass -- through the C ABI against the long-double statement of tests/ssm_reference.py on the cases of tests/ssm_cases.py.

Tolerance rule (every comparison with the long-double reference): tol = max(100 e_oracle, 1e-13), e_oracle = the worst error of
the float64 oracle (oracle/ssm.py) against the same reference over the same points, modes and outputs, per shape (rollouts: measured
on the rollouts); input condition e_oracle <= 1e-11 (asserted here; tests/test_ssm_reference_cpu.py asserts it without a GPU).
Error measure: max|a - b| / max(1, max|b|) per point and output.  Every figure is printed before it is asserted (pytest -s).

Measured on an MI355X (worst device error over the twelve shapes, per path; e_oracle lies between 2.6e-16 and 1.3e-14):
  sssm_linearize  cont 2.1e-14 | fe 3.1e-16 | discrete map 3.7e-15
  sssm_linearize  be@0.01  EP=1 5.6e-16 | EP=2 5.7e-16 | EP=4 2.4e-15 | un-gathered loop 2.6e-15
  sssm_linearize  be@0.05  EP=1 1.0e-15 | EP=2 1.9e-15 | EP=4 2.9e-15 | un-gathered loop 9.3e-16
  sssm_linearize  bil@0.05 EP=1 2.1e-15 | EP=2 1.7e-15 | EP=4 7.6e-15 | un-gathered loop 2.7e-15
  sssm_dynamics 2.1e-15 | sssm_observe 1.7e-15 | sssm_reduce 8.1e-16 (rectangular 3.7e-16)
  sssm_rollout    fe 7.5e-16 | be@0.01 2.1e-15 | be@0.05 1.8e-15 | bil 2.1e-15 | map 3.4e-15
  staged compact  fe@0.01 3.1e-16 | be@0.01 1.4e-15 | be@0.05 1.2e-15 | bil@0.05 2.0e-15 | map 7.9e-16
  staged dense    fe@0.01 3.1e-16 | be@0.01 1.4e-15 | be@0.05 1.2e-15 | bil@0.05 2.0e-15 | map 9.0e-16
  exact case: bit-identical.  Every shape within its tolerance (1e-13 .. 1.3e-12) on the first run.
"""
import ctypes as C

import numpy as np
import pytest

import ssm_cases as sc
import ssm_reference as sr
from oracle import ssm as ossm

pytestmark = pytest.mark.gpu

WORST = {}                          # path -> [worst device error, comparisons]


@pytest.fixture(scope='module', autouse=True)
def worst_errors_per_path():
    yield
    for path, (e, count) in sorted(WORST.items()):
        print('\nssm_exact worst over %2d comparisons on path %-22s: %.2e' % (count, path, e), end='')
    print()


def record(path, e):
    w = WORST.setdefault(path, [0.0, 0])
    w[0], w[1] = max(w[0], e), w[1] + 1


_DEVICES = {}


def device(s):
    if s not in _DEVICES:
        _DEVICES[s] = sc.DeviceModel(sc.model(s))
    return _DEVICES[s]


def model_kernel_outputs(dev, X, U, Z, modes=sc.MODES, observer=True, discrete_map=True):
    got = {}
    for label, code, _, dt in modes:
        for name, v in zip('ABd', dev.linearize(X, U, code, dt)):
            got['lin/%s/%s' % (label, name)] = v
    got['dyn/cont'] = dev.dynamics(X, U, 0)
    if discrete_map:
        got['dyn/map'] = dev.dynamics(X, U, 1)
    if observer:
        z, _, _ = dev.observe(X, True, False, False)              # Z alone
        _, H, c = dev.observe(X, False, True, True)               # H and c alone
        z3, H3, c3 = dev.observe(X)                               # all three in one launch: the same numbers
        np.testing.assert_array_equal(z3, z); np.testing.assert_array_equal(H3, H); np.testing.assert_array_equal(c3, c)
        got['obs/z'], got['obs/H'], got['obs/c'] = z, H, c
    got['reduce'] = dev.reduce(Z)
    return got


@pytest.mark.parametrize('s', sc.SHAPES, ids=sc.shape_id)
def test_model_kernels_against_long_double(s):
    """sssm_linearize in continuous mode, fe, be (two steps), bil and on the discrete map, sssm_dynamics (both maps), sssm_observe
    (Z alone, H and c alone, all three) and sssm_reduce at nine points per shape."""
    ref, e_oracle, _ = sc.reference(s)
    tol = sc.tolerance(e_oracle)
    errs = sc.errors(model_kernel_outputs(device(s), *sc.points(s)), ref)
    per_path = sc.by_path(errs)
    print('ssm_exact %-14s inverse %-4s e_oracle %.2e tol %.2e | %s'
          % (sc.shape_id(s), sc.inverse_path(s[0]), e_oracle, tol, ' '.join('%s %.1e' % kv for kv in sorted(per_path.items()))))
    for p, e in per_path.items():
        record(p + (' ' + sc.inverse_path(s[0]) if '/b' in p else ''), e)
    bad = {k: e for k, e in errs.items() if not e <= tol}
    assert not bad, (sc.shape_id(s), tol, bad)


@pytest.mark.parametrize('s', sc.SHAPES, ids=sc.shape_id)
def test_rollouts_against_long_double(s):
    """sssm_rollout, N = 6 at batch 3, re-linearised at every step, in every discretisation mode, with and without Z (the state
    trajectory does not depend on whether Z is asked for)."""
    ref, e_oracle = sc.rollout_reference(s)
    tol = sc.tolerance(e_oracle)
    x0, U = sc.rollout_inputs(s)
    dev, out, bad = device(s), [], {}
    for label, code, _, dt in sc.DISCRETE:
        X, Z = dev.rollout(x0, U, code, dt)
        X2, none = dev.rollout(x0, U, code, dt, with_z=False)
        assert none is None
        np.testing.assert_array_equal(X2, X)
        ex, ez = sc.worst(X, ref[label][0]), sc.worst(Z, ref[label][1])
        out.append('%s x %.1e z %.1e' % (label, ex, ez))
        record('rollout ' + label, max(ex, ez))
        if not max(ex, ez) <= tol:
            bad[label] = (ex, ez)
    print('ssm_exact %-14s rollout e_oracle %.2e tol %.2e | %s' % (sc.shape_id(s), e_oracle, tol, ' '.join(out)))
    assert not bad, (sc.shape_id(s), tol, bad)


@pytest.mark.parametrize('s', [(2, 3, 4, 1), (10, 8, 3, 2), (17, 4, 2, 1)], ids=sc.shape_id)
def test_batch_invariance(s):
    """One workgroup owns one problem: problems 0, 64 and 129 of a 130-problem batch equal the single-problem call bit for bit, in
    every kernel."""
    n, m = s[0], s[1]
    rng = np.random.default_rng(7000 + n)
    Bn, N = 130, 3
    X, U = 0.3 * rng.standard_normal((Bn, n)), rng.standard_normal((Bn, m))
    Ur = rng.standard_normal((Bn, N, m))
    Z = sc.model(s)['z_ref'] + X
    dev = device(s)
    modes = [sc.CONT, sc.DISCRETE[2], sc.DISCRETE[3]]             # continuous, be, bil
    whole = model_kernel_outputs(dev, X, U, Z, modes)
    roll = dev.rollout(X, Ur, 2, 0.05)
    for b in (0, 64, 129):
        one = model_kernel_outputs(dev, X[b:b + 1], U[b:b + 1], Z[b:b + 1], modes)
        for k in whole:
            np.testing.assert_array_equal(one[k][0], whole[k][b], err_msg='%s problem %d' % (k, b))
        for got, want in zip(dev.rollout(X[b:b + 1], Ur[b:b + 1], 2, 0.05), roll):
            np.testing.assert_array_equal(got[0], want[b], err_msg='rollout problem %d' % b)


def test_empty_batch_is_a_no_op():
    s = (2, 3, 4, 1)
    dev, L = device(s), device(s).L
    n, m = s[0], s[1]
    x, u = np.zeros((1, n)), np.zeros((1, m))
    outs = [np.full(8, 7.25) for _ in range(3)]
    p, h, lib, zero = L.dptr, dev.h, dev.lib, C.c_int64(0)
    L.check(lib.sssm_linearize(h, p(x), p(u), zero, C.c_int(2), C.c_double(0.01), p(outs[0]), p(outs[1]), p(outs[2])), 'sssm_linearize')
    L.check(lib.sssm_dynamics(h, p(x), p(u), zero, C.c_int(0), p(outs[0])), 'sssm_dynamics')
    L.check(lib.sssm_observe(h, p(x), zero, p(outs[0]), p(outs[1]), p(outs[2])), 'sssm_observe')
    L.check(lib.sssm_reduce(h, p(x), zero, p(outs[0])), 'sssm_reduce')
    L.check(lib.sssm_rollout(h, p(x), p(u), C.c_int(1), zero, C.c_int(2), C.c_double(0.01), p(outs[0]), p(outs[1])), 'sssm_rollout')
    for o in outs:
        np.testing.assert_array_equal(o, np.full(8, 7.25))


def test_exact_case_bit_for_bit():
    """Anti-diagonal A_c, be at dt = 0.5 (tests/ssm_cases.py: exact_case): every operation is exact in binary64, so the device equals
    the long-double result bit for bit -- any row / column or pivot mix-up shows without a tolerance."""
    d, X, U, (method, code, dt) = sc.exact_case()
    M = sc.reference_model(d)
    dev = sc.DeviceModel(d)
    got = dev.linearize(X, U, code, dt)
    want = [np.array(v, dtype=np.float64) for v in zip(*[sr.jacobians(M, x, u, dt, method) for x, u in zip(X, U)])]
    for name, g, w in zip(('A_d', 'B_d', 'd_d'), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert np.abs(want[0]).max() == 0.5 and np.abs(want[1]).max() > 0        # a result with structure, not zeros
    print('ssm_exact exact case: A_d, B_d, d_d of 3 points bit-identical to the long-double result')


def test_rectangular_reduce():
    """n_x = 4, n_o = 6: sssm_reduce evaluates a six-variable basis against a 4 x 27 V; the maps that need n_x == n_o refuse."""
    d, Z, ref, e_oracle = sc.rectangular_case()
    tol = sc.tolerance(e_oracle)
    dev = sc.DeviceModel(d)
    e = sc.worst(dev.reduce(Z), ref)
    print('ssm_exact rectangular reduce (n_x 4, n_o 6): err %.2e | e_oracle %.2e tol %.2e' % (e, e_oracle, tol))
    record('reduce (rectangular)', e)
    assert e <= tol
    X = np.zeros((2, 4))
    with pytest.raises(RuntimeError, match='n_x == n_o'):
        dev.observe(X)
    with pytest.raises(RuntimeError, match='n_x == n_o'):
        dev.rollout(X, np.zeros((2, 3, 2)), 1, 0.01, with_z=True)
    Xr, _ = dev.rollout(X, np.zeros((2, 3, 2)), 1, 0.01, with_z=False)       # without Z the rollout has no use for the observer
    np.testing.assert_array_equal(Xr, np.zeros((2, 4, 4)))                   # f(0, 0) = 0


def test_singular_continuous_jacobian_is_reported():
    """A_c = diag(2 a x_1, -1) with x_1 = 0 at the middle point of three: be and bil (sep = inv(A_c) (A_d - I)) report
    SRH_ENUMERIC naming problem 1, from sssm_linearize and from sssm_rollout; fe and the continuous mode have no inverse and still
    succeed and match; the same batch without the middle point succeeds and matches."""
    from sofacontrol_amd._lib import HipError
    d, X, U = sc.singular_case()
    Mr, Mo = sc.reference_model(d), sc.oracle_model(d)
    dev = sc.DeviceModel(d)
    keep = [0, 2]

    def check(idx, label, code, method, dt):
        got = dev.linearize(X[idx], U[idx], code, dt)
        ref = [sr.jacobians(Mr, X[b], U[b], dt, method) for b in idx]
        orc = [ossm.continuous_jacobians(Mo, X[b], U[b]) if method is None else ossm.jacobians(Mo, X[b], U[b], dt, method) for b in idx]
        e_oracle = max(sr.err(o[i], r[i]) for o, r in zip(orc, ref) for i in range(3))
        e = max(sc.worst(got[i], [r[i] for r in ref]) for i in range(3))
        print('ssm_exact singular case, %s on problems %s: err %.2e | e_oracle %.2e tol %.2e' % (label, list(idx), e, e_oracle, sc.tolerance(e_oracle)))
        assert e <= sc.tolerance(e_oracle)

    for label, code, method, dt in sc.MODES[:5]:
        if method in ('be', 'bil'):
            with pytest.raises(HipError, match=r'code -4.*singular.*problem 1\b'):
                dev.linearize(X, U, code, dt)
            check(keep, label, code, method, dt)
        else:
            check([0, 1, 2], label, code, method, dt)
    Ur = np.tile(U[:, None, :], (1, 2, 1))
    with pytest.raises(HipError, match=r'code -4.*singular.*problem 1\b'):
        dev.rollout(X, Ur, 2, 0.01, with_z=False)
    Xk, _ = dev.rollout(X[keep], Ur[keep], 2, 0.01, with_z=False)
    ref = [sr.rollout(Mr, X[b], Ur[b], 0.01, 'be', with_z=False)[0] for b in keep]
    e_oracle = sc.worst([ossm.rollout(Mo, X[b], Ur[b], 0.01, 'be')[0] for b in keep], ref)
    print('ssm_exact singular case, be rollout on problems %s: err %.2e | e_oracle %.2e tol %.2e' % (keep, sc.worst(Xk, ref), e_oracle, sc.tolerance(e_oracle)))
    assert sc.worst(Xk, ref) <= sc.tolerance(e_oracle)
    Xf, _ = dev.rollout(X, Ur, 1, 0.01, with_z=False)                        # forward Euler: nothing to invert
    assert np.isfinite(Xf).all()


@pytest.mark.parametrize('s', sc.STAGED_SHAPES, ids=sc.shape_id)
def test_staged_evaluator_through_the_first_ilqr_forward_pass(s, monkeypatch):
    """ssm::stage / basis_l / jacobians_l / observe_l, which only silqr_solve_ssm reaches: with max_iter = -1 the kernel returns the
    rollout of u_warm (iters = 0 -- asserted, so that a change of the loop condition fails loudly).  Once as dispatched (compact
    derivative lists), once under SRH_SSM_DENSE_JACOBIAN=1 (read per call): each against the long-double rollout, and against each
    other to 1e-13 (their f sums are ordered differently; A, which they claim to share bit for bit, is not observable here)."""
    ref, e_oracle = sc.rollout_reference(s)
    tol = sc.tolerance(e_oracle)
    x0, U = sc.rollout_inputs(s)
    dev, out, bad = device(s), [], {}
    for label, code, _, dt in sc.DISCRETE:
        monkeypatch.delenv('SRH_SSM_DENSE_JACOBIAN', raising=False)
        xc, itc = dev.ilqr_first_forward_pass(x0, U, code, dt)
        monkeypatch.setenv('SRH_SSM_DENSE_JACOBIAN', '1')
        xd, itd = dev.ilqr_first_forward_pass(x0, U, code, dt)
        np.testing.assert_array_equal(itc, 0); np.testing.assert_array_equal(itd, 0)
        ec, ed, ecd = sc.worst(xc, ref[label][0]), sc.worst(xd, ref[label][0]), sc.worst(xc, xd)
        out.append('%s compact %.1e dense %.1e apart %.1e' % (label, ec, ed, ecd))
        record('staged compact ' + label, ec); record('staged dense ' + label, ed)
        if not (ec <= tol and ed <= tol and ecd <= 1e-13):
            bad[label] = (ec, ed, ecd)
    print('ssm_exact %-14s staged evaluator e_oracle %.2e tol %.2e | %s' % (sc.shape_id(s), e_oracle, tol, ' | '.join(out)))
    assert not bad, (sc.shape_id(s), tol, bad)
