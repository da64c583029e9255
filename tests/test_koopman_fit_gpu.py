"""GPU: the Koopman fit of csrc/koopman_fit.hip (KoopmanSysID / fit_koopman) against the long-double statement of its definition
(tests/koopman_fit_reference.py) on the cases of tests/koopman_fit_cases.py.  Every figure is printed before it is asserted.

  sums     every element of the device's G and R within (S + 2 degree + 2) eps sum |terms| of the long-double sums; pairs exact
  solve    as a certificate on the device's own sums, |X (G + ridge I) - R|_F <= 4 n^2 eps |X|_F |G + ridge I|_F, on the iid cases and on a
           smooth (ill-conditioned) trajectory; forward on the iid cases: A and B within max(100 e_oracle, 1e-13) of long double
  and      bit-identical reruns, two adds against one, device pointers against host arrays, recovery of a linear system, a
           rank-deficient G with and without ridge, a NaN record, the computed scaling, and the model through KoopmanClosedLoopBatch."""
import numpy as np
import pytest

import koopman_fit_cases as kc
import koopman_fit_reference as kr

pytestmark = pytest.mark.gpu

SOLVE = [c for c in kc.CASES if c[1] == 'solve']
_cache = {}


def sysid_of(c, scale='case'):
    from sofacontrol_amd.baselines.koopman.sysid import KoopmanSysID
    return KoopmanSysID(c['n_y'], c['m'], 0.05, obs_degree=c['degree'], delays=c['delays'], DMD=c['dmd'],
                        scale=c['scale'] if scale == 'case' else scale)


def run(c, scale='case'):
    sid = sysid_of(c, scale)
    for Y, U in c['adds']:
        sid.add(Y, U, stride=c['stride'], u_lag=c['u_lag'])
    return sid


def device(case):
    """(KoopmanSysID, sums) of a case, computed once."""
    if case not in _cache:
        sid = run(kc.records(case))
        _cache[case] = (sid, sid.sums())
    return _cache[case]


@pytest.mark.parametrize('case', kc.CASES, ids=kc.case_id)
def test_sums(case):
    """The device uses 0.17 to 0.71 of the bound on the one-pair cases (0.31 at degree 3) and at most 0.30 on every other, the figures of
    the float64 statement: the kernel rounds a scaled sample once, as that statement does (tests/test_koopman_fit_reference_cpu.py has
    the count of roundings, and what the bound covers as a worst case)."""
    c = kc.records(case)
    ref = kc.reference(case, kr.LD)
    sid, got = device(case)
    use = kr.sums_use(got['G'], got['R'], ref, c['degree'])
    q = abs(got['Q'] - float(ref['Q'])) / max(1.0, float(ref['Q']))
    print('%s: pairs %d (expected %d), device uses %.3g of the sums bound, Q off by %.2e' % (kc.case_id(case), got['pairs'], ref['pairs'], use, q))
    assert got['pairs'] == sid.pairs == ref['pairs'] == kc.expected_pairs(case)
    np.testing.assert_array_equal(got['G'], got['G'].T)
    assert use <= 1.0
    # Q's terms are all positive, so the bound is relative to Q: a term passes through at most S additions in its thread, 768 over the
    # workgroups and 256 over the threads, and carries 4 degree roundings of its own (2 degree of the scaled samples, 2 degree of products)
    assert abs(got['Q'] - float(ref['Q'])) <= (ref['pairs'] + 1024 + 4 * c['degree']) * kr.EPS * float(ref['Q'])


@pytest.mark.parametrize('case', SOLVE, ids=kc.case_id)
def test_solve_certificate_and_forward(case):
    sid, got = device(case)
    A, B = sid.solve_AB(0.0)
    res, bound = kr.certificate(np.hstack([A, B]), got['G'], got['R'], 0.0)
    Ar, Br = kc.model_reference(case, kr.LD)
    e = kc.e_oracle(case)
    tol = kr.tolerance(e)
    ea, eb = kr.err(A, Ar), kr.err(B, Br)
    print('%s: certificate %.3e of %.3e; e_oracle %.3e, tolerance %.3e, device A %.3e, B %.3e' % (kc.case_id(case), res, bound, e, tol, ea, eb))
    assert e <= kr.E_ORACLE_MAX
    assert res <= bound
    assert ea <= tol and eb <= tol


def test_certificate_on_the_smooth_trajectory():
    c = kc.smooth_case()
    sid = run(c, scale=None)
    got = sid.sums()
    A, B = sid.solve_AB(0.0)
    res, bound = kr.certificate(np.hstack([A, B]), got['G'], got['R'], 0.0)
    print('smooth: pairs %d, cond(G) %.2e, certificate %.3e of %.3e' % (got['pairs'], np.linalg.cond(got['G']), res, bound))
    assert got['pairs'] == 600
    assert res <= bound


def test_two_runs_are_bit_identical():
    for case in (((3, 4, 1, 2, False), 'E3-unaligned'), ((14, 8, 0, 2, False), 'solve')):
        a, b = run(kc.records(case)), run(kc.records(case))
        sa, sb = a.sums(), b.sums()
        for k in ('G', 'R'):
            np.testing.assert_array_equal(sa[k], sb[k])
        assert sa['Q'] == sb['Q'] and sa['pairs'] == sb['pairs']
        if case[1] == 'solve':
            for x, y in zip(a.solve_AB(1e-9), b.solve_AB(1e-9)):
                np.testing.assert_array_equal(x, y)
        # reset brings the sums back to zero, and the same records then give the same bits again
        a.reset()
        assert a.pairs == 0 and not a.sums()['G'].any()
        for Y, U in kc.records(case)['adds']:
            a.add(Y, U, stride=kc.records(case)['stride'], u_lag=kc.records(case)['u_lag'])
        np.testing.assert_array_equal(a.sums()['R'], sb['R'])


@pytest.mark.parametrize('shape', list(kc.SHAPES), ids=lambda s: '%d-%d-%d-%d-%s' % (s[:4] + ('dmd' if s[4] else 'const',)))
def test_two_adds_equal_one(shape):
    (_, two), (_, one) = device((shape, 'two-adds')), device((shape, 'one-add'))
    ref = kc.reference((shape, 'one-add'), kr.LD)
    use = kr.sums_use(two['G'], two['R'], ref, shape[3])
    d = max(np.abs(two[k] - one[k]).max() for k in ('G', 'R'))
    print('%s: two adds use %.3g of the sums bound, largest difference from one add %.2e' % (shape, use, d))
    assert two['pairs'] == one['pairs'] == 120
    assert use <= 1.0


def test_device_pointers_give_the_bits_of_host_arrays():
    from sofacontrol_amd import _lib
    case = ((3, 4, 1, 2, False), 'stride3-lag1')
    c = kc.records(case)
    _, host = device(case)
    sid = sysid_of(c)
    bufs = []
    for Y, U in c['adds']:
        dy, du = _lib.DeviceBuffer.from_array(Y), _lib.DeviceBuffer.from_array(U)
        bufs += [dy, du]
        sid.add(dy, du, stride=c['stride'], u_lag=c['u_lag'], shape=Y.shape[:2])
    got = sid.sums()
    for k in ('G', 'R'):
        np.testing.assert_array_equal(got[k], host[k])
    assert got['Q'] == host['Q'] and got['pairs'] == host['pairs']
    # the scale from device records is the scale from host records
    from sofacontrol_amd.baselines.koopman.sysid import KoopmanSysID
    a, b = KoopmanSysID(3, 4, 0.05), KoopmanSysID(3, 4, 0.05)
    Y, U = c['adds'][0]
    a.add(Y, U, stride=3, u_lag=1)
    b.add(bufs[0], bufs[1], stride=3, u_lag=1, shape=Y.shape[:2])
    for k in a.scale:
        np.testing.assert_array_equal(a.scale[k], b.scale[k])
    np.testing.assert_array_equal(a.sums()['G'], b.sums()['G'])


@pytest.mark.parametrize('dmd', [True, False])
def test_recovery_of_a_linear_system(dmd):
    from sofacontrol_amd.baselines.koopman.sysid import fit_koopman
    c = kc.linear_case(dmd)
    Y, U = c['adds'][0]
    model, res = fit_koopman(Y, U, 0.05, obs_degree=1, delays=0, DMD=dmd, scale=c['scale'])
    ny = c['n_y']
    Ar, Br, _ = kr.fit(c['adds'], c['scale'], 0, 1, dmd, 1, 0, 0.0, kr.LD)
    a64, b64, _ = kr.fit(c['adds'], c['scale'], 0, 1, dmd, 1, 0, 0.0, np.float64)
    e = max(kr.err(a64, Ar), kr.err(b64, Br))
    tol = kr.tolerance(e)
    ea, eb = kr.err(model.A_d[:ny, :ny], c['A0']), kr.err(model.B_d[:ny], c['B0'])
    print('linear (dmd %s): pairs %d, e_oracle %.3e, tolerance %.3e, A0 off by %.3e, B0 by %.3e, residual rms %.2e' % (dmd, res.pairs, e, tol, ea, eb,
                                                                                                               res.residual_rms))
    assert res.pairs == 2 * 59 and e <= kr.E_ORACLE_MAX
    assert ea <= tol and eb <= tol
    np.testing.assert_array_equal(model.C, np.eye(ny, ny + (0 if dmd else 1)))
    assert model.M is None and model.K is None
    if not dmd:
        want = np.zeros(ny + 1)
        want[ny] = 1.0
        ec = max(kr.err(model.A_d[ny], want), kr.err(model.A_d[:ny, ny], np.zeros(ny)), kr.err(model.B_d[ny], np.zeros(c['m'])))
        print('  the constant\'s row and column off by %.3e' % ec)
        assert ec <= tol


def test_rank_deficient_needs_ridge():
    from sofacontrol_amd import _lib
    shape = (3, 4, 1, 2, False)                           # n = 70 on 50 pairs
    sid, got = device((shape, 'empty-between'))
    assert got['pairs'] == 50 < kc.SHAPES[shape]
    with pytest.raises(_lib.HipError, match=r'pivot (\d+) of G \+ ridge I .* increase ridge') as exc:
        sid.solve(0.0)
    print('rank deficient: %s (info %d)' % (exc.value, sid.last_info))
    assert 0 <= sid.last_info < 70 and ('pivot %d ' % sid.last_info) in str(exc.value)
    A, B = sid.solve_AB(1e-3)
    res, bound = kr.certificate(np.hstack([A, B]), got['G'], got['R'], 1e-3)
    print('  with ridge 1e-3: certificate %.3e of %.3e' % (res, bound))
    assert sid.last_info == -1 and res <= bound


def test_a_nan_record_is_reported():
    from sofacontrol_amd import _lib
    case = ((4, 2, 0, 2, False), 'solve')
    c = kc.records(case)
    for where in ('y', 'u', 'last-y'):
        Y, U = (a.copy() for a in c['adds'][0])
        if where == 'y':
            Y[1, 7, 2] = np.nan
        elif where == 'u':
            U[2, 11, 1] = np.nan
        else:
            Y[0, -1, 0] = np.nan                            # the last row of an episode reaches R alone
        sid = sysid_of(c)
        sid.add(Y, U)
        with pytest.raises(_lib.HipError, match='skoop_fit_solve'):
            sid.solve(0.0)
        print('NaN in %s: info %d' % (where, sid.last_info))
        assert sid.last_info >= 0


def test_computed_scaling_is_numpys():
    rng = np.random.default_rng(4800)
    E, T, ny, m = 3, 50, 3, 4
    Y, U = rng.uniform(-3.0, 5.0, (E, T, ny)), rng.uniform(0.0, 100.0, (E, T, m))
    from sofacontrol_amd.baselines.koopman.sysid import KoopmanSysID
    for stride in (1, 3):
        sid = KoopmanSysID(ny, m, 0.05)
        sid.add(Y, U, stride=stride)
        want = kr.scale_from([(Y, U)], stride)
        for k, v in want.items():
            np.testing.assert_array_equal(np.ravel(sid.scale[k]), v)
    Yc = Y.copy()
    Yc[:, :, 1] = 0.25
    with pytest.raises(RuntimeError, match=r'channel y\[1\] is constant'):
        KoopmanSysID(ny, m, 0.05).add(Yc, U)


def test_fitted_model_closes_the_batched_loop():
    """The model object is complete: KoopmanClosedLoopBatch takes it for two periods at B = 2 on the small plant of cl_cases."""
    import cl_cases as cc
    import koopman_loop_cases as klc
    from test_koopman_loop_gpu import plant
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.baselines.koopman.sysid import fit_koopman, one_step_error
    from sofacontrol_amd.utils import QuadraticCost
    mname, ny, B = 'g6', 2, 2
    m = cc.MODELS[mname][1]
    Cm, y_ref = klc.measurement(mname, ny, 1)
    rng = np.random.default_rng(4700)
    U = rng.uniform(0.0, 60.0, (4, 80, m))
    Y = y_ref + np.cumsum(0.02 * rng.standard_normal((4, 80, ny)), axis=1)
    model, res = fit_koopman(Y, U, klc.TS, obs_degree=2, delays=1, u_lag=1, ridge=1e-6)
    print('loop model: %r, one-step error on its own records %.3e' % (res, one_step_error(model, Y, U, u_lag=1)))
    assert model.A_d.shape == (36, 36) and model.B_d.shape == (36, m) and np.isfinite(model.A_d).all()
    cost = QuadraticCost(Q=np.eye(ny), R=1e-3 * np.eye(m))
    cl = KoopmanClosedLoopBatch(model, klc.N, cost, plant(mname), Cm, y_ref, klc.DT_SIM[5], 1, batch=B, u0=np.full(m, 30.0))
    base = cc.advance_case(('fit-loop', mname, B, klc.DT_SIM[5], 5, False, False, 71))
    cl.reset(x0=base['x'], y_hist=np.tile(y_ref, (B, 1, 1)), u_hist=np.full((B, 1, m), 30.0), u_prev0=np.full((B, m), 30.0))
    out = cl.run(2)
    print('  status %s, iters %s' % (np.ravel(out.status), np.ravel(out.iters)))
    for f in ('x', 'y', 'u', 'x_lift', 'J'):
        assert np.isfinite(getattr(out, f)).all(), f
