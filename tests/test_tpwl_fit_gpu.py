"""GPU: the TPWL fit (csrc/tpwl_fit.hip, tpwl.sysid) against its long-double statement (tests/tpwl_fit_reference.py) on the seeded
cases of tests/tpwl_fit_cases.py: the assignment and the counts exactly, every element of the sums within the derived bound
(tpwl_fit_reference.sums_constant), the bits on a rerun and from device records, the tables against the long-double solution and the
generating model, the per-point status, and the hand-over to the planners.  Every figure is printed before it is asserted."""
import contextlib
import io

import numpy as np
import pytest

import tpwl_fit_cases as fc
import tpwl_fit_reference as fr

pytestmark = pytest.mark.gpu

# Recovery constant: the largest share of kappa eps |coeff|_max that the device tables used against the long-double solution of the same
# equations, measured on the MI355X over the five cases (n12 0.79, n16 0.67, n17 0.90, n77 1.25, n128 0.79),
# times 8, the margin section 41 set for shape-dependent rounding.
C_RECOVERY = 8 * 1.25

_cache = {}


def rom_info(r):
    n_f = 3 * r
    return dict(type='POD', U=np.eye(n_f)[:, :r].copy(), q_ref=np.zeros(n_f), v_ref=np.zeros(n_f))


def sysid_of(mdl):
    from sofacontrol_amd.tpwl.sysid import TPWLSysID
    return TPWLSysID(mdl['q'], mdl['v'], mdl['w'], mdl['m'], mdl['Ts'])


def fitted(name):
    """The case's records added in one call (kept for the tests that read its sums and tables)."""
    if name not in _cache:
        mdl = fc.known_model(name)
        X, U, _ = fc.records(name)
        sid = sysid_of(mdl)
        assert sid.add(X, U) == X.shape[0] * (X.shape[1] - 1)
        _cache[name] = sid
    return _cache[name]


def known_tpwl(mdl, Hf=None):
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    data = dict(q=mdl['q'], v=mdl['v'], u=mdl['u'], A_c=mdl['A_c'], B_c=mdl['B_c'], d_c=mdl['d_c'], rom_info=rom_info(mdl['r']))
    return TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights=dict(mdl['w'])), Hf=Hf, discr_method='fe')


def check_sums(sid, ref, P, what):
    """Every element of every G_p, R_p within the bound; G_p symmetric bit for bit; the counts exact.  Returns the largest share."""
    worst = 0.0
    np.testing.assert_array_equal(sid.counts(), ref['S'])
    for p in range(P):
        s = sid.sums(p)
        assert s['samples'] == ref['S'][p]
        assert np.array_equal(s['G'], s['G'].T)
        use = fr.sums_use(s['G'], s['R'], ref, p)
        q_err = abs(fr.LD(s['Q']) - ref['Q'][p])
        # |g|^2 terms: 2 roundings of g twice, at most S additions and the 256 per-thread parts' sum
        assert q_err <= (ref['S'][p] + 4 + 256) * fr.EPS * ref['Q'][p], (what, p, float(q_err))
        worst = max(worst, use)
    print('%s: the device sums use %.3f of the bound (S_p + 4) eps sum |terms|' % (what, worst))
    assert worst <= 1.0
    return worst


def sums_bits(sid, P):
    return [tuple(sid.sums(p)[k].tobytes() if k != 'Q' else sid.sums(p)[k] for k in ('G', 'R', 'Q')) for p in range(P)]


def test_assignment_and_counts_at_the_chunk_and_granule_edges():
    """Points with 0, 1, 63, 64, 65 samples (the chunk's edges), 600 (two granules) and 30, in one-sample episodes shuffled over the
    points: 1646 kept rows, two assign workgroups.  The assignment at every sample through the same search (calc_nearest_point)."""
    mdl = fc.known_model('n12')
    counts = [0, 1, 63, 64, 65, 600, 30]
    X, U = fc.counted_records(mdl, counts)
    ref = fr.sums([(X, U, 1)], mdl['q'], mdl['v'], mdl['w'], mdl['Ts'])
    print('aimed counts %r, reference counts %r, least margin %.3g' % (counts, ref['S'], ref['margin']))
    assert ref['S'] == counts and ref['margin'] >= 1e-6
    got = known_tpwl(mdl).calc_nearest_point(X[:, 0])
    np.testing.assert_array_equal(got, ref['region'])
    sid = sysid_of(mdl)
    assert sid.add(X, U) == sum(counts)
    check_sums(sid, ref, mdl['P'], 'chunk and granule edges')
    # episodes of one kept row add nothing; of two kept rows one sample each (stride 5 on rows 0 .. 5 and 0 .. 4)
    before = sums_bits(sid, mdl['P'])
    X6 = np.repeat(X[:40], 3, axis=1)                            # (40, 6, n_x): rows 0 and 5 are the episode's two states
    assert sid.add(X6[:, :5], np.repeat(U[:40], 3, axis=1)[:, :5], stride=5) == 0
    assert sums_bits(sid, mdl['P']) == before and sid.counts().tolist() == counts
    sid.reset()
    assert sid.add(X6, np.repeat(U[:40], 3, axis=1), stride=5) == 40
    ref6 = fr.sums([(X6, np.repeat(U[:40], 3, axis=1), 5)], mdl['q'], mdl['v'], mdl['w'], mdl['Ts'])
    assert sum(ref6['S']) == 40
    check_sums(sid, ref6, mdl['P'], 'two kept rows under stride 5')


def test_one_point_takes_all_a_single_point_and_a_duplicated_point():
    mdl = fc.known_model('n12')
    X, U, _ = fc.records('n12')
    # stride 5 on the case's records: 8 samples per episode
    ref5 = fr.sums([(X, U, 5)], mdl['q'], mdl['v'], mdl['w'], mdl['Ts'])
    sid = sysid_of(mdl)
    assert sid.add(X, U, stride=5) == X.shape[0] * 8 == sum(ref5['S'])
    assert ref5['margin'] >= 1e-6
    check_sums(sid, ref5, mdl['P'], 'stride 5')
    # P = 1
    one = dict(mdl, P=1, q=mdl['q'][:1], v=mdl['v'][:1])
    ref1 = fr.sums([(X, U, 1)], one['q'], one['v'], one['w'], one['Ts'])
    sid = sysid_of(one)
    sid.add(X, U)
    check_sums(sid, ref1, 1, 'P = 1')
    # the other points far away: all samples in point 3
    far = dict(mdl, q=mdl['q'] + 1e3 * (np.arange(mdl['P']) != 3)[:, None])
    reff = fr.sums([(X, U, 1)], far['q'], far['v'], far['w'], far['Ts'])
    assert reff['S'][3] == sum(reff['S']) == X.shape[0] * (X.shape[1] - 1)
    sid = sysid_of(far)
    sid.add(X, U)
    check_sums(sid, reff, mdl['P'], 'all samples in one point')
    # point 5 a copy of point 2: the first-minimum rule gives the copy no samples, and it reports status 1
    dup = dict(mdl, q=mdl['q'].copy(), v=mdl['v'].copy())
    dup['q'][5], dup['v'][5] = dup['q'][2], dup['v'][2]
    refd = fr.sums([(X, U, 1)], dup['q'], dup['v'], dup['w'], dup['Ts'])
    assert refd['S'][5] == 0 and refd['S'][2] > 0 and refd['margin'] >= 1e-6
    sid = sysid_of(dup)
    sid.add(X, U)
    check_sums(sid, refd, mdl['P'], 'a duplicated point')
    t = sid.solve_tables()
    print('duplicated point: status %r' % t['status'].tolist())
    assert t['status'][5] == 1 and t['status'][2] == 0


@pytest.mark.parametrize('name', list(fc.CASES))
def test_sums_and_their_bits(name):
    from sofacontrol_amd import _lib
    mdl = fc.known_model(name)
    X, U, _ = fc.records(name)
    ref = fc.reference(name)
    sid = fitted(name)
    check_sums(sid, ref, mdl['P'], name)
    bits = sums_bits(sid, mdl['P'])
    # the same call again: the same bits; device-resident records: the bits of host arrays
    again = sysid_of(mdl)
    again.add(X, U)
    assert sums_bits(again, mdl['P']) == bits
    dev = sysid_of(mdl)
    dX, dU = _lib.DeviceBuffer.from_array(X), _lib.DeviceBuffer.from_array(U)
    dev.add(dX, dU, shape=X.shape[:2])
    assert sums_bits(dev, mdl['P']) == bits
    # two adds against one: other chains of additions, the same bound
    two = sysid_of(mdl)
    h = X.shape[0] // 2 + 1
    two.add(X[:h], U[:h])
    two.add(X[h:], U[h:])
    check_sums(two, ref, mdl['P'], name + ' in two adds')
    print('%s: two adds give the bits of one: %r' % (name, sums_bits(two, mdl['P']) == bits))


@pytest.mark.parametrize('name', list(fc.CASES))
def test_recovery(name):
    mdl = fc.known_model(name)
    X, U, _ = fc.records(name)
    ref = fc.reference(name)
    sid = fitted(name)
    t = sid.solve_tables()
    assert not t['status'].any(), t['status']
    ld = fr.tables(ref, mdl['q'], mdl['v'], mdl['m'], range(mdl['P']))
    share_ld, share_gen = 0.0, 0.0
    for p in range(mdl['P']):
        cmax = max(float(np.abs(ld[k][p]).max()) for k in ('A_c', 'B_c', 'd_c'))
        gmax = max(float(np.abs(mdl[k][p]).max()) for k in ('A_c', 'B_c', 'd_c'))
        for k in ('A_c', 'B_c', 'd_c'):
            share_ld = max(share_ld, float(np.abs(t[k][p] - ld[k][p]).max()) / (ld['kappa'] * fr.EPS * cmax))
            share_gen = max(share_gen, float(np.abs(t[k][p] - mdl[k][p]).max()) / (ld['kappa'] * fr.EPS * max(gmax, np.abs(X).max() / mdl['Ts'])))
        # u = G[input, constant] / S: the sum's bound over S, and the division
        assert float(np.abs(t['u'][p] - np.asarray(ld['u'][p], dtype=np.float64)).max()) <= (ref['S'][p] + 5) * fr.EPS * np.abs(U).max()
    print('%s: kappa %.3g; device tables against the long-double solution: %.3g kappa eps |coeff|_max; against the generating tables: %.3g '
          'kappa eps max(|coeff|_max, |x|_max / Ts); bound %.3g' % (name, ld['kappa'], share_ld, share_gen, C_RECOVERY))
    assert share_ld <= C_RECOVERY
    assert share_gen <= C_RECOVERY
    res = sid.result(t)
    print('%s: residual rms per point %s, floors %s' % (name, np.array2string(res.residual_rms, precision=2), np.array2string(res.residual_floor, precision=2)))
    assert np.all(np.isfinite(res.residual_rms)) and np.all(res.residual_floor > 0) and res.samples == sum(ref['S'])


def test_status_per_point_and_the_refusal_of_a_row_that_is_not_finite():
    from sofacontrol_amd.tpwl.sysid import column_name
    mdl = fc.known_model('n12')
    n = 12
    # point 3 under-sampled (n + 1 = 13 needed); the counts are the reference's (the records only aim at them)
    X, U = fc.counted_records(mdl, [60, 60, 60, 5, 60, 60, 60], seed=5, jitter=0.1)
    reg = fr.nearest(X[:, 0], mdl['q'], mdl['v'], mdl['w'])[0]
    U[reg == 2, :, 1] = 0.0                                       # input u2 held at 0 over the samples of point 2: a zero column of phi
    for e in np.flatnonzero(reg == 2):
        X[e, 1] = fc.step(mdl, X[e, 0], U[e, 0])[0]
    ref = fr.sums([(X, U, 1)], mdl['q'], mdl['v'], mdl['w'], mdl['Ts'])
    counts = ref['S']
    print('counts %r, least margin %.3g' % (counts, ref['margin']))
    assert counts[3] < n + 1 and min(c for p, c in enumerate(counts) if p != 3) >= 2 * n and ref['margin'] >= 1e-6
    assert np.array_equal(fr.nearest(X[:, 0], mdl['q'], mdl['v'], mdl['w'])[0] == 2, reg == 2)
    sid = sysid_of(mdl)
    sid.add(X, U)
    t = sid.solve_tables()
    print('status %r, columns %r (%s)' % (t['status'].tolist(), t['column'].tolist(), column_name(int(t['column'][2]), 8, 3)))
    assert t['status'].tolist() == [0, 0, 2, 1, 0, 0, 0]
    assert t['column'][2] == 8 + 1 and column_name(int(t['column'][2]), 8, 3) == 'input u2' and t['column'][3] == -1
    assert not t['A_c'][2].any() and not t['A_c'][3].any()
    ok = [0, 1, 4, 5, 6]
    ld = fr.tables(ref, mdl['q'], mdl['v'], mdl['m'], ok)
    for i, p in enumerate(ok):
        cmax = max(float(np.abs(ld[k][i]).max()) for k in ('A_c', 'B_c', 'd_c'))
        for k in ('A_c', 'B_c', 'd_c'):
            assert float(np.abs(t[k][p] - ld[k][i]).max()) <= C_RECOVERY * ld['kappa'] * fr.EPS * cmax
    # ridge > 0: the rank-deficient point solves (its zero column gets the coefficient 0); min_samples = 5 lets point 3 through the
    # count, and with 5 samples for 12 unknowns only the ridge makes its pivots positive
    tr = sid.solve_tables(ridge=1e-6)
    print('ridge 1e-6: status %r' % tr['status'].tolist())
    assert tr['status'].tolist() == [0, 0, 0, 1, 0, 0, 0] and not tr['B_c'][2][:, 1].any() and tr['A_c'][2].any()
    assert sid.solve_tables(ridge=1e-6, min_samples=5)['status'].tolist() == [0] * 7
    with pytest.raises(RuntimeError, match=r'2 of 7 points did not solve .*point 2: failing pivot at input u2 .*point 3: %d samples' % counts[3]):
        sid.solve(rom_info(4))
    with contextlib.redirect_stdout(io.StringIO()):
        model = sid.solve(rom_info(4), on_fail='drop')
    assert model.num_points == 5 and sid.last_result.kept.tolist() == ok and model.discr_method == 'fe' and model.tpwl_method == 'nn'
    np.testing.assert_array_equal(np.asarray(model.tpwl_dict['q']), mdl['q'][ok])
    # a NaN row: refused with its episode and row, the sums unchanged
    before, cb = sums_bits(sid, 7), sid.counts().tolist()
    Xn = X.copy()
    Xn[17, 1, 3] = np.nan
    Xn[200, 0, 0] = np.inf
    with pytest.raises(RuntimeError, match=r'episode 17, row 1 of the records is not finite'):
        sid.add(Xn, U)
    Un = np.repeat(U, 3, axis=1)
    Un[9, 5, 2] = np.nan
    with pytest.raises(RuntimeError, match=r'episode 9, row 5 of the records is not finite'):
        sid.add(np.repeat(X, 3, axis=1), Un, stride=5)
    assert sums_bits(sid, 7) == before and sid.counts().tolist() == cb and sid.samples == sum(counts)


def test_hand_over_to_rollout_nearest_point_and_the_closed_loop():
    import scipy.sparse as sp
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    from sofacontrol_amd.tpwl.sysid import one_step_error
    name = 'n12'
    mdl = fc.known_model(name)
    r, m, Ts = mdl['r'], mdl['m'], mdl['Ts']
    X, U, _ = fc.records(name)
    ref = fc.reference(name)
    sid = fitted(name)
    Hf = sp.lil_matrix((6, 6 * r))
    for a in range(3):
        Hf[a, a] = 1.0                                            # full-order velocity and position of the first three coordinates:
        Hf[3 + a, 3 * r + a] = 1.0                                # with U = [I; 0] these are v_0..2 and q_0..2
    with contextlib.redirect_stdout(io.StringIO()):
        model = sid.solve(rom_info(r), Hf=Hf.tocsr())
        model.pre_discretize(Ts)
        known = known_tpwl(mdl, Hf=Hf.tocsr())
        known.pre_discretize(Ts)
    # the fitted model's point search is the fit's assignment
    np.testing.assert_array_equal(model.calc_nearest_point(X[:, :-1].reshape(-1, 2 * r)), ref['region'])
    # held-out episodes: one_step_error, and the rollout of one of them against the known model's
    Xh, Uh, _ = fc.records(name, seed=1)
    e_rms, e = one_step_error(model, Xh, Uh), one_step_error(model, Xh, Uh, worst=True)
    ep = 3
    T = Xh.shape[1] - 1
    xa, _ = model.rollout(Xh[ep, 0], Uh[ep, :T], Ts)
    xb, _ = known.rollout(Xh[ep, 0], Uh[ep, :T], Ts)
    # gamma: the largest norm of a product A_d(j) .. A_d(i) of the known model's Jacobians along the episode
    pts = fr.nearest(xb[:-1], mdl['q'], mdl['v'], mdl['w'], np.float64)[0]
    gamma = 1.0
    for i in range(T):
        Pr = np.eye(2 * r)
        for j in range(i, T):
            Pr = (np.eye(2 * r) + Ts * mdl['A_c'][pts[j]]) @ Pr
            gamma = max(gamma, float(np.linalg.norm(Pr, 2)))
    err = float(np.abs(xa - xb).max())
    print('held-out one-step error rms %.3g, worst %.3g; rollout of %d steps: |fitted - known| %.3g, bound T gamma e = %.3g (gamma %.3g)'
          % (e_rms, e, T, err, T * gamma * e, gamma))
    assert np.array_equal(xb[:-1], Xh[ep, :T]) or float(np.abs(xb - Xh[ep]).max()) <= 1e-9
    assert err <= T * gamma * e
    # one period of the batched closed loop with a GuSTO plan on the fitted model
    N, B, n_keep = 3, 2, 2
    gm = TPWLGuSTO(model)
    x0 = np.stack([np.concatenate([mdl['v'][0], mdl['q'][0]]) + 0.01 * b for b in range(B)])      # at and next to point 0
    u_init = np.tile(mdl['u'][0], (B, N, 1))
    x_init, _ = gm.rollout(x0, u_init, Ts)
    # (x_char, f_char stay at ones: every point of the known model is an equilibrium under its u_p, so the table's own characteristic
    # step is zero)
    Qz, R = np.diag([0, 0, 0, 100., 100., 0]), 1e-3 * np.eye(m)
    z_goal = np.asarray(model.H) @ x0[0] + np.asarray(model.z_ref) + 0.01                        # a small move of the outputs, held
    zt = np.tile(z_goal, (B, N + 1, 1))
    gusto = GuSTO(gm, N, Ts, Qz, R, x0, u_init, x_init, z=zt, convg_thresh=1e-3, batch=B, first_solve_cap=1, max_trace=0)
    loop = ClosedLoopBatch(gusto, model, Ts, n_keep, t=np.array([0.0, 1.0]), z=np.tile(z_goal, (2, 1)), max_steps_per_run=n_keep)
    loop.reset(x0)
    res = loop.run(1)
    print('closed loop: status %r, iterations %r, |u| max %.3g' % (res.status.tolist(), res.iters.tolist(), np.abs(res.u).max()))
    assert not res.status.any() and np.isfinite(res.x).all() and np.isfinite(res.u).all()


def test_points_from_records_are_the_device_kmeans_centroids_split():
    from sofacontrol_amd.mor import pod
    from sofacontrol_amd.tpwl.sysid import TPWLSysID, points_from_records
    mdl = fc.known_model('n12')
    X, U, _ = fc.records('n12')
    with contextlib.redirect_stdout(io.StringIO()):
        q, v = points_from_records(X, 7, stride=5)
        cent = pod.compute_kmeans_centroids(np.ascontiguousarray(X[:, ::5].reshape(-1, 8)), 7, n_init=10, random_state=0)
    assert q.shape == v.shape == (7, 4) and q.flags['C_CONTIGUOUS'] and np.isfinite(cent).all()
    np.testing.assert_array_equal(np.hstack([v, q]), cent)
    # the points serve a fit: the counts are the reference's
    ref = fr.sums([(X, U, 1)], q, v, mdl['w'], mdl['Ts'])
    print('k-means points: counts %r, least margin %.3g' % (ref['S'], ref['margin']))
    assert ref['margin'] >= 1e-6
    sid = TPWLSysID(q, v, mdl['w'], mdl['m'], mdl['Ts'])
    sid.add(X, U)
    np.testing.assert_array_equal(sid.counts(), ref['S'])
