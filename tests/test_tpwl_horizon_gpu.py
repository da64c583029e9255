"""GPU: the TPWL horizon error (csrc/tpwl_horizon.hip) against its definition ("TPWL horizon error").

Predictions are the rollout's bits; the curves lie within the bounds of tpwl_horizon_reference against the long-double evaluation of the
device's own predictions; end to end both lie within max(100 e_np, 1e-13) of the long-double chain, e_np the float64 restatement's own
distance from that chain in the same quantity (the rule of test_gusto_ssm_loop_tpwl_gpu.py); window arithmetic, status, ties, bits,
guards, and a fitted model's held-out episode against the 40-step rollout comparison of DESIGN.md section 47."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import tpwl_fit_cases as fc
import tpwl_fit_reference as fr
import tpwl_horizon_cases as hc
import tpwl_horizon_reference as hr

pytestmark = pytest.mark.gpu

MODES = {'n4': 'staged_held', 'n12': 'staged_held', 'n12v': 'staged', 'p65': 'staged', 'r33': 'staged', 'n84': 'staged', 'n128': 'staged',
         'n12s3': 'staged_held', 'n128l2': 'l2'}
_cache = {}


def rom_info(r):
    n_f = 3 * r
    return dict(type='POD', U=np.eye(n_f)[:, :r].copy(), q_ref=np.zeros(n_f), v_ref=np.zeros(n_f))


def tpwl_of(mdl, key=None, tables=None):
    """The TPWLATV of a case's model with the case's dense output model (one per model name; `tables` replaces the discrete tables)."""
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    key = key or mdl['name'] + repr(sorted(mdl['w'].items()))
    if key not in _cache:
        data = dict(q=mdl['q'], v=mdl['v'], u=mdl['u'], A_c=mdl['A_c'], B_c=mdl['B_c'], d_c=mdl['d_c'], rom_info=rom_info(mdl['r']))
        model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights=dict(mdl['w'])), Hf=hc.output_Hf(mdl), discr_method='fe')
        model.fit_Ts = mdl['Ts']
        if tables is not None:
            model.handle_for(mdl['Ts'], tables=tables)
        assert np.array_equal(model.H, hc.output_matrix(mdl)) and not model.z_ref.any()
        _cache[key] = model
    return _cache[key]


def device_tables(model, dt):
    A, B, d = model.discretize_batch(model._tabs[3], model._tabs[4], model._tabs[5], dt)
    return np.stack(A), np.stack(B), np.stack(d)


def rollout_of(model, ref, dt):
    """model.rollout over the windows' own start rows and input windows: (W, H + 1, n_x)."""
    return model.rollout(np.ascontiguousarray(ref['Xw'][:, 0]), np.ascontiguousarray(ref['Uw']), dt)[0]


def check_against_own_predictions(res, ref_status, Xw, Hm, n_x, n_z, wins, stride, what):
    """The curves, norms and maxima of a result against the long-double evaluation of ITS predictions; returns the shares of the bounds."""
    np.testing.assert_array_equal(res.status, ref_status)
    cv = hr.curves(res.x_pred, Xw, Hm, res.status)
    ok = cv['ok']
    assert res.windows == len(ok) and res.diverged == int((res.status == 1).sum()) and res.bad_rows == int((res.status == 2).sum())
    assert res.sse_x[0] == 0.0 and res.sse_z[0] == 0.0 and res.worst_x[0] == 0.0 and res.worst_z[0] == 0.0 if ok.any() else True
    bx, bz = hr.sse_x_bound(cv, n_x), hr.sse_z_bound(cv, n_x, n_z)
    ex, ez = np.abs(res.sse_x.astype(hr.LD) - cv['sse_x']), np.abs(res.sse_z.astype(hr.LD) - cv['sse_z'])
    assert (ex <= bx).all() and (ez <= bz).all(), (what, ex, bx, ez, bz)
    with np.errstate(all='ignore'):
        share = (float(np.nanmax(np.where(bx > 0, ex / bx, 0))), float(np.nanmax(np.where(bz > 0, ez / bz, 0))))
    W_ok = int(ok.sum())
    if W_ok:
        np.testing.assert_array_equal(res.rms_x, np.sqrt(res.sse_x / (W_ok * n_x)))
        np.testing.assert_array_equal(res.rms_z, np.sqrt(res.sse_z / (W_ok * n_z)))
    # per-window norms at k = H, NaN where the status is not 0
    assert np.isnan(res.final_x[~ok]).all() and np.isnan(res.final_z[~ok]).all()
    assert hr.norm_sq_check(res.final_x[ok], cv['sq_x'][ok, -1], hr.sq_x_bound(cv, n_x)[ok, -1]).all(), what
    assert hr.norm_sq_check(res.final_z[ok], cv['sq_z'][ok, -1], hr.sq_z_bound(cv, n_x, n_z)[ok, -1]).all(), what
    if W_ok:
        # the maxima: exact over the device's own norms at k = H, the long-double maximum to the norm's bound at every k, the window exact
        assert res.worst_x[-1] == res.final_x[ok].max() and res.worst_z[-1] == res.final_z[ok].max()
        for name, worst, at, sqb in (('x', res.worst_x, res.worst_x_at, hr.sq_x_bound(cv, n_x)), ('z', res.worst_z, res.worst_z_at, hr.sq_z_bound(cv, n_x, n_z))):
            w = cv['w' + name]
            k = np.arange(len(w))
            assert hr.norm_sq_check(worst, cv['sq_' + name][w, k], sqb[w, k]).all(), (what, name)
            if len(ok) > 1 and len(np.unique(wins, axis=0)) == len(wins):
                gap = hr.top_gap(cv['sq_' + name], ok)[1:]
                assert (gap > 1e-9).all(), (what, name, gap)                 # the case decides its maxima by more than rounding
            want = np.stack([wins[w, 0], wins[w, 1] * stride], axis=1)
            np.testing.assert_array_equal(at[1:], want[1:], err_msg='%s worst_%s_at' % (what, name))
            assert at[0, 0] == wins[np.flatnonzero(ok)[0], 0] and at[0, 1] == wins[np.flatnonzero(ok)[0], 1] * stride          # all zeros at k = 0: the first
    return share


def run_case(name):
    """(result, long-double chain, float64 restatement, model) of a case: computed once and left unchanged."""
    if ('run', name) not in _cache:
        from sofacontrol_amd.tpwl.sysid import horizon_error, horizon_plan
        c = hc.case(name)
        mdl = c['model']
        model = tpwl_of(mdl)
        tabs = device_tables(model, mdl['Ts'])
        args = (mdl['q'], mdl['v'], mdl['w'], c['X'], c['U'], c['H'], c['stride'], c['every'])
        ld, f8 = hr.predict(tabs, *args, hr.LD), hr.predict(tabs, *args, np.float64)
        plan = horizon_plan(model, c['X'].shape[0], c['X'].shape[1], c['H'], c['stride'], c['every'])
        res = horizon_error(model, c['X'], c['U'], c['H'], stride=c['stride'], every=c['every'], per_window=True, predictions=True)
        _cache[('run', name)] = (res, ld, f8, model, c, plan)
    return _cache[('run', name)]


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_predictions_are_the_rollouts_bits(name):
    res, ld, f8, model, c, plan = run_case(name)
    assert plan['mode'] == MODES[name] and plan['windows'] == ld['windows'].shape[0] == res.windows
    if name in ('n12', 'n12v', 'p65', 'n128l2'):
        assert ld['switches'] > 0                                   # region switches inside windows
    assert ld['margin'] >= 1e-6 and (ld['status'] == 0).all()
    want = rollout_of(model, ld, c['model']['Ts'])
    assert res.x_pred.shape == want.shape and np.array_equal(res.x_pred, want)
    assert np.array_equal(res.x_pred[:, 0], ld['Xw'][:, 0])


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_curves_against_the_long_double_evaluation_of_the_devices_predictions(name):
    res, ld, f8, model, c, plan = run_case(name)
    mdl = c['model']
    share = check_against_own_predictions(res, ld['status'], ld['Xw'], c['Hm'], 2 * mdl['r'], mdl['n_z'], ld['windows'], c['stride'], name)
    print('%s: sse_x uses %.3f, sse_z %.3f of their bounds' % (name, share[0], share[1]))


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_end_to_end_against_the_long_double_chain(name):
    res, ld, f8, model, c, plan = run_case(name)
    cl, c8 = hr.curves(ld['x_pred'], ld['Xw'], c['Hm'], ld['status']), hr.curves(f8['x_pred'], f8['Xw'], c['Hm'], f8['status'])
    e8 = f8['x_pred'] - f8['Xw']
    own8 = {'x_pred': f8['x_pred'], 'sse_x': (e8 * e8).sum(axis=(0, 2)), 'sse_z': ((e8 @ c['Hm'].T) ** 2).sum(axis=(0, 2))}
    refs = {'x_pred': ld['x_pred'], 'sse_x': cl['sse_x'], 'sse_z': cl['sse_z']}
    for key in ('x_pred', 'sse_x', 'sse_z'):
        scale = np.abs(refs[key]).max()
        e_np = float(np.abs(own8[key].astype(hr.LD) - refs[key]).max() / scale)
        e_dev = float(np.abs(getattr(res, key).astype(hr.LD) - refs[key]).max() / scale)
        print('%s %s: device %.2e, numpy restatement %.2e of the largest entry' % (name, key, e_dev, e_np))
        assert e_dev <= max(100 * e_np, 1e-13), (name, key, e_dev, e_np)


def n12_setup():
    mdl = hc.model('n12')
    return mdl, tpwl_of(mdl), device_tables(tpwl_of(mdl), mdl['Ts'])


def window_arithmetic_cases():
    from sofacontrol_amd.tpwl.sysid import horizon_plan
    block = 16
    # (E, T, H, stride, every, windows): s = 1 and 3 with T no multiple of s; w = 1 and w > T'; H = T' - 1; W = 1; W = block, block + 1,
    # 2 block + 1 (one episode: two and three workgroups, the last with one window); E = 1 and 5
    return block, [(5, 38, 9, 1, 1, 5 * 29), (5, 38, 4, 3, 1, 5 * 9), (5, 38, 4, 3, 2, 5 * 5), (5, 38, 9, 1, 50, 5), (5, 38, 37, 1, 1, 5), (1, 38, 12, 3, 1, 1),
                   (1, 9 + block, 9, 1, 1, block), (1, 10 + block, 9, 1, 1, block + 1), (1, 10 + 2 * block, 9, 1, 1, 2 * block + 1),
                   (5, 2 * (9 + block) + 1, 4, 2, 1, 5 * (block + 6))]


@pytest.mark.parametrize('i', range(10))
def test_window_arithmetic(i):
    from sofacontrol_amd.tpwl.sysid import horizon_error, horizon_plan
    block, cases = window_arithmetic_cases()
    E, T, H, stride, every, W = cases[i]
    mdl, model, tabs = n12_setup()
    X, U = hc.records('n12', E, T)
    plan = horizon_plan(model, E, T, H, stride, every)
    assert plan['block'] == block and plan['windows'] == W and plan['blocks'] == E * -(-(W // E) // block)
    ref = hr.predict(tabs, mdl['q'], mdl['v'], mdl['w'], X, U, H, stride, every, np.float64)
    res = horizon_error(model, X, U, H, stride=stride, every=every, per_window=True, predictions=True)
    assert res.windows == W == ref['windows'].shape[0]
    assert np.array_equal(res.x_pred, rollout_of(model, ref, mdl['Ts']))
    check_against_own_predictions(res, ref['status'], ref['Xw'], hc.output_matrix(mdl), 12, 6, ref['windows'], stride, repr(cases[i]))


def test_status_diverged_windows_and_rows_that_are_not_finite():
    from sofacontrol_amd.tpwl.sysid import horizon_error
    mdl = hc.model('n12')
    Ts, H, every = mdl['Ts'], 9, 2
    A, B, d = hr.fe_tables(mdl, Ts)
    A[0], B[0], d[0] = 1e200 * np.eye(12), 0.0, 0.0             # region 0: x -> 1e200 x, whose nearest point is 0 again (every distance inf): inf in two steps
    model = tpwl_of(mdl, key='n12-diverging', tables=(A, B, d))
    X, U = hc.records('n12', 7, 30, seed=5, uamp=1.0)            # gentle inputs: an episode stays in the region it starts in
    Hm = hc.output_matrix(mdl)
    args = (mdl['q'], mdl['v'], mdl['w'])
    ref = hr.predict((A, B, d), *args, X, U, H, 1, every, np.float64)
    assert set(ref['windows'][ref['status'] == 1][:, 0]) == {0} and (ref['status'] == 1).sum() == 11        # episode 0 starts at point 0
    assert np.abs(ref['x_pred'][ref['status'] == 0]).max() < 1e3
    res = horizon_error(model, X, U, H, every=every, per_window=True, predictions=True)
    assert res.diverged == 11 and res.bad_rows == 0 and res.windows_ok == res.windows - 11
    check_against_own_predictions(res, ref['status'], ref['Xw'], Hm, 12, 6, ref['windows'], 1, 'diverging region')
    assert np.isnan(res.x_pred[res.status == 1][:, 3:]).all() and np.isinf(res.x_pred[res.status == 1][:, 2]).any()
    # rows that are not finite reach only the windows that read them; a NaN start row that also diverges has status 2, and so has a
    # window that diverges before it reaches the row
    Xb, Ub = X.copy(), U.copy()
    Xb[3, 12, 3], Ub[5, 20, 1], Xb[0, 4, 2], Ub[6, 29, 0] = np.nan, np.inf, np.nan, np.nan          # (the last input row is read by no window)
    refb = hr.predict((A, B, d), *args, Xb, Ub, H, 1, every, np.float64)
    w = refb['windows']
    reads = lambda e, row, last: (w[:, 0] == e) & (w[:, 1] <= row) & (row <= w[:, 1] + last)
    bad = reads(3, 12, H) | reads(5, 20, H - 1) | reads(0, 4, H)
    assert bad.sum() == 5 + 5 + 3 and (refb['status'][bad] == 2).all() and (refb['status'][~bad] == ref['status'][~bad]).all()
    resb = horizon_error(model, Xb, Ub, H, every=every, per_window=True, predictions=True)
    assert resb.bad_rows == 13 and resb.diverged == 11 - 3
    check_against_own_predictions(resb, refb['status'], refb['Xw'], Hm, 12, 6, w, 1, 'bad rows')
    # the windows that read no such row are untouched, bit for bit
    assert np.array_equal(resb.x_pred[~bad], res.x_pred[~bad], equal_nan=True) and np.array_equal(resb.final_x[~bad], res.final_x[~bad], equal_nan=True)
    # no status-0 window at all: counts, NaN curves, no window named
    Xn = X[:1].copy()
    none = horizon_error(model, Xn, U[:1], H, every=every, per_window=True)
    assert none.windows == 11 == none.diverged and none.windows_ok == 0 and np.isnan(none.rms_x).all() and np.isnan(none.worst_x).all()
    assert (none.worst_x_at == -1).all() and (none.sse_x == 0).all() and (none.status == 1).all()


def test_ties_name_the_first_window():
    from sofacontrol_amd.tpwl.sysid import horizon_error
    res, ld, f8, model, c, plan = run_case('n12')
    X2, U2 = np.concatenate([c['X'], c['X']]), np.concatenate([c['U'], c['U']])
    two = horizon_error(model, X2, U2, c['H'], stride=c['stride'], every=c['every'], per_window=True)
    E = c['X'].shape[0]
    assert two.windows == 2 * res.windows
    np.testing.assert_array_equal(two.worst_x_at, res.worst_x_at)
    np.testing.assert_array_equal(two.worst_z_at, res.worst_z_at)
    assert (two.worst_x_at[:, 0] < E).all() and np.array_equal(two.worst_x, res.worst_x) and np.array_equal(two.worst_z, res.worst_z)
    assert np.array_equal(two.final_x[:res.windows], res.final_x) and np.array_equal(two.final_x[res.windows:], res.final_x)


def test_the_blocks_partial_sums_join_in_block_order():
    """A block is `block` consecutive windows of one episode.  The same windows as a call of their own are one block with the same
    order inside, hence the block's partial sums bit for bit; the whole call's sums are those partials added in block order from 0.0."""
    from sofacontrol_amd.tpwl.sysid import horizon_error, horizon_plan
    mdl, model, tabs = n12_setup()
    E, T, H, block = 3, 50, 9, 16
    X, U = hc.records('n12', E, T)
    plan = horizon_plan(model, E, T, H)
    assert plan['block'] == block and plan['windows'] == E * 41 and plan['blocks'] == E * 3         # 16 + 16 + 9 windows per episode
    whole = horizon_error(model, X, U, H)
    sx, sz = np.zeros(H + 1), np.zeros(H + 1)
    for e in range(E):
        for j0 in range(0, 41, block):
            rows = slice(j0, min(j0 + block, 41) + H)            # the rows the block's windows read
            part = horizon_error(model, X[e, rows], U[e, rows], H)
            assert part.windows == min(block, 41 - j0)
            sx, sz = sx + part.sse_x, sz + part.sse_z
    assert np.array_equal(whole.sse_x, sx) and np.array_equal(whole.sse_z, sz)
    rev = np.zeros(H + 1)                                        # (the check can tell the orders apart on this case)
    for e in reversed(range(E)):
        for j0 in reversed(range(0, 41, block)):
            rows = slice(j0, min(j0 + block, 41) + H)
            rev = rev + horizon_error(model, X[e, rows], U[e, rows], H).sse_x
    assert not np.array_equal(rev, sx)


def fields(res):
    keys = ('sse_x', 'sse_z', 'rms_x', 'rms_z', 'worst_x', 'worst_z', 'worst_x_at', 'worst_z_at', 'final_x', 'final_z', 'status', 'x_pred')
    return [getattr(res, k).tobytes() for k in keys] + [res.windows, res.diverged, res.bad_rows]


@pytest.mark.parametrize('name', ['n12', 'n12v', 'n128l2'])
def test_bits_rerun_device_records_and_an_unrelated_kernel_in_between(name):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import horizon_error
    res, ld, f8, model, c, plan = run_case(name)
    kw = dict(stride=c['stride'], every=c['every'], per_window=True, predictions=True)
    again = horizon_error(model, c['X'], c['U'], c['H'], **kw)
    assert fields(again) == fields(res)
    dX, dU = _lib.DeviceBuffer.from_array(c['X']), _lib.DeviceBuffer.from_array(c['U'])
    dev = horizon_error(model, dX, dU, c['H'], shape=c['X'].shape[:2], **kw)
    assert fields(dev) == fields(res)
    model.calc_nearest_point(c['X'][0])                          # an unrelated kernel on the stream
    model.rollout(c['X'][0, 0], c['U'][0, :3], c['model']['Ts'])
    after = horizon_error(model, dX, dU, c['H'], shape=c['X'].shape[:2], **kw)
    assert fields(after) == fields(res)
    np.testing.assert_array_equal(dX.to_array(c['X'].shape), c['X'])          # the records are read, not written
    np.testing.assert_array_equal(dU.to_array(c['U'].shape), c['U'])


@pytest.mark.parametrize('device', [False, True])
def test_every_output_lies_between_its_guards(device):
    """The unit's outputs are host arrays (nothing of size n_x stays on the device): sentinels on either side of each, the guard words
    and the sentinel of test_pod_build_exact_gpu.Guarded."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    from test_pod_build_exact_gpu import GUARD, SENTINEL
    res, ld, f8, model, c, plan = run_case('n12')
    E, T = c['X'].shape[:2]
    H, W, n = c['H'], res.windows, 12
    spec = [('sse', np.float64, 2 * (H + 1)), ('worst', np.float64, 2 * (H + 1)), ('at', np.int64, 4 * (H + 1)), ('counts', np.int64, 3),
            ('fin', np.float64, 2 * W), ('status', np.int32, W), ('pred', np.float64, W * (H + 1) * n)]
    sent = {np.float64: SENTINEL, np.int64: -(2 ** 62) + 12345, np.int32: -(2 ** 30) + 12345}
    bufs = {k: np.full(cnt + 2 * GUARD, sent[dt], dtype=dt) for k, dt, cnt in spec}
    ptrs = [C.cast(C.c_void_p(bufs[k].ctypes.data + GUARD * bufs[k].itemsize), C.POINTER({np.float64: C.c_double, np.int64: C.c_int64, np.int32: C.c_int32}[dt]))
            for k, dt, cnt in spec]
    h = model.handle_for(c['model']['Ts'])
    L = sysid._bind()
    if device:
        dX, dU = _lib.DeviceBuffer.from_array(c['X']), _lib.DeviceBuffer.from_array(c['U'])
        _lib.check(L.stpwl_horizon_error_dev(h, dX.ptr, dU.ptr, E, T, H, c['stride'], c['every'], *ptrs, None), 'stpwl_horizon_error_dev')
    else:
        _lib.check(L.stpwl_horizon_error(h, _lib.dptr(_lib.f64(c['X'])), _lib.dptr(_lib.f64(c['U'])), E, T, H, c['stride'], c['every'], *ptrs), 'stpwl_horizon_error')
    for k, dt, cnt in spec:
        assert (bufs[k][:GUARD] == sent[dt]).all() and (bufs[k][-GUARD:] == sent[dt]).all(), k
        assert not (bufs[k][GUARD:-GUARD] == sent[dt]).any(), k                   # and every entry was written
    pay = {k: bufs[k][GUARD:-GUARD] for k, _, _ in spec}
    assert np.array_equal(pay['sse'], np.concatenate([res.sse_x, res.sse_z])) and np.array_equal(pay['pred'].reshape(W, H + 1, n), res.x_pred)
    assert np.array_equal(pay['fin'], np.concatenate([res.final_x, res.final_z])) and np.array_equal(pay['status'], res.status)
    assert list(pay['counts']) == [W, 0, 0] and np.array_equal(pay['at'].reshape(2, H + 1, 2)[0], res.worst_x_at)


def test_a_handle_without_discrete_tables_is_refused():
    from sofacontrol_amd.tpwl import sysid
    res, ld, f8, model, c, plan = run_case('n12')
    L = sysid._bind()
    cnt = (C.c_int64 * 3)()
    X, U = np.ascontiguousarray(c['X']), np.ascontiguousarray(c['U'])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.stpwl_horizon_error(model.handle_for(None), dp(X), dp(U), X.shape[0], X.shape[1], c['H'], 1, 1, None, None, None, cnt, None, None, None)
    assert rc == -1 and b'stpwl_horizon_error: the handle has no discrete tables' in L.srh_last_error()


def test_fitted_model_on_a_held_out_episode_agrees_with_the_rollout_comparison():
    """The fit tests' hand-over (test_tpwl_fit_gpu.py) compares the fitted model's 40-step rollout of a held-out
    episode with the known model's within T gamma e; horizon_error is that rollout against the record itself."""
    import scipy.sparse as sp
    from sofacontrol_amd.tpwl.sysid import TPWLSysID, horizon_error, one_step_error
    mdl = fc.known_model('n12')
    r, Ts = mdl['r'], mdl['Ts']
    X, U, _ = fc.records('n12')
    Hf = sp.lil_matrix((6, 6 * r))
    for a in range(3):
        Hf[a, a] = 1.0
        Hf[3 + a, 3 * r + a] = 1.0
    sid = TPWLSysID(mdl['q'], mdl['v'], mdl['w'], mdl['m'], Ts)
    sid.add(X, U)
    with contextlib.redirect_stdout(io.StringIO()):
        model = sid.solve(rom_info(r), Hf=Hf.tocsr())
    Xh, Uh, _ = fc.records('n12', seed=1)
    ep, T = 3, Xh.shape[1] - 1
    e = one_step_error(model, Xh, Uh, worst=True)
    res = horizon_error(model, Xh[ep], Uh[ep], T, per_window=True, predictions=True)
    assert res.windows == 1 and res.status[0] == 0 and res.dt == Ts
    xa, za = model.rollout(Xh[ep, 0], Uh[ep, :T], Ts)
    assert np.array_equal(res.x_pred[0], xa)
    pts = fr.nearest(Xh[ep, :-1], mdl['q'], mdl['v'], mdl['w'], np.float64)[0]
    gamma = 1.0
    for i in range(T):
        Pr = np.eye(2 * r)
        for j in range(i, T):
            Pr = (np.eye(2 * r) + Ts * mdl['A_c'][pts[j]]) @ Pr
            gamma = max(gamma, float(np.linalg.norm(Pr, 2)))
    err = np.sqrt(((xa - Xh[ep]) ** 2).sum(axis=1))
    np.testing.assert_allclose(res.worst_x, err, rtol=1e-12, atol=0)
    np.testing.assert_allclose(res.worst_z, np.sqrt((((xa - Xh[ep]) @ model.H.T) ** 2).sum(axis=1)), rtol=1e-10, atol=1e-300)
    print('held-out episode, %d steps: worst |e_k| %.3g, bound T gamma e = %.3g (gamma %.3g, one-step e %.3g)' % (T, res.worst_x.max(), T * gamma * e, gamma, e))
    assert res.worst_x.max() <= T * gamma * e + 1e-9 and res.worst_x[-1] == res.final_x[0]
    # all held-out episodes at once: the same episode's window is among them, bit for bit
    all_ = horizon_error(model, Xh, Uh, T, per_window=True)
    assert all_.windows == Xh.shape[0] and all_.final_x[ep] == res.final_x[0] and all_.rms_x[1] <= e
