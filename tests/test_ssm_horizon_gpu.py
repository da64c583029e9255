"""GPU: the SSM horizon error (csrc/ssm_horizon.hip) against its definition ("SSM horizon error").

Predictions are the bits of the SSM closed loop's plant step (sgusto_ssm_loop_advance); the curves lie within the bounds of
ssm_horizon_reference against the long-double evaluation of the device's own predictions; end to end everything lies within
ssm_cases.tolerance(e_np) = max(100 e_np, 1e-13) of the long-double chain, e_np the float64 restatement's own distance from that chain in
the same quantity; the reference's model check on its shipped model and record (golden g17); window arithmetic, bits, status, guards.
Every case's references are computed once (ssm_horizon_cases.reference) and left unchanged."""
import numpy as np
import pytest

import cl_cases as cc
import ssm_cases as sc
import ssm_horizon_cases as shc
import ssm_horizon_reference as shr

pytestmark = pytest.mark.gpu

_cache = {}


def _mat(v):
    a = np.empty((1, 1), dtype=object)
    a[0, 0] = np.asarray(v)
    return a


def product(d, method, key=None):
    """The SSMDynamics of a model dict (the layout of ssm_cases.model) in a mode: 'map' is the discrete map, else the discr_method."""
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    key = key or (id(d), method)
    if key not in _cache:
        s = lambda v: _mat(np.array([[v]]))
        params = dict(state_dim=s(d['n']), input_dim=s(d['m']), output_dim=s(d['n_o']), SSM_order=s(d['ssm_order']), ROM_order=s(d['rom_order']))
        mdl = dict(Ts=s(0.01), w_coeff=_mat(d['W']), v_coeff=_mat(d['V']), r_coeff=_mat(d['R']), B=_mat(d['B']), rd_coeff=_mat(d['Rd']),
                   Bd=_mat(d['Bd']))
        kw = dict(discrete=True, discr_method='be') if method == 'map' else dict(discrete=False, discr_method=method)
        _cache[key] = (SSMDynamics(np.asarray(d['z_ref'], dtype=np.float64).copy(), model=mdl, params=params, **kw), d)      # (d kept: its id is the key)
    return _cache[key][0]


def run_case(name, label):
    """(result, long-double chain, float64 restatement, model, case) of a case in a mode: computed once and left unchanged."""
    if ('run', name, label) not in _cache:
        from sofacontrol_amd.SSM.sysid import horizon_error, horizon_plan
        c = shc.case(name)
        _, _, method, dt = shc.MODES[label]
        model = product(c['d'], method)
        ld, f8 = shc.reference(name, label)
        plan = horizon_plan(model, c['Y'].shape[0], c['Y'].shape[1], c['H'], c['stride'], c['every'])
        res = horizon_error(model, c['Y'], c['U'], c['H'], dt=dt, stride=c['stride'], every=c['every'], per_window=True, predictions=True)
        _cache[('run', name, label)] = (res, ld, f8, model, c, plan)
    return _cache[('run', name, label)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. the loop's bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('label', [m[0] for m in sc.DISCRETE])
@pytest.mark.parametrize('name', ['m-n5-m5-r3-s3', 'm-n9-m4-r2-s2', 'm-shipped'])
def test_predictions_are_the_loops_plant_step_bit_for_bit(name, label):
    from sofacontrol_amd.scp.closed_loop_ssm import advance
    from sofacontrol_amd.SSM.sysid import horizon_error
    c = shc.case(name)
    method, H, dt = shc.MODES[label][2], c['H'], 2.0 ** -6
    model = product(c['d'], method)
    res = horizon_error(model, c['Y'], c['U'], H, dt=dt, stride=c['stride'], every=c['every'], per_window=True, predictions=True)
    assert (res.status == 0).all()
    wins = shr.windows(c['Y'].shape[0], c['Y'].shape[1], H, c['stride'], c['every'])
    _, Uw, _ = shr.gather(c['Y'][:, ::c['stride']], c['U'][:, ::c['stride']], res.x_obs, wins, H)
    _, _, j, theta = cc.direct_schedule(H, dt, dt, H, 0.0, 0)
    assert list(j) == list(range(H)) and not np.any(theta)              # sub-step s reads plan interval s at its start: u = uopt[s]
    out = advance(model, model, dt, H, j, theta, np.ascontiguousarray(Uw), np.ascontiguousarray(res.x_pred[:, 0]))
    assert same_bits(res.x_pred[:, 1:], out['X']), (name, label, np.abs(res.x_pred[:, 1:] - out['X']).max())
    assert same_bits(res.z_pred[:, 1:], out['Z'] + model.z_ref), (name, label)
    assert same_bits(res.x_pred[:, 0], res.x_obs[wins[:, 0], wins[:, 1]])
    # THE ESTIMATE: the loop's measurement record read as records gives the loop's Xhat record as x_obs (ssm_step_estimate of
    # csrc/ssm_step_dev.h against ssm_loop_estimate of csrc/gusto_ssm_loop.hip)
    again = horizon_error(model, out['Y'], np.zeros(out['U'].shape), 1, dt=dt, predictions=True)
    assert same_bits(again.x_obs, out['Xhat']), (name, label)


# ---- 2. the curves against the device's own predictions -------------------------------------------------------------------------

def check_against_own_predictions(res, ref_status, Yw, wins, stride, n, what, x_start=False, linear=False):
    np.testing.assert_array_equal(res.status, ref_status)
    Xow = res.x_obs[wins[:, :1], wins[:, 1:2] + np.arange(res.horizon + 1)[None]]
    cv = shr.curves(res.x_pred, res.z_pred, Xow, Yw, res.status)
    ok = cv['ok']
    W_ok = int(ok.sum())
    assert res.windows == len(ok) and res.diverged == int((res.status == 1).sum()) and res.bad_rows == int((res.status == 2).sum())
    if W_ok and not x_start:
        assert res.sse_x[0] == 0.0 and res.worst_x[0] == 0.0
    share = {}
    for key in ('x', 'z'):
        sse, worst, at = getattr(res, 'sse_' + key), getattr(res, 'worst_' + key), getattr(res, 'worst_%s_at' % key)
        fin = getattr(res, 'final_' + key)
        err, bound = np.abs(sse.astype(shr.LD) - cv['sse_' + key]), shr.sse_bound(cv['sse_' + key], n, W_ok)
        assert (err <= bound).all(), (what, key, err, bound)
        with np.errstate(all='ignore'):
            share[key] = float(np.nanmax(np.where(bound > 0, err / bound, 0)))
        sqb = shr.sse_bound(cv['sq_' + key], n, 1)
        assert np.isnan(fin[~ok]).all()
        assert shr.norm_sq_check(fin[ok], cv['sq_' + key][ok, -1], sqb[ok, -1]).all(), (what, key)
        if not W_ok:
            assert np.isnan(worst).all() and (at == -1).all() and np.isnan(getattr(res, 'rms_' + key)).all()
            continue
        np.testing.assert_array_equal(getattr(res, 'rms_' + key), np.sqrt(sse / (W_ok * n)))
        assert worst[-1] == fin[ok].max()
        w = cv['w' + key]
        k = np.arange(len(w))
        assert shr.norm_sq_check(worst, cv['sq_' + key][w, k], sqb[w, k]).all(), (what, key)
        # the window of the maximum, exact: row 0 of x is all zeros (the first window), row 0 of z under a linear chart is rounding alone
        first = 1 if (key == 'x' and not x_start) or (key == 'z' and linear) else 0
        want = np.stack([wins[w, 0], wins[w, 1] * stride], axis=1)
        np.testing.assert_array_equal(at[first:], want[first:], err_msg='%s worst_%s_at' % (what, key))
        if key == 'x' and not x_start:
            i0 = np.flatnonzero(ok)[0]
            assert at[0, 0] == wins[i0, 0] and at[0, 1] == wins[i0, 1] * stride
    return share


@pytest.mark.parametrize('name,label', shc.case_modes())
def test_curves_against_the_long_double_evaluation_of_the_devices_predictions(name, label):
    res, ld, f8, model, c, plan = run_case(name, label)
    assert plan['block'] == shc.BLOCK and plan['windows'] == len(ld['status']) == res.windows
    share = check_against_own_predictions(res, ld['status'], ld['Yw'], ld['windows'], c['stride'], c['d']['n'], (name, label), linear=shc.linear_chart(name))
    print('%s %s: sse_x uses %.3f, sse_z %.3f of their bounds' % (name, label, share['x'], share['z']))


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,label', shc.case_modes())
def test_end_to_end_against_the_long_double_chain(name, label):
    res, ld, f8, model, c, plan = run_case(name, label)
    e_np, ref = shc.e_np(ld, f8)
    for key in ('x_obs', 'x_pred', 'z_pred', 'sse_x', 'sse_z'):
        e_dev = shr.rel_err(getattr(res, key), ref[key])
        print('%s %s %s: device %.2e, numpy restatement %.2e of the largest entry' % (name, label, key, e_dev, e_np[key]))
        assert e_dev <= sc.tolerance(e_np[key]), (name, label, key, e_dev, e_np[key])


# ---- 4. the reference's model check ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['discrete', 'be', 'fe'])
def test_the_references_model_check_on_its_shipped_model(tag):
    """examples/hardware/diamond_SSM.py module_test: p0 = zeros, the 1002 recorded inputs, the MSE against the recorded outputs (golden g17
    holds the data and what the imported reference computes).  1e-8 is the figure tests/test_ssm_gpu.py holds SSM.rollout to on this data."""
    from sofacontrol_amd.SSM.sysid import horizon_error
    g, d = shc.golden(), shc.model(shc.SHIPPED)
    model = product(d, 'map' if tag == 'discrete' else tag)
    Y, U = g['z_true_qv'][None], g['u_interp'][None]
    res = horizon_error(model, Y, U, 1001, dt=float(g['dt']), x_start=np.zeros(6), per_window=True, predictions=True)
    assert res.windows == 1 and res.status[0] == 0
    p, z = g[tag + '_p'][:-1], g[tag + '_z'][:-1]
    ex, ez = float(np.abs(res.x_pred[0] - p).max() / max(1.0, np.abs(p).max())), float(np.abs(res.z_pred[0] - z).max() / max(1.0, np.abs(z).max()))
    mse = res.sse_z.sum() / 1002
    xr, zr = model.rollout(np.zeros(6), g['u_interp'], float(g['dt']))
    print('%s: staged route x_pred %.2e, z_pred %.2e, mse rel %.2e; SSM.rollout x %.2e, z %.2e' % (
        tag, ex, ez, abs(mse / float(g[tag + '_mse']) - 1), np.abs(xr - g[tag + '_p']).max() / max(1.0, np.abs(p).max()),
        np.abs(zr - g[tag + '_z']).max() / max(1.0, np.abs(z).max())))
    assert ex <= 1e-8 and ez <= 1e-8
    assert mse == pytest.approx(float(g[tag + '_mse']), rel=1e-8)


# ---- 5. window arithmetic and bits ----------------------------------------------------------------------------------------------

def test_the_same_window_has_the_same_bits_alone_inside_a_block_and_across_every():
    from sofacontrol_amd.SSM.sysid import horizon_error
    c = shc.case('w2')
    model, H = product(c['d'], 'bil'), c['H']
    runs = {w: horizon_error(model, c['Y'], c['U'], H, dt=0.05, every=w, per_window=True, predictions=True) for w in (1, 2, 5)}
    assert runs[1].windows == 26 and runs[2].windows == 13 and runs[5].windows == 6           # every = 1: two blocks
    for w in (2, 5):
        pick = np.arange(runs[w].windows) * w
        for f in ('x_pred', 'z_pred', 'final_x', 'final_z'):
            assert same_bits(getattr(runs[w], f), getattr(runs[1], f)[pick]), (w, f)
        assert same_bits(runs[w].x_obs, runs[1].x_obs)
    for j0 in (0, 15, 16, 25):                                     # alone: the record cut to the window's own rows
        one = horizon_error(model, c['Y'][:, j0:j0 + H + 1], c['U'][:, j0:j0 + H + 1], H, dt=0.05, per_window=True, predictions=True)
        assert one.windows == 1
        for f in ('x_pred', 'z_pred', 'final_x', 'final_z'):
            assert same_bits(getattr(one, f)[0], getattr(runs[1], f)[j0]), (j0, f)
        assert np.sqrt(one.sse_x[-1]) == runs[1].final_x[j0] and np.sqrt(one.sse_z[-1]) == runs[1].final_z[j0]       # one window: its own squares
        assert one.worst_x[-1] == runs[1].final_x[j0] and one.worst_z[-1] == runs[1].final_z[j0]


def test_a_rerun_and_device_records_give_the_same_bits():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.SSM.sysid import horizon_error
    res, ld, f8, model, c, plan = run_case('e3-b17', 'be@0.01')
    kw = dict(dt=0.01, stride=c['stride'], every=c['every'], per_window=True, predictions=True)
    again = horizon_error(model, c['Y'], c['U'], c['H'], **kw)
    dY, dU = _lib.DeviceBuffer.from_array(np.ascontiguousarray(c['Y'])), _lib.DeviceBuffer.from_array(np.ascontiguousarray(c['U']))
    dev = horizon_error(model, dY, dU, c['H'], shape=c['Y'].shape[:2], **kw)
    for other in (again, dev):
        for f in ('sse_x', 'sse_z', 'worst_x', 'worst_z', 'rms_x', 'rms_z', 'final_x', 'final_z', 'x_pred', 'z_pred', 'x_obs'):
            assert same_bits(getattr(other, f), getattr(res, f)), f
        for f in ('worst_x_at', 'worst_z_at', 'status'):
            np.testing.assert_array_equal(getattr(other, f), getattr(res, f))


def test_three_episodes_equal_the_three_run_alone():
    from sofacontrol_amd.SSM.sysid import horizon_error
    res, ld, f8, model, c, plan = run_case('e3-b17', 'be@0.01')
    assert plan['blocks'] == 6 and res.windows == 51
    kw = dict(dt=0.01, per_window=True, predictions=True)
    parts = [horizon_error(model, c['Y'][e], c['U'][e], c['H'], **kw) for e in range(3)]
    assert sum(p.windows for p in parts) == res.windows and sum(p.windows_ok for p in parts) == res.windows_ok
    for f in ('final_x', 'final_z', 'x_pred', 'z_pred', 'status'):
        assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(res, f)), f
    assert same_bits(np.concatenate([p.x_obs for p in parts]), res.x_obs)
    for key in ('x', 'z'):
        np.testing.assert_array_equal(getattr(res, 'worst_' + key), np.max([getattr(p, 'worst_' + key) for p in parts], axis=0))


def test_stride_rows_and_the_single_window_episodes():
    res, ld, f8, model, c, plan = run_case('s3', 'fe@0.01')
    assert res.windows == 2 * 9 and (res.worst_x_at[:, 1] % 3 == 0).all() and res.x_obs.shape == (2, 13, 5)
    res, ld, f8, model, c, plan = run_case('e3-one', 'map')
    assert res.windows == 3 and plan['blocks'] == 3 and (res.worst_z_at[:, 1] == 0).all()
    res, ld, f8, model, c, plan = run_case('h1', 'be@0.05')
    assert res.horizon == 1 and res.sse_x.shape == (2,) and res.windows == 2 * 5


# ---- 6. status ------------------------------------------------------------------------------------------------------------------

def test_bad_rows_affect_exactly_the_windows_that_read_them():
    from sofacontrol_amd.SSM.sysid import horizon_error
    c = shc.case('e3-b17')
    model, H = product(c['d'], 'be'), c['H']
    Y, U = c['Y'].copy(), c['U'].copy()
    Y[0, 5, 1], U[1, 7, 0], U[2, 19, 2] = np.nan, np.inf, np.nan                     # (the last input row of an episode is never read)
    ref = shr.predict(sc.oracle_model(c['d']), 'be', 0.01, Y, U, H, dtype=np.float64)
    assert (ref['status'] == 2).sum() == (H + 1) + H
    res = horizon_error(model, Y, U, H, dt=0.01, per_window=True, predictions=True)
    check_against_own_predictions(res, ref['status'], ref['Yw'], ref['windows'], 1, c['d']['n'], 'bad rows')
    bad = res.status == 2
    assert np.isnan(res.x_pred[bad]).all() and np.isnan(res.z_pred[bad]).all() and np.isfinite(res.x_pred[~bad]).all()
    clean = run_case('e3-b17', 'be@0.01')[0]
    assert same_bits(res.x_pred[~bad], clean.x_pred[~bad]) and same_bits(res.final_z[~bad], clean.final_z[~bad])


def diverging(d):
    """The model with the linear part of its discrete map replaced by 1e200 I: xh_2 = 1e400 x overflows in any summation order."""
    q = dict(d)
    q['Rd'] = np.hstack([1e200 * np.eye(d['n']), np.zeros((d['n'], d['Rd'].shape[1] - d['n']))])
    return q


def test_divergence_and_two_wins_over_one():
    from sofacontrol_amd.SSM.sysid import horizon_error
    c = shc.case('e3-b17')
    dd = _cache.setdefault('diverging', diverging(c['d']))
    model, H = product(dd, 'map'), c['H']
    res = horizon_error(model, c['Y'], c['U'], H, per_window=True, predictions=True)
    assert (res.status == 1).all() and res.diverged == res.windows == 51 and res.bad_rows == 0 and res.windows_ok == 0
    assert np.isnan(res.x_pred[:, 3:]).all() and np.isfinite(res.x_pred[:, 0]).all()            # left its loop at k <= 2: the rows behind are NaN
    assert not np.isfinite(res.x_pred[:, :3]).all(axis=(1, 2)).any()
    for f in ('rms_x', 'rms_z', 'worst_x', 'worst_z', 'final_x', 'final_z'):
        assert np.isnan(getattr(res, f)).all(), f
    assert (res.worst_x_at == -1).all() and (res.worst_z_at == -1).all() and not res.sse_x.any() and not res.sse_z.any()
    Y = c['Y'].copy()
    Y[1, 4, 0] = np.inf
    res = horizon_error(model, Y, c['U'], H, per_window=True)
    wins = shr.windows(3, 20, H, 1, 1)
    want = np.where((wins[:, 0] == 1) & (wins[:, 1] <= 4) & (4 <= wins[:, 1] + H), 2, 1)
    np.testing.assert_array_equal(res.status, want)
    assert res.bad_rows == int((want == 2).sum()) == 4 and res.diverged == 51 - 4 and np.isnan(res.rms_z).all()


# ---- 7. guards with a real handle ------------------------------------------------------------------------------------------------

def test_guards():
    from sofacontrol_amd.SSM.sysid import horizon_error, horizon_plan
    c = shc.case('h1')
    model = product(c['d'], 'be')
    with pytest.raises(RuntimeError, match=r'H = 1025, need 1 <= H <= 1024'):
        horizon_error(model, np.zeros((1, 1030, 5)), np.zeros((1, 1030, 5)), 1025)
    with pytest.raises(RuntimeError, match=r"W = 0 windows: T' = 6 kept rows per episode, H = 6"):
        horizon_error(model, c['Y'], c['U'], 6)
    cap = horizon_plan(model, 1, 2, 1)['pred_cap_bytes']
    E, T = 64, 4000                                                # 64 x 3989 windows x 13 rows x 10 doubles: above the cap
    with pytest.raises(RuntimeError, match=r'need \d+ bytes, above the cap of %d bytes' % cap):
        horizon_error(model, np.zeros((E, T, 5)), np.zeros((E, T, 5)), 12, predictions=True)
    d, _, _, _ = sc.rectangular_case()                             # n_x = 4, n_o = 6
    q = dict(d, W=np.zeros((6, 27)), Rd=d['R'], Bd=d['B'])
    rect = product(q, 'be', key='rect')
    with pytest.raises(RuntimeError, match=r'n_x = 4 != n_o = 6'):
        horizon_error(rect, np.zeros((1, 9, 6)), np.zeros((1, 9, 2)), 3)
