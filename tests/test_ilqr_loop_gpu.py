"""GPU: the resident iLQR plan (csrc/lqr.hip) and the batched closed-loop iLQR (csrc/ilqr_loop.hip, lqr/closed_loop.py).

1. the plan against the host-pointer call, bit for bit; 2. the advance kernel alone against the long-double statement
(tests/ilqr_loop_reference.py) on the seeded policies of tests/ilqr_loop_cases.py; 3. composition of runs; 4. the plan inside the loop;
5. the observed loop; 6. the traces of the reference's own controller (tests/golden/g25_ilqr_loop.npz); 7. the example.  Comparisons
between two runs of the same kernel on the same bits are exact; comparisons with the long-double statement use the project's rule
tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the float64 statement's own error on the same case (asserted
<= 1e-11), every figure printed before it is asserted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cl_cases as cc
import clobs_cases as oc
import ilqr_loop_cases as ic
import ilqr_loop_reference as ir
from helpers import product_tpwl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_SIMS = (0.05, 0.01)
_cache = {}


def plant(mname):
    """The product's TPWL model with the CPU tables of cl_cases installed at both time steps in use (so the statement reads the tables
    the kernels read)."""
    if ('tp', mname) not in _cache:
        m = cc.model(mname)
        tp = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        for dt in DT_SIMS:
            tp.handle_for(dt, tables=cc.tables(mname, dt))
        _cache[('tp', mname)] = tp
    return _cache[('tp', mname)]


def ilqr_of(mname, N):
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    tp = plant(mname)
    m = tp.get_input_dim()
    Qz = np.diag([0., 0., 0., 100., 100., 10.])
    return iLQR(ic.DT, tp, QuadraticCost(Q=Qz, R=1e-3 * np.eye(m), Qf=10 * Qz), N)


def solve_inputs(mname, N, B, seed):
    """x0 (B, n), z_target (B, N+1, 6), u_warm (B, N, m), u_last (B, m): all members distinct."""
    tp = plant(mname)
    n, m = tp.get_state_dim(), tp.get_input_dim()
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 1.0, N + 1)
    zt = np.zeros((B, N + 1, 6))
    for b in range(B):
        zt[b, :, 3] = -0.02 * (1 + 0.3 * b) * np.sin(th); zt[b, :, 4] = 0.01 * (1 - 0.2 * b) * np.sin(2 * th)
    zt = zt + np.asarray(tp.z_ref)
    return dict(x0=1e-3 * rng.standard_normal((B, n)), z=zt, uw=rng.uniform(0.0, 2.0, (B, N, m)), ul=rng.uniform(0.0, 1.0, (B, m)))


def make_loop(case, member=None, shared=False, **kw):
    """(loop, inputs) of an ADVANCE row with its seeded policy installed; member = b: the B = 1 loop of member b; shared: member 0's policy
    for every member, installed in the shared form."""
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    name, mname, B, N, r, steps, idle, dist, seed = case
    c = ic.advance_case(case)
    sel = slice(None) if member is None else slice(member, member + 1)
    c = dict(c, xbar=c['xbar'][sel], ubar=c['ubar'][sel], K=c['K'][sel], x=c['x'][sel], W=None if c['W'] is None else c['W'][:, sel])
    tp = plant(mname)
    cl = ILQRClosedLoopBatch(ilqr_of(mname, N), tp, ic.dt_sim_of(case), c['x'].shape[0], u0=c['u0'], **kw)
    if shared:
        cl.set_policy(c['xbar'][0], c['ubar'][0], c['K'][0])
    else:
        cl.set_policy(c['xbar'], c['ubar'], c['K'])
    return cl, c


def check(what, got, ref, e_oracle):
    e = ir.err(got, ref)
    print('%s: e_oracle %.3e, device %.3e, tolerance %.3e' % (what, e_oracle, e, ir.tolerance(e_oracle)))
    assert e_oracle <= ir.E_ORACLE_MAX
    assert e <= ir.tolerance(e_oracle)


# ------------------------------------------------------------------------------------------------ 1. plan equals host call, bit for bit
def plan_solve(il, B, z, shared, x0, uw, ul, outputs=True):
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    N, n, m = il.planning_horizon, il.state_dim, il.input_dim
    cp, par = il.cost_params, il._params()
    h = C.c_void_p()
    _lib.check(lib.silqr_plan_create(C.byref(h), il.model.handle_for(il.dt), C.c_int(N), C.c_int64(B), _lib.dptr(_lib.f64(cp.Q)),
                                     _lib.dptr(_lib.f64(cp.R)), _lib.dptr(_lib.f64(cp.Qf)), C.byref(par)), 'silqr_plan_create')
    try:
        _lib.check(lib.silqr_plan_set_target(h, _lib.dptr(_lib.f64(z)), C.c_int(1 if shared else 0)), 'silqr_plan_set_target')
        x, u, K = np.empty((B, N + 1, n)), np.empty((B, N, m)), np.empty((B, N, m, n))
        cost, iters = np.empty(B), np.empty(B, dtype=np.int32)
        if outputs:
            _lib.check(lib.silqr_plan_solve(h, _lib.dptr(_lib.f64(x0)), _lib.dptr(None if uw is None else _lib.f64(uw)),
                                            _lib.dptr(None if ul is None else _lib.f64(ul)), _lib.dptr(x), _lib.dptr(u), _lib.dptr(K),
                                            _lib.dptr(cost), _lib.iptr(iters)), 'silqr_plan_solve')
        else:                       # every output NULL: nothing comes back with the solve; the accessor fetches it afterwards
            _lib.check(lib.silqr_plan_solve(h, _lib.dptr(_lib.f64(x0)), _lib.dptr(None if uw is None else _lib.f64(uw)),
                                            _lib.dptr(None if ul is None else _lib.f64(ul)), None, None, None, None, None), 'silqr_plan_solve')
            _lib.check(lib.silqr_plan_policy(h, _lib.dptr(x), _lib.dptr(u), _lib.dptr(K), _lib.dptr(cost), _lib.iptr(iters)), 'silqr_plan_policy')
    finally:
        lib.silqr_plan_destroy(h)
    return x, u, K, cost, iters


def host_solve(il, B, z, x0, uw, ul):
    from sofacontrol_amd import _lib
    N, n, m = il.planning_horizon, il.state_dim, il.input_dim
    cp, par = il.cost_params, il._params()
    x, u, K = np.empty((B, N + 1, n)), np.empty((B, N, m)), np.empty((B, N, m, n))
    cost, iters = np.empty(B), np.empty(B, dtype=np.int32)
    _lib.check(_lib.lib().silqr_solve(il.model.handle_for(il.dt), C.c_int(N), C.c_int64(B), _lib.dptr(_lib.f64(x0)), _lib.dptr(_lib.f64(z)),
                                      _lib.dptr(None if uw is None else _lib.f64(uw)), _lib.dptr(None if ul is None else _lib.f64(ul)),
                                      _lib.dptr(_lib.f64(cp.Q)), _lib.dptr(_lib.f64(cp.R)), _lib.dptr(_lib.f64(cp.Qf)), C.byref(par),
                                      _lib.dptr(x), _lib.dptr(u), _lib.dptr(K), _lib.dptr(cost), _lib.iptr(iters)), 'silqr_solve')
    return x, u, K, cost, iters


@pytest.mark.parametrize('no_mfma', [False, True], ids=['mfma', 'valu'])
@pytest.mark.parametrize('mname,N', [('g6', 12), ('r36', 6)])
def test_plan_equals_the_host_call_bit_for_bit(mname, N, no_mfma, monkeypatch):
    if no_mfma:
        monkeypatch.setenv('SRH_ILQR_NO_MFMA', '1')
    else:
        monkeypatch.delenv('SRH_ILQR_NO_MFMA', raising=False)
    B = 3
    il = ilqr_of(mname, N)
    s = solve_inputs(mname, N, B, 21)
    for warm in (False, True):
        uw, ul = (s['uw'], s['ul']) if warm else (None, None)
        ref = host_solve(il, B, s['z'], s['x0'], uw, ul)
        assert (ref[4] > 0).all() and np.isfinite(ref[2]).all()
        got = plan_solve(il, B, s['z'], False, s['x0'], uw, ul)
        for a, b, f in zip(got, ref, ('x', 'u', 'K', 'cost', 'iters')):
            np.testing.assert_array_equal(a, b, err_msg='%s warm=%s' % (f, warm))
    # a shared target equals the same target tiled per member; NULL outputs and the accessor give the same policy
    tiled = np.ascontiguousarray(np.broadcast_to(s['z'][1], s['z'].shape))
    a = plan_solve(il, B, s['z'][1], True, s['x0'], s['uw'], s['ul'])
    b = plan_solve(il, B, tiled, False, s['x0'], s['uw'], s['ul'], outputs=False)
    c = host_solve(il, B, tiled, s['x0'], s['uw'], s['ul'])
    for x, y, z, f in zip(a, b, c, ('x', 'u', 'K', 'cost', 'iters')):
        np.testing.assert_array_equal(x, y, err_msg=f); np.testing.assert_array_equal(x, z, err_msg=f)


# ------------------------------------------------------------------------------------------------ 2. the advance kernel alone
@pytest.mark.parametrize('case', ic.ADVANCE, ids=ic.IDS)
def test_advance_against_the_long_double_statement(case):
    name, mname, B, N, r, steps, idle, dist, seed = case
    cl, c = make_loop(case)
    H = np.asarray(plant(mname).H)
    ref, e_oracle = ic.advance_measured(case, H)
    assert ref[4] >= ir.MARGIN
    X, Z, U, idx = cl._advance(c['x'], steps, W=c['W'])
    np.testing.assert_array_equal(idx, ref[3])
    check(name + ' U', U, ref[1], e_oracle); check(name + ' X', X, ref[0], e_oracle); check(name + ' Z', Z, ref[2], e_oracle)
    if idle:
        tail = c['rows'][np.minimum(np.arange(steps) // r, len(c['rows']) - 1)] < 0
        assert tail.any()
        np.testing.assert_array_equal(U[:, tail], np.broadcast_to(c['u0'], U[:, tail].shape))


def test_shared_policy_equals_the_same_policy_per_member():
    case = ic.ADVANCE[1]
    cl, c = make_loop(case, shared=True)
    B = case[2]
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a[0], a.shape))
    got = cl._advance(c['x'], case[5], W=c['W'])
    xb, ub, K = cl.last_policy()
    assert xb.shape == c['xbar'][0].shape
    np.testing.assert_array_equal(K, c['K'][0])
    cl.set_policy(tile(c['xbar']), tile(c['ubar']), tile(c['K']))
    assert cl.last_policy()[2].shape == (B,) + K.shape
    ref = cl._advance(c['x'], case[5], W=c['W'])
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(got[2][0], got[2][1])         # (the members start at different states)


# ------------------------------------------------------------------------------------------------ 3. composition
def same(a, b, fields=('x', 'z', 'u')):
    for f in fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def cat(rs):
    for a, b in zip(rs[:-1], rs[1:]):
        np.testing.assert_array_equal(a.x[:, -1], b.x[:, 0]); np.testing.assert_array_equal(a.z[:, -1], b.z[:, 0])
        assert a.t[-1] == pytest.approx(b.t[0], abs=1e-12)
    from sofacontrol_amd.lqr.closed_loop import ILQRLoopResult
    return ILQRLoopResult(np.concatenate([rs[0].x] + [r.x[:, 1:] for r in rs[1:]], axis=1),
                          np.concatenate([rs[0].z] + [r.z[:, 1:] for r in rs[1:]], axis=1), np.concatenate([r.u for r in rs], axis=1), None, None,
                          None, np.concatenate([rs[0].t] + [r.t[1:] for r in rs[1:]]))


def test_run_composes_and_equals_the_advance_kernel():
    case = ic.ADVANCE[1]                                    # r = 5, S = 67: the held input crosses the run boundary at step 7
    S = case[5]
    cl, c = make_loop(case, max_steps_per_run=S)
    cl.reset(c['x'])
    whole = cl.run(S, W=c['W'])
    assert cl.stats() == {'steps': S, 'waits_last_run': 1}
    np.testing.assert_array_equal(whole.x[:, 0], c['x'])
    assert whole.t.shape == (S + 1,) and whole.t[-1] == pytest.approx(S * 0.01) and whole.x_hat is None and whole.ekf_status is None
    X, Z, U, idx = cl._advance(c['x'], S, W=c['W'])
    np.testing.assert_array_equal(whole.x[:, 1:], X); np.testing.assert_array_equal(whole.z[:, 1:], Z); np.testing.assert_array_equal(whole.u, U)
    cl.reset(c['x'])
    split = cat([cl.run(7, W=c['W'][:7]), cl.run(S - 7, W=c['W'][7:])])
    same(whole, split)
    assert cl.stats()['steps'] == S
    cl.reset(c['x'])
    same(whole, cat([cl.run(1, W=c['W'][s:s + 1]) for s in range(S)]))
    # the advance hook resumes in the middle of a controller step from the held input
    X2, Z2, U2, _ = cl._advance(whole.x[:, 7], S - 7, step0=7, u_held=whole.u[:, 6], W=c['W'][7:])
    np.testing.assert_array_equal(X2, whole.x[:, 8:]); np.testing.assert_array_equal(U2, whole.u[:, 7:])
    # record_x = False
    cl.reset(c['x'])
    lean = cl.run(S, W=c['W'], record_x=False)
    assert lean.x is None
    same(whole, lean, ('z', 'u'))
    # W = 0 equals W = None
    cl.reset(c['x'])
    a = cl.run(12)
    cl.reset(c['x'])
    same(a, cl.run(12, W=np.zeros((12,) + c['W'].shape[1:])))
    # a member of the batch equals the member alone
    for b in (0, 2):
        one, c1 = make_loop(case, member=b, max_steps_per_run=S)
        one.reset(c1['x'])
        r1 = one.run(S, W=c1['W'])
        for f in ('x', 'z', 'u'):
            np.testing.assert_array_equal(getattr(r1, f)[0], getattr(whole, f)[b], err_msg=f)


def test_z_row_0_is_the_output_of_the_start_state():
    case = ic.ADVANCE[0]
    cl, c = make_loop(case)
    cl.reset(c['x'])
    r = cl.run(2)
    X, Z, U, _ = cl._advance(c['x'], 2)
    H = np.asarray(plant('g6').H)
    ref = np.asarray(c['x'], dtype=np.longdouble) @ np.asarray(H, dtype=np.longdouble).T
    check('z row 0', r.z[:, 0], ref, ir.err(c['x'] @ H.T, ref))
    np.testing.assert_array_equal(r.z[:, 1:], Z)


def test_refusals_that_need_a_handle():
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    case = ic.ADVANCE[0]
    c = ic.advance_case(case)
    cl = ILQRClosedLoopBatch(ilqr_of('g6', 12), plant('g6'), 0.05, 3, max_steps_per_run=10)
    with pytest.raises(RuntimeError, match='silqr_loop_run: no plant state yet'):
        cl.run(1)
    cl.reset(c['x'])
    with pytest.raises(RuntimeError, match='silqr_loop_run: no policy yet'):
        cl.run(1)
    with pytest.raises(RuntimeError, match='silqr_plan_solve_dev: no target yet'):
        cl.plan()
    with pytest.raises(RuntimeError, match='silqr_loop_last_policy: no policy yet'):
        cl.last_policy()
    cl.set_policy(c['xbar'], c['ubar'], c['K'])
    with pytest.raises(RuntimeError, match=r'steps = 11 exceeds max_steps_per_run = 10'):
        cl.run(11)
    with pytest.raises(RuntimeError, match='steps must be positive'):
        cl.run(0)
    with pytest.raises(RuntimeError, match="the loop's policy is not a plan's"):
        cl.plan_info()
    with pytest.raises(RuntimeError, match='x_bar must have shape'):
        cl.set_policy(c['xbar'][:, :5], c['ubar'], c['K'])
    assert cl.run(10).u.shape == (3, 10, 3)
    # (a TPWLATV without tables at dt_sim discretises them on demand: that refusal is the library's own, on a raw handle)
    m = cc.model('g6')
    bare = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], None)
    with pytest.raises(RuntimeError, match='output model'):
        ILQRClosedLoopBatch(ilqr_of('g6', 12), bare, 0.05, 3)
    from sofacontrol_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().silqr_loop_create(C.byref(h), None, plant('g6').handle_for(None), C.c_int(12), C.c_int(1), C.c_int64(3), C.c_int64(10))
    assert rc == -1 and b'has not been pre-discretised at dt_sim' in _lib.lib().srh_last_error()


# ------------------------------------------------------------------------------------------------ 4. the plan inside the loop
@pytest.mark.parametrize('mname,N,r', [('g6', 12, 5), ('r36', 6, 1)])
def test_plan_inside_the_loop(mname, N, r):
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    B, S = 3, 3 * r + 2
    s = solve_inputs(mname, N, B, 31)
    il = ilqr_of(mname, N)
    cl = ILQRClosedLoopBatch(il, plant(mname), ic.DT / r, B, z=s['z'])
    cl.reset(s['x0'])
    il.set_u_last(s['ul'])
    for uw in (None, s['uw']):
        cl.plan(uw)
        xb, ub, K = cl.last_policy()
        il.set_target(s['z'])
        x, u, Kh = il.ilqr_computation(s['x0'], uw)
        np.testing.assert_array_equal(xb, x); np.testing.assert_array_equal(ub, u); np.testing.assert_array_equal(K, Kh)
        info = cl.plan_info()
        np.testing.assert_array_equal(info['cost'], il.cost); np.testing.assert_array_equal(info['iters'], il.iters)
        assert (info['iters'] > 0).all()
    res = cl.run(S)
    assert cl.stats()['waits_last_run'] == 1 and np.isfinite(res.x).all()
    # the same steps by the advance kernel under the plan's policy, and under the same policy uploaded
    X, Z, U, _ = cl._advance(s['x0'], S)
    np.testing.assert_array_equal(res.x[:, 1:], X); np.testing.assert_array_equal(res.u, U); np.testing.assert_array_equal(res.z[:, 1:], Z)
    cl.set_policy(xb, ub, K)
    X2, Z2, U2, _ = cl._advance(s['x0'], S)
    np.testing.assert_array_equal(X2, X); np.testing.assert_array_equal(U2, U)
    # the plan tracks its own nominal on its own model: at r = 1 the undisturbed plant is the model of the plan's forward pass under the
    # same step rule, x - x_bar is 0 at step 0 and a rounding error at steps 1 and 2 (rows 0, 1, 2; step 3 reads row 2 again), so rows
    # 1..3 of the run are x_bar's up to rounding times the gain: 1e-9 leaves seven digits for |K|
    if r == 1:
        e = ir.err(res.x[:, 1:4], xb[:, 1:4])
        print('%s: closed loop on the plan\'s own model against x_bar, rows 1..3: %.3e' % (mname, e))
        assert e <= 1e-9


# ------------------------------------------------------------------------------------------------ 5. observed
def filter_model(same):
    """The product model the filters run on -- the plant's own, or the mismatched copy of clobs_cases -- with the measurement model."""
    if ('ftp', same) not in _cache:
        if same:
            tp = plant('g6')
        else:
            m = cc.model('g6')
            tp = product_tpwl(oc.mismatched_model('g6'), m['U'], m['q_ref'], m['v_ref'], m['Hf'])
            for dt in DT_SIMS:
                t = oc.filter_tables('g6', False, dt)
                tp.handle_for(dt, tables=(t['A_d'], t['B_d'], t['d_d']))
        ms = oc.measurement('g6')
        tp.C, tp.y_ref, tp.meas_dim = ms['C'], ms['y_ref'], ms['ny']
        _cache[('ftp', same)] = tp
    return _cache[('ftp', same)]


def make_observed(cs, member=None, **obs_kw):
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    name, same, r, steps, dist, noise, seed = cs
    c, ms = ic.observed_case(cs), oc.measurement('g6')
    sel = slice(None) if member is None else slice(member, member + 1)
    pick = lambda a, axis=0: None if a is None else (a[sel] if axis == 0 else a[:, sel])
    c = dict(c, xbar=c['xbar'][sel], ubar=c['ubar'][sel], K=c['K'][sel], x=c['x'][sel], x_hat=c['x_hat'][sel], W=pick(c['W'], 1), V=pick(c['V'], 1))
    B = c['x'].shape[0]
    kw = dict(Sigma0=ms['Sigma0'], W=ms['W'], V=ms['V'])
    kw.update(obs_kw)
    obs = DiscreteEKFObserverBatch(filter_model(same), B, **kw)
    cl = ILQRClosedLoopBatch(ilqr_of('g6', ic.OBS_N), plant('g6'), ic.DT / r, B, observer=obs)
    cl.set_policy(c['xbar'], c['ubar'], c['K'])
    return cl, c


@pytest.mark.parametrize('cs', ic.OBSERVED, ids=ic.OBS_IDS)
def test_observed_loop_against_the_long_double_statement(cs):
    name, same, r, steps, dist, noise, seed = cs
    cl, c = make_observed(cs)
    H = np.asarray(plant('g6').H)
    ref, e_oracle = ic.observed_measured(cs, H)
    assert ref['margin'] >= ir.MARGIN
    cl.reset(c['x'], c['x_hat'])
    res = cl.run(steps, W=c['W'], V=c['V'])
    assert cl.stats() == {'steps': steps, 'waits_last_run': 1}
    np.testing.assert_array_equal(res.x_hat[:, 0], c['x_hat']); np.testing.assert_array_equal(res.x[:, 0], c['x'])
    assert not res.ekf_status.any()
    for what, got, key in (('U', res.u, 'U'), ('X', res.x[:, 1:], 'X'), ('Z', res.z[:, 1:], 'Z'), ('Xhat', res.x_hat[:, 1:], 'Xhat'), ('Y', res.y, 'Y')):
        check('%s %s' % (name, what), got, ref[key], e_oracle)
    # split runs compose, and a member equals the same loop run with B = 1
    cl.reset(c['x'], c['x_hat'])
    k = 2
    a = cl.run(k, W=None if c['W'] is None else c['W'][:k], V=None if c['V'] is None else c['V'][:k])
    b = cl.run(steps - k, W=None if c['W'] is None else c['W'][k:], V=None if c['V'] is None else c['V'][k:])
    np.testing.assert_array_equal(np.concatenate((a.x_hat, b.x_hat[:, 1:]), axis=1), res.x_hat)
    np.testing.assert_array_equal(np.concatenate((a.u, b.u), axis=1), res.u)
    one, c1 = make_observed(cs, member=1)
    one.reset(c1['x'], c1['x_hat'])
    r1 = one.run(steps, W=c1['W'], V=c1['V'])
    for f in ('x', 'z', 'u', 'x_hat', 'y'):
        np.testing.assert_array_equal(getattr(r1, f)[0], getattr(res, f)[1], err_msg=f)


def test_a_filter_without_a_positive_definite_innovation_keeps_its_estimate():
    """The failing case of tests/ekf_cases.py (indefinite_sigmas, 'minus_identity': the one tests/test_ekf_batch_gpu.py hands a member)
    as the covariance every reset installs: Sigma0 = -1e6 I makes S = C (A Sigma0 A^T + W) C^T + V negative definite, so every filter
    keeps its estimate and its covariance at every step and sets its status word; the loop goes on, finite, under the law at the kept
    estimate, and the plants are those of the same loop with healthy filters as long as the law has not read a moved estimate."""
    cs = ic.OBSERVED[0]
    cl, c = make_observed(cs, Sigma0=-1e6 * np.eye(8))
    cl.reset(c['x'], c['x_hat'])
    res = cl.run(4)
    print('ekf_status', res.ekf_status)
    assert (res.ekf_status == 1).all()
    assert np.isfinite(res.x).all() and np.isfinite(res.u).all() and np.isfinite(res.y).all()
    np.testing.assert_array_equal(res.x_hat, np.broadcast_to(c['x_hat'][:, None], res.x_hat.shape))
    good, _ = make_observed(cs)
    good.reset(c['x'], c['x_hat'])
    ok = good.run(4)
    assert not ok.ekf_status.any()
    np.testing.assert_array_equal(res.u[:, 0], ok.u[:, 0]); np.testing.assert_array_equal(res.x[:, 1], ok.x[:, 1])
    assert not np.array_equal(res.u[:, 1], ok.u[:, 1])


# ------------------------------------------------------------------------------------------------ 6. the reference's traces (g25)
def g25_loop(tag):
    """The loop of the golden's problem (B = 1): the product model with the reference's own tables installed at dt and dt_sim, the
    golden's measurement model and filter covariances; the filter starts from the covariance behind the reference's first update."""
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    from sofacontrol_amd.utils import QuadraticCost
    from helpers import meas_selector
    g = ic.g25()
    if 'g25tp' not in _cache:
        mdl, U, q_ref, v_ref, Hf = g['problem']
        tp = product_tpwl(mdl, U, q_ref, v_ref, Hf, Cf=meas_selector([int(k) for k in g['meas_nodes']], 20))
        tp.handle_for(float(g['dt']), tables=(g['Ad'], g['Bd'], g['dd']))
        tp.handle_for(float(g['dt_sim']), tables=(g['Ad_sim'], g['Bd_sim'], g['dd_sim']))
        np.testing.assert_allclose(np.asarray(tp.C), g['C'], rtol=0, atol=1e-14)
        tp.C, tp.y_ref = g['C'], g['y_ref']
        _cache['g25tp'] = tp
    tp = _cache['g25tp']
    Q = np.diag([0, 0, 0, 100., 100., 0])
    il = iLQR(float(g['dt']), tp, QuadraticCost(Q=Q, R=1e-3 * np.eye(3), Qf=Q), ic.G25_N)
    obs = DiscreteEKFObserverBatch(tp, 1, Sigma0=g['ekf_Sigma_first'], W=g['Wf'], V=g['Vf']) if tag == 'ekf' else None
    cl = ILQRClosedLoopBatch(il, tp, float(g['dt_sim']), 1, z=g['z_target'], observer=obs, u0=g['u0'], max_steps_per_run=ic.G25_STEPS,
                             final_time=float(g['final_time']))
    np.testing.assert_array_equal(cl.rows, g['rows'])
    return cl, g


def g25_run(cl, g, tag):
    if tag == 'full':
        cl.reset(g['x0'][None])
        return cl.run(ic.G25_STEPS)
    S = ic.G25_STEPS - 1
    cl.reset(g['x0'][None], g['ekf_x_hat'][:1])
    return cl.run(S, W=g['w'][:S, None], V=g['v'][1:, None])


@pytest.mark.parametrize('tag', ['full', 'ekf'])
def test_the_references_traces_under_the_goldens_policy(tag):
    cl, g = g25_loop(tag)
    ref, e_oracle = ic.g25_measured(tag)
    gold = ic.g25_golden(tag)
    cl.set_policy(g[tag + '_x_bar'], g[tag + '_u_bar'], g[tag + '_K'])
    res = g25_run(cl, g, tag)
    assert cl.stats()['waits_last_run'] == 1
    check('g25 %s u against the golden' % tag, res.u[0], gold['U'], e_oracle)
    check('g25 %s x against the golden' % tag, res.x[0, 1:], gold['X'], e_oracle)
    if tag == 'ekf':
        check('g25 ekf x_hat against the golden', res.x_hat[0, 1:], gold['Xhat'], e_oracle)
        assert not res.ekf_status.any()
    np.testing.assert_array_equal(res.u[0, 65:], np.broadcast_to(g['u0'], res.u[0, 65:].shape))


@pytest.mark.parametrize('tag', ['full', 'ekf'])
def test_the_references_traces_under_the_loops_own_plan(tag):
    """plan() from the belief the reference planned from, then the run: x_bar to 1e-6 max(1, max|x_bar|) and u to 1e-5 max(1, max|u|) of
    the reference's -- the bounds tests/test_controllers_gpu.py holds the iLQR controller to against the same reference."""
    cl, g = g25_loop(tag)
    if tag == 'full':
        cl.reset(g['x0'][None])
    else:
        cl.reset(g['x0'][None], g['ekf_x_hat'][:1])
    cl.plan()
    xb, ub, K = cl.last_policy()
    ex = np.abs(xb[0] - g[tag + '_x_bar']).max() / max(1.0, np.abs(g[tag + '_x_bar']).max())
    print('g25 %s: x_bar of the loop\'s plan against the reference\'s %.3e (bound 1e-6), iterations %s' % (tag, ex, cl.plan_info()['iters']))
    assert ex <= 1e-6
    res = g25_run(cl, g, tag)
    gold = ic.g25_golden(tag)
    eu = np.abs(res.u[0] - gold['U']).max() / max(1.0, np.abs(gold['U']).max())
    print('g25 %s: u of the run against the reference\'s %.3e (bound 1e-5)' % (tag, eu))
    assert eu <= 1e-5


# ------------------------------------------------------------------------------------------------ 7. the example
@pytest.mark.parametrize('observer', [False, True], ids=['state', 'ekf'])
def test_the_example_runs(observer):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'diamond_ilqr_closed_loop_batch.py'), '--loops', '8', '--steps', '40']
    out = subprocess.run(cmd + (['--observer'] if observer else []), capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert 'waits_last_run 1' in out.stdout and 'tip error' in out.stdout
