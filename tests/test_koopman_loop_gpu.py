"""GPU: the batched closed-loop Koopman MPC (csrc/koopman_loop.hip, baselines/koopman/closed_loop.py), every arrow of a period.

Advance (koop_loop_advance_kernel alone on the seeded cases of tests/koopman_loop_cases.py, with the ring it leaves), fix-up
(loop_plan_shift_kernel of csrc/mpc_loop_host.h alone on seeded plans and status words, at N = 1 too, and in place inside a run),
preparation and solve (the request against the lift handle's own ring lift, the loop's plan against a second slocp plan fed with the loop's own inputs), their composition, and the reference's own
KoopmanMPC.evaluate traces (tests/golden/g22_koopman.npz) replayed through the loop.  Comparisons between two runs of the same kernel on
the same bits are exact; comparisons with the long-double reference (tests/koopman_loop_reference.py) use the project's rule
tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the float64 statement's own error on the same case (asserted
<= 1e-11 in tests/test_koopman_loop_reference_cpu.py), every figure printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import koopman_loop_cases as kc
import koopman_loop_reference as kr
from helpers import product_tpwl, Poly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('x', 'y', 'u', 'x_lift', 'iters', 'status', 'J')
_cache = {}


def plant(mname):
    """The product's TPWL model with the CPU tables of cl_cases installed at the two time steps the cases use."""
    if ('tp', mname) not in _cache:
        m = cc.model(mname)
        tp = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        for dt in kc.DT_SIM.values():
            tp.handle_for(dt, tables=tuple(cc.tables(mname, dt)))
        _cache[('tp', mname)] = tp
    return _cache[('tp', mname)]


def model_of(key):
    """The product's KoopmanModel of a spec of koopman_loop_cases."""
    from sofacontrol_amd.baselines.koopman import koopman_utils as ku
    s = kc.spec(key)
    arrays = {'A': s['A'], 'B': s['B'], 'C': s['H']}
    if s['W'] is not None:
        arrays['W'] = s['W']
    params = {'n': s['n_y'], 'm': s['m'], 'N': s['n_lift'], 'nzeta': s['nzeta'], 'delays': s['delays'], 'obs_degree': s['degree'], 'obs_type': 'poly',
              'Ts': kc.TS, 'scale': {k: s[k][None] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}}
    return ku.KoopmanModel(arrays, params, DMD=s['dmd'])


def ring_of(lift):
    """(ring (B, slots, n_y + m), head, count) of a lift handle, after everything enqueued on the device."""
    from sofacontrol_amd import _lib
    _lib.sync()
    ptr, slots, head, count, _ = lift.state()
    out = np.empty((lift.batch, slots, lift.n_y + lift.m))
    _lib.check(_lib.lib().srh_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes)), 'd2h')
    return out, head, count


def ring_lift(lift):
    """skoop_ring_lift_dev of the handle's ring as it stands: (B, n_lift)."""
    from sofacontrol_amd import _lib
    buf = _lib.DeviceBuffer(8 * lift.batch * lift.n_out)
    lift.ring_lift_dev(buf.ptr)
    _lib.sync()
    return buf.to_array((lift.batch, lift.n_out))


def advance_loop(case):
    """The loop of an ADVANCE row (no target: its own solve is not what the advance and fix-up cases are about)."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    name, mname, key, r, rh, B, dist, noise, mode, seed = case
    if ('adv', name) not in _cache:
        c = kc.advance_case(case)
        s = c['spec']
        cost = QuadraticCost(Q=np.eye(s['n_y']), R=1e-3 * np.eye(s['m']))
        sim = mode == 'sim'
        _cache[('adv', name)] = KoopmanClosedLoopBatch(model_of(key), kc.N, cost, plant(mname) if sim else None, c['C'] if sim else None,
                                                       c['y_ref'] if sim else None, c['dt_sim'], rh, batch=B, u0=np.full(s['m'], 30.0))
    return _cache[('adv', name)]


# ---------------------------------------------------------------------------------------------------------------- advance alone
@pytest.mark.parametrize('case', kc.ADVANCE, ids=lambda c: c[0])
def test_advance_alone(case):
    name, mname, key, r, rh, B, dist, noise, mode, seed = case
    c = kc.advance_case(case)
    s, nk = c['spec'], c['n_keep']
    cl = advance_loop(case)
    e_oracle, ref, f64 = kc.e_oracle(case)
    tol = cr.tolerance(e_oracle)
    h = kc.history(case, B)
    sim = mode == 'sim'
    cl.reset(x0=c['x'] if sim else None, y0=None if sim else c['Y_plant'][:, 0], y_hist=h['y_hist'], u_hist=h['u_hist'], u_prev0=h['u_prev0'],
             v0=h['v0'] if sim else None)
    ring0, head0, count0 = ring_of(cl.lift)
    assert (head0, count0) == (s['delays'], s['delays'] + 1)
    got = cl._advance(c['uopt'], c['x'] if sim else None, W=c['W'], V=c['V'], Y_plant=c['Y_plant'], U_applied=c['U_applied'])
    ring1, head1, count1 = ring_of(cl.lift)
    errs = {k: cr.err(got[k], ref[k]) for k in ('X', 'Y', 'U') if ref[k] is not None}
    print('%s: e_oracle %.3e, tolerance %.3e, device %s' % (name, e_oracle, tol, ', '.join('%s %.3e' % kv for kv in errs.items())))
    assert e_oracle <= cr.E_ORACLE_MAX
    for k, e in errs.items():
        assert got[k].shape == ref[k].shape, k
        assert e <= tol, (k, e, tol)
    np.testing.assert_array_equal(got['idx'], ref['picks'])
    if not sim:
        assert got['X'] is None
        np.testing.assert_array_equal(got['Y'], c['Y_plant'][:, 1:])
    if B == 260:
        assert len({got['Y'][b].tobytes() for b in range(B)}) == B
    # the ring: what n_keep skoop_push calls of the same raw samples leave, bit for bit; the slots the advance did not reach are untouched
    slots = s['delays'] + 1
    assert (head1, count1) == ((head0 + nk) % slots, count0 + nk)
    other = cl.model.new_lift(project=True, batch=B)
    for j in range(s['delays']):
        other.push(h['y_hist'][:, j], h['u_hist'][:, j])
    other.push(f64['Y'][:, 0] * 0.0, h['u_prev0'])                 # (a stand-in for y_0: its slot is compared with the loop's own below)
    pushed_u = got['U'] if c['U_applied'] is None else c['U_applied']
    for k in range(nk):
        other.push(got['Y'][:, k], pushed_u[:, k])
    ring2, head2, count2 = ring_of(other)
    assert (head2, count2) == (head1, count1)
    written = sorted({(head0 + 1 + k) % slots for k in range(nk)})
    kept = [q for q in range(slots) if q not in written]
    np.testing.assert_array_equal(ring1[:, written], ring2[:, written])
    np.testing.assert_array_equal(ring1[:, kept], ring0[:, kept])
    e_ring = cr.err(ring1[:, [(head0 + 1 + k) % slots for k in range(max(0, nk - slots), nk)]], ref['ring'][:, max(0, nk - slots):])
    print('%s: ring against the reference %.3e' % (name, e_ring))
    assert e_ring <= tol


# ---------------------------------------------------------------------------------------------------------------- fix-up alone
@pytest.mark.parametrize('case', [c for c in kc.ADVANCE if c[0] in ('r36-ship-5-1', 'g6-syn2-260', 'm8-w-1-1', 'g6-dmd-5-1')], ids=lambda c: c[0])
def test_fixup_alone(case):
    name, mname, key, r, rh, B = case[:6]
    cl = advance_loop(case)
    s = kc.spec(key)
    c = kc.fixup_case(B, s['n_lift'], s['m'], case[-1])
    assert B == 1 or (c['status'][1] != 0 and c['status'][0] == 0)
    if B == 1:
        c['status'][0] = 5
    u0s = (np.full(s['m'], 30.0) - s['u_offset']) / s['u_factor']             # (the loop's u0, scaled down by the same two operations)
    for first in (True, False):
        xo, uo = cl._fixup(c['xsol'], c['usol'], c['x0'], c['status'], None if first else c['xprev'], None if first else c['uprev'], first=first)
        for b in range(B):
            ex, eu = kr.fixup(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, u0s, np.float64)
            # copies, the idle input and the failure shift are exact
            np.testing.assert_array_equal(xo[b], ex); np.testing.assert_array_equal(uo[b], eu)
            if c['status'][b] != 0 and first:
                assert (xo[b] == c['x0'][b]).all() and (uo[b] == u0s).all()
            elif c['status'][b] != 0:
                np.testing.assert_array_equal(xo[b, :-1], c['xprev'][b, 1:]); np.testing.assert_array_equal(xo[b, -1], c['xprev'][b, -1])
                np.testing.assert_array_equal(uo[b, :-1], c['uprev'][b, 1:]); np.testing.assert_array_equal(uo[b, -1], c['uprev'][b, -1])
            else:
                np.testing.assert_array_equal(xo[b], c['xsol'][b]); np.testing.assert_array_equal(uo[b], c['usol'][b])


# ---------------------------------------------------------------------------------------------------------------- whole loops
# the shipped model on the r36 plant with the driver's cost, box and figure-8 target (tests/golden/g22_koopman.npz): name -> (r, rollout_horizon)
LOOPS = {'5-1': (5, 1), '1-3': (1, 3)}
PERIODS = 3
U0 = np.full(4, 300.0)


def loop_inputs(name, B):
    """Members 0..2 are the same for every B >= 3, and differ."""
    r, rh = LOOPS[name]
    nk = r * rh
    s = kc.spec('ship')
    mdl = cc.model('r36')['model']
    rng = np.random.default_rng(4100)
    nb = max(B, 3)
    x0 = np.concatenate((np.zeros((nb, 36)), mdl['q'][:nb] + 0.02 * rng.standard_normal((nb, 36))), axis=1)
    Cm = s['y_factor'][:, None] * kc.measurement('r36', 3, 0)[0]
    inp = dict(x0=x0, C=Cm, y_ref=s['y_offset'].copy(), phase=np.array([-0.2, 0.37, 9.8, 1.0])[:nb] if nb <= 4 else rng.uniform(0, 3, nb),
               y_hist=s['y_offset'] + 0.3 * s['y_factor'] * rng.standard_normal((nb, 1, 3)), u_hist=rng.uniform(250.0, 400.0, (nb, 1, 4)),
               u_prev0=rng.uniform(250.0, 400.0, (nb, 4)), v0=1e-3 * rng.standard_normal((nb, 3)),
               W=1e-4 * rng.standard_normal((PERIODS, 25, nb, 72))[:, :nk], V=1e-3 * rng.standard_normal((PERIODS, 25, nb, 3))[:, :nk])
    return {k: (v if k in ('C', 'y_ref') else (np.ascontiguousarray(v[:, :, :B]) if k in ('W', 'V') else v[:B])) for k, v in inp.items()}


def member_of(inp, b):
    s = slice(b, b + 1)
    return {k: (v if k in ('C', 'y_ref') else (np.ascontiguousarray(v[:, :, s]) if k in ('W', 'V') else v[s])) for k, v in inp.items()}


def make_loop(name, B, member=None, U=None, max_steps_per_run=None):
    """(loop, inputs) of LOOPS[name] with B members; member = b: the B = 1 loop of member b of the three-member batch."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    r, rh = LOOPS[name]
    g = kc.golden()
    inp = loop_inputs(name, 3 if member is not None else B)
    if member is not None:
        inp = member_of(inp, member)
    cost = QuadraticCost(Q=g['cost_Q'], R=g['cost_R'], Qf=2.0 * g['cost_Q'] if name == '1-3' else None)
    cl = KoopmanClosedLoopBatch(model_of('ship'), kc.N, cost, plant('r36'), inp['C'], inp['y_ref'], kc.DT_SIM[r], rh, t=g['cost_t'], z=g['cost_z'],
                                u=g['cost_u'], phase=inp['phase'], U=Poly(g['cost_UA'], g['cost_Ub']) if U is None else U, u0=U0, batch=B,
                                max_steps_per_run=max_steps_per_run)
    return cl, inp


def reset(cl, inp, t_start=0.1):
    cl.reset(x0=inp['x0'], y_hist=inp['y_hist'], u_hist=inp['u_hist'], u_prev0=inp['u_prev0'], v0=inp['v0'], t_start=t_start)


def same(a, b, what=''):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg='%s %s' % (what, f))


def cat(rs):
    """Records of consecutive runs as one: the first row of a later run repeats the last row of the one before."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanLoopResult
    for a, b in zip(rs[:-1], rs[1:]):
        for f in ('x', 'y'):
            np.testing.assert_array_equal(getattr(a, f)[:, -1], getattr(b, f)[:, 0], err_msg=f)
        assert a.t[-1] == pytest.approx(b.t[0], abs=1e-12)
    rows1 = lambda f: np.concatenate([getattr(rs[0], f)] + [getattr(r, f)[:, 1:] for r in rs[1:]], axis=1)
    per = lambda f: np.concatenate([getattr(r, f) for r in rs])
    return KoopmanLoopResult(rows1('x'), rows1('y'), np.concatenate([r.u for r in rs], axis=1), per('x_lift'), per('iters'), per('status'), per('J'),
                             np.concatenate([rs[0].t] + [r.t[1:] for r in rs[1:]]))


def second_plan_solve(cl, li):
    """slocp_plan_solve on a second plan of the loop's problem and batch, fed the loop's own inputs: x, u, J, status, iters."""
    from sofacontrol_amd import _lib
    B, N, n, m = cl.B, cl.N, cl.n_x, cl.n_u
    L = _lib.lib()
    plan = C.c_void_p()
    _lib.check(L.slocp_plan_create(C.byref(plan), C.byref(cl.problem()), C.c_int64(B)), 'slocp_plan_create')
    try:
        tile = lambda a: _lib.f64(np.broadcast_to(np.asarray(a), (B, N) + np.shape(a)))
        Ad, Bd, dd = tile(cl.model.A_d), tile(cl.model.B_d), tile(np.zeros(n))
        x, u, s = np.empty((B, N + 1, n)), np.empty((B, N, m)), np.empty((B, N + 1))
        J, st, it = np.empty(B), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        zero = np.zeros(B)
        _lib.check(L.slocp_plan_solve(plan, _lib.dptr(Ad), _lib.dptr(Bd), _lib.dptr(dd), _lib.dptr(_lib.f64(li['x0'])), None, _lib.dptr(zero),
                                      _lib.dptr(zero), _lib.dptr(li['z']), _lib.dptr(li['zf']), _lib.dptr(li['u']), _lib.dptr(x), _lib.dptr(u),
                                      _lib.dptr(s), _lib.dptr(J), _lib.iptr(st), _lib.iptr(it)), 'slocp_plan_solve')
    finally:
        L.slocp_plan_destroy(plan)
    return x, u, J, st, it


@pytest.mark.parametrize('name', list(LOOPS))
def test_preparation_and_solve(name):
    from sofacontrol_amd.scp.closed_loop import schedule
    from test_gusto_loop_gpu import check_window
    r, rh = LOOPS[name]
    nk = r * rh
    g = kc.golden()
    s = kc.spec('ship')
    cl, inp = make_loop(name, 3)
    t_start, N = 0.1, kc.N
    assert cc.DT == kc.TS                                         # (check_window steps the window at cc.DT)
    reset(cl, inp, t_start)
    # y_0 = (C x0 + y_ref) + v0 and the history, as the reference statement lifts them
    y0 = inp['x0'] @ inp['C'].T + inp['y_ref'] + inp['v0']
    sd_y = lambda v: kr.scale_down(v, s['y_offset'], s['y_factor'], cr.LD)
    sd_u = lambda v: kr.scale_down(v, s['u_offset'], s['u_factor'], cr.LD)
    want = np.stack([kr.lift(s, [sd_y(inp['y_hist'][b, 0]), sd_y(y0[b])], [sd_u(inp['u_hist'][b, 0]), sd_u(inp['u_prev0'][b])], cr.LD) for b in range(3)])
    runs = []
    for p in range(2):
        xl = ring_lift(cl.lift)
        res = cl.step(W=inp['W'][p:p + 1], V=inp['V'][p:p + 1])
        li, (xo, uo) = cl.last_inputs(), cl.last_plan()
        runs.append(res)
        # the request: the lift handle's own ring lift of the same ring, bit for bit
        np.testing.assert_array_equal(res.x_lift[0], xl); np.testing.assert_array_equal(li['x0'], xl)
        sk = schedule(N, kc.TS, kc.DT_SIM[r], nk, t_start, p)
        assert res.t[0] == sk.t_k and res.t.shape == (nk + 1,)
        check_window('z, period %d' % p, li['z'], g['cost_t'], g['cost_z'], sk.t_k + inp['phase'], N + 1)
        np.testing.assert_array_equal(li['u'], np.broadcast_to(g['cost_u'], (3, N, 4)))
        if name == '1-3':
            np.testing.assert_array_equal(li['zf'], li['z'][:, -1])
        else:
            assert li['zf'] is None
        x, u, J, st, it = second_plan_solve(cl, li)
        print('period %d: status %s, iterations %s' % (p, st, it))
        assert not st.any()
        np.testing.assert_array_equal(res.status[0], st); np.testing.assert_array_equal(res.iters[0], it); np.testing.assert_array_equal(res.J[0], J)
        np.testing.assert_array_equal(xo, x); np.testing.assert_array_equal(uo, u)
        # the inputs applied: scale_up of the plan row of the controller step that has fired
        for k in range(nk):
            np.testing.assert_array_equal(res.u[:, k], u[:, k // r] * s['u_factor'] + s['u_offset'])
    assert (inp['phase'][0] + t_start < g['cost_t'][0]) and (inp['phase'][2] + t_start + kc.TS * N > g['cost_t'][-1])      # both clamped ends
    measure = lambda x, v, dtype: (np.einsum('ij,b...j->b...i', inp['C'].astype(dtype), x.astype(dtype)) + inp['y_ref'].astype(dtype)) + v.astype(dtype)
    y0_ref = measure(inp['x0'], inp['v0'], cr.LD)
    e0, ey, ey_oracle = cr.err(runs[0].x_lift[0], want), cr.err(runs[0].y[:, 0], y0_ref), cr.err(measure(inp['x0'], inp['v0'], np.float64), y0_ref)
    print('%s: first request against the long-double lift %.3e, y_0 %.3e (e_oracle %.3e)' % (name, e0, ey, ey_oracle))
    assert e0 <= 1e-12 and ey <= cr.tolerance(ey_oracle)
    np.testing.assert_array_equal(runs[0].x[:, 0], inp['x0'])
    np.testing.assert_array_equal(runs[1].y[:, 0], runs[0].y[:, -1])
    v1 = inp['V'][1].transpose(1, 0, 2)
    y_ref = measure(runs[1].x[:, 1:], v1, cr.LD)
    e, e_oracle = cr.err(runs[1].y[:, 1:], y_ref), cr.err(measure(runs[1].x[:, 1:], v1, np.float64), y_ref)
    print('%s: recorded y against (C x + y_ref) + v: %.3e (e_oracle %.3e)' % (name, e, e_oracle))
    assert e <= cr.tolerance(e_oracle)


def test_member_of_a_batch_equals_the_member_alone():
    name = '5-1'
    cl, inp = make_loop(name, 3)
    reset(cl, inp)
    rb = cl.run(2, W=inp['W'][:2], V=inp['V'][:2])
    assert not rb.status.any()
    for b in range(3):
        one, i1 = make_loop(name, 1, member=b)
        reset(one, i1)
        r1 = one.run(2, W=i1['W'][:2], V=i1['V'][:2])
        for f in FIELDS:
            got = getattr(rb, f)
            np.testing.assert_array_equal(got[:, b:b + 1] if f in ('iters', 'status', 'J', 'x_lift') else got[b:b + 1], getattr(r1, f),
                                          err_msg='member %d %s' % (b, f))
    assert not np.array_equal(rb.u[0], rb.u[1])


@pytest.mark.parametrize('name', list(LOOPS))
def test_composition(name):
    r, rh = LOOPS[name]
    nk = r * rh
    cl, inp = make_loop(name, 3)
    W, V = inp['W'], inp['V']
    reset(cl, inp)
    whole = cl.run(PERIODS, W=W, V=V)
    assert cl.stats() == {'steps': PERIODS, 'waits_last_run': 1}
    assert whole.x.shape == (3, PERIODS * nk + 1, 72) and whole.y.shape == (3, PERIODS * nk + 1, 3) and whole.u.shape == (3, PERIODS * nk, 4)
    assert whole.x_lift.shape == (PERIODS, 3, 66) and whole.J.shape == (PERIODS, 3)
    print('%s: status %s, iterations %s' % (name, whole.status.ravel(), whole.iters.ravel()))
    assert not whole.status.any()
    # two consecutive runs equal one run; so do single steps
    reset(cl, inp)
    same(cat([cl.run(2, W=W[:2], V=V[:2]), cl.run(1, W=W[2:], V=V[2:])]), whole, 'two runs')
    assert cl.stats() == {'steps': PERIODS, 'waits_last_run': 1}
    reset(cl, inp)
    same(cat([cl.step(W=W[p:p + 1], V=V[p:p + 1]) for p in range(PERIODS)]), whole, 'three steps')
    # W = 0 equals W = None
    reset(cl, inp)
    a = cl.run(2, W=np.zeros_like(W[:2]), V=V[:2])
    reset(cl, inp)
    b = cl.run(2, V=V[:2])
    same(a, b, 'W = 0')
    nox = cl.run(1, V=V[2:3], record_x=False)
    assert nox.x is None and nox.y.shape == (3, nk + 1, 3)
    # run = reset + the per-period arrows chained by hand on a second loop: ring lift -> plan solve -> _fixup -> _advance
    hand, _ = make_loop(name, 3)
    reset(cl, inp)
    reset(hand, inp)
    x = inp['x0']
    xprev = uprev = None
    for p in range(PERIODS):
        res = cl.step(W=W[p:p + 1], V=V[p:p + 1])
        li = cl.last_inputs()
        xl = ring_lift(hand.lift)
        np.testing.assert_array_equal(res.x_lift[0], xl, err_msg='period %d request' % p)
        xs, us, J, st, it = second_plan_solve(cl, dict(li, x0=xl))
        xo, uo = hand._fixup(xs, us, xl, st, xprev, uprev, first=p == 0)
        adv = hand._advance(uo, x, W=W[p], V=V[p])
        np.testing.assert_array_equal(res.x[:, 1:], adv['X'], err_msg='period %d x' % p)
        np.testing.assert_array_equal(res.y[:, 1:], adv['Y'], err_msg='period %d y' % p)
        np.testing.assert_array_equal(res.u, adv['U'], err_msg='period %d u' % p)
        np.testing.assert_array_equal(res.J[0], J); np.testing.assert_array_equal(res.status[0], st)
        x, xprev, uprev = adv['X'][:, -1], xo, uo
    np.testing.assert_array_equal(ring_of(cl.lift)[0], ring_of(hand.lift)[0])
    # refusals that need the handle
    with pytest.raises(RuntimeError, match='exceeds max_steps_per_run'):
        cl.run(17)
    with pytest.raises(RuntimeError, match='call reset first'):
        hand.run(1)                                               # (_advance moved its ring on)
    fresh, _ = make_loop(name, 3)
    with pytest.raises(RuntimeError, match='call reset first'):
        fresh.run(1)


def test_failed_solves_go_on():
    """An input box no input satisfies: every QP reports a non-zero status, the status is recorded and the loop goes on -- period 0 on
    the request state and the scaled-down u0, later periods on the plan moved up one row."""
    s = kc.spec('ship')
    box = Poly(np.vstack((np.eye(4), -np.eye(4))), np.concatenate((np.full(4, -1.0), np.full(4, -1.0))))       # u <= -1 and u >= 1
    cl, inp = make_loop('1-3', 3, U=box)
    reset(cl, inp)
    r0 = cl.run(1)
    xo0, uo0 = cl.last_plan()
    r1 = cl.run(2)
    xo, uo = cl.last_plan()
    print('infeasible box: status %s' % np.concatenate((r0.status, r1.status)).ravel())
    assert r0.status.all() and r1.status.all()
    u0s = (U0 - s['u_offset']) / s['u_factor']
    assert (xo0 == r0.x_lift[0][:, None]).all() and (uo0 == u0s).all()
    assert (xo == r0.x_lift[0][:, None]).all() and (uo == u0s).all()                  # (a constant plan moved up stays what it was)
    np.testing.assert_array_equal(r0.u, np.broadcast_to(u0s * s['u_factor'] + s['u_offset'], r0.u.shape))
    np.testing.assert_array_equal(r1.u, np.broadcast_to(u0s * s['u_factor'] + s['u_offset'], r1.u.shape))
    assert np.isfinite(r1.x).all() and np.isfinite(r1.y).all() and np.isfinite(r1.x_lift).all()
    # later periods alone: a plan that is not constant moves up ONE row whatever rollout_horizon is (here 3)
    c = kc.fixup_case(3, 66, 4, 2)
    c['status'][:] = 7
    xs, us = cl._fixup(c['xsol'], c['usol'], c['x0'], c['status'], c['xprev'], c['uprev'], first=False)
    np.testing.assert_array_equal(xs[:, :-1], c['xprev'][:, 1:]); np.testing.assert_array_equal(us[:, :-1], c['uprev'][:, 1:])
    np.testing.assert_array_equal(xs[:, -1], c['xprev'][:, -1]); np.testing.assert_array_equal(us[:, -1], c['uprev'][:, -1])


# ---------------------------------------------------------------------------------------------------------------- the shortest horizon
def short_loop():
    """(loop, inputs) of the shipped model on the r36 plant at N = 1 -- the shortest horizon slocp_plan_create accepts (scp_host.h:
    N >= 1) -- with B = 2, r = 5, rollout_horizon = 1."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    inp = loop_inputs('5-1', 2)
    if 'short' not in _cache:
        g = kc.golden()
        _cache['short'] = KoopmanClosedLoopBatch(model_of('ship'), 1, QuadraticCost(Q=g['cost_Q'], R=g['cost_R']), plant('r36'), inp['C'],
                                                 inp['y_ref'], kc.DT_SIM[5], 1, t=g['cost_t'], z=g['cost_z'], u=g['cost_u'], phase=inp['phase'],
                                                 U=Poly(g['cost_UA'], g['cost_Ub']), u0=U0, batch=2)
    return _cache['short'], inp


def test_fixup_alone_at_the_shortest_horizon():
    """N = 1, one member solved and one failed, first and later period: min(k + 1, N - 1) = 0 for the one input row and min(k + 1, N) = N
    for both state rows of the failed member."""
    cl, _ = short_loop()
    s = kc.spec('ship')
    n, m = s['n_lift'], s['m']
    rng = np.random.default_rng(9877)
    c = dict(xsol=rng.standard_normal((2, 2, n)), usol=rng.standard_normal((2, 1, m)), x0=rng.standard_normal((2, n)),
             xprev=rng.standard_normal((2, 2, n)), uprev=rng.standard_normal((2, 1, m)), status=np.array([0, 3], dtype=np.int32))
    u0s = (U0 - s['u_offset']) / s['u_factor']
    for first in (True, False):
        xo, uo = cl._fixup(c['xsol'], c['usol'], c['x0'], c['status'], None if first else c['xprev'], None if first else c['uprev'], first=first)
        for b in range(2):
            ex, eu = kr.fixup(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, u0s, np.float64)
            np.testing.assert_array_equal(xo[b], ex); np.testing.assert_array_equal(uo[b], eu)
        np.testing.assert_array_equal(xo[0], c['xsol'][0]); np.testing.assert_array_equal(uo[0], c['usol'][0])
        if first:
            assert (xo[1] == c['x0'][1]).all() and (uo[1] == u0s).all()
        else:                      # one row up with the last row held: both state rows are the previous plan's last, the input row its only one
            assert (xo[1] == c['xprev'][1, 1]).all()
            np.testing.assert_array_equal(uo[1], c['uprev'][1])


def test_run_shifts_in_place_as_the_fixup_alone():
    """Inside a run the shift kernel's output is the array the solve wrote (xsol is xout).  The same N = 1 loop with member 1 forced to
    fail -- the older sample of its ring is not a number, so is its request, which the interior point reports (ipm_rule.h:
    verdict_failed) -- and member 0 solved: the plan behind the period equals the stand-alone entry's answer, which writes into a third
    array, for the same inputs; the request record is the request."""
    cl, inp = short_loop()
    inp = dict(inp, y_hist=inp['y_hist'].copy())
    inp['y_hist'][1] = np.nan
    reset(cl, inp)
    r = cl.step()
    li, (xo, uo) = cl.last_inputs(), cl.last_plan()
    assert np.isnan(li['x0'][1]).any() and np.isfinite(li['x0'][0]).all()
    np.testing.assert_array_equal(r.x_lift[0], li['x0'])
    xs, us, J, st, it = second_plan_solve(cl, li)
    print('status %s' % st)
    assert st[0] == 0 and st[1] != 0
    np.testing.assert_array_equal(r.status[0], st)
    ax, au = cl._fixup(xs, us, li['x0'], st, None, None, first=True)
    np.testing.assert_array_equal(xo, ax); np.testing.assert_array_equal(uo, au)
    np.testing.assert_array_equal(xo[0], xs[0]); np.testing.assert_array_equal(uo[0], us[0])
    s = kc.spec('ship')
    assert (uo[1] == (U0 - s['u_offset']) / s['u_factor']).all()
    np.testing.assert_array_equal(xo[1], np.broadcast_to(li['x0'][1], xo[1].shape))


# ---------------------------------------------------------------------------------------------------------------- the reference's trace
@pytest.mark.parametrize('rh,periods', [(1, 11), (3, 3)])
def test_reference_trace(rh, periods):
    """The reference's own KoopmanMPC.evaluate runs replayed through the loop: B = 1, plant=None, Y_plant = trace_y[200:] (from the first
    solve on), U_applied = tr_<rh>_0_u of the same rows, history from rows 199 / 198.  Bounds: t[::n_keep] against req_t at 1e-9, the
    requests against req_x0 to 1e-12 relative, u against the trace within 1e-6 max|u| (the figures of tests/test_koopman_gpu.py::
    test_evaluate_trace); the same run without U_applied -- the loop's own inputs go into the ring -- within the looser of the two."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    g = kc.golden()
    tag = 'tr_%d_0_' % rh
    nk = 5 * rh
    S = periods * nk
    y, u = g['trace_y'], g[tag + 'u']
    assert {1: (256, 55), 3: (246, 45)}[rh] == (200 + S + 1, S)
    cl = KoopmanClosedLoopBatch(model_of('ship'), int(g['mpc_N']), QuadraticCost(Q=g['cost_Q'], R=g['cost_R']), None, None, None, 0.01, rh,
                                t=g['cost_t'], z=g['cost_z'], u=g['cost_u'], U=Poly(g['cost_UA'], g['cost_Ub']), u0=U0, max_steps_per_run=S)
    req_t, req_x = g[tag + 'req_t'], g[tag + 'req_x0']
    np_ = min(periods, len(req_t))
    for with_u in (True, False):
        cl.reset(y0=y[None, 200], y_hist=y[None, 199:200], u_hist=u[None, 198:199], u_prev0=u[None, 199], t_start=0.0)
        res = cl.run(periods, Y_plant=y[None, 200:200 + S + 1], U_applied=u[None, 200:200 + S] if with_u else None)
        assert cl.stats()['waits_last_run'] == 1 and not res.status.any() and res.x is None
        np.testing.assert_array_equal(res.y[0], y[200:200 + S + 1])
        e_x = np.abs(res.x_lift[:np_, 0] - req_x[:np_]).max() / np.abs(req_x[:np_]).max()
        e_u = np.abs(res.u[0] - u[200:200 + S]).max() / np.abs(u).max()
        print('trace rh %d, U_applied %s: %d periods, requests %.3e relative, u %.3e of max|u|' % (rh, with_u, periods, e_x, e_u))
        np.testing.assert_allclose(res.t[::nk][:np_], req_t[:np_], rtol=0, atol=1e-9)
        assert e_u <= 1e-6
        assert e_x <= (1e-12 if with_u else 1e-6)


# ---------------------------------------------------------------------------------------------------------------- the example
def test_batch_example_runs():
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'diamond_koopman_closed_loop_batch.py'), '--batch', '3', '--periods', '2'],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'koopman closed loop batch: 3 loops x 2 periods' in res.stdout and 'waits_last_run 1' in res.stdout, res.stdout[-2000:]
