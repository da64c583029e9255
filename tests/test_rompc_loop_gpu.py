"""GPU: the batched closed-loop ROMPC (csrc/rompc_loop.hip, baselines/rompc/closed_loop.py), every arrow of a period.

Preparation (request state, target window), solve (the loop's plan against a second slocp plan fed with the loop's own inputs), chain
(loop_plan_shift_kernel of csrc/mpc_loop_host.h alone on seeded plans and status words, at N = 1 too, and in place inside a run),
advance (rompc_loop_advance_kernel alone on the seeded cases of tests/rompc_loop_cases.py), their composition, and the imported
reference's trace (tests/golden/g23_rompc.npz) replayed through the loop.
Comparisons between two runs of the same kernel on the same bits are exact; comparisons with the long-double reference
(tests/rompc_loop_reference.py) use the project's rule tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the
float64 statement's own error on the same case (asserted <= 1e-11 in tests/test_rompc_loop_reference_cpu.py), every figure printed
before it is asserted."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import rompc_loop_cases as rc
import rompc_loop_reference as rr
from helpers import product_tpwl, Poly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_SIMS = (0.05, 0.01, 0.03)
FIELDS = ('x', 'x_hat', 'y', 'z', 'u', 'u_bar', 'x_bar', 'iters', 'status', 'J')
_cache = {}


def plant(mname, mode='sim'):
    """The product's TPWL model with the CPU tables of cl_cases installed at every time step the cases use; 'one': its first point alone."""
    if mode == 'replay':
        return None
    if ('tp', mname, mode) not in _cache:
        m = cc.model(mname)
        mdl, cut = m['model'], (lambda a: a[:1]) if mode == 'one' else (lambda a: a)
        if mode == 'one':
            mdl = dict(mdl, **{k: mdl[k][:1] for k in ('q', 'v', 'u', 'A_c', 'B_c', 'd_c')})
        tp = product_tpwl(mdl, m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        for dt in DT_SIMS:
            tp.handle_for(dt, tables=tuple(cut(t) for t in cc.tables(mname, dt)))
        _cache[('tp', mname, mode)] = tp
    return _cache[('tp', mname, mode)]


def observer(ctrl, B):
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    s = types.SimpleNamespace(A_d=ctrl['A'], B_d=ctrl['B'], d_d=ctrl['d'], C=ctrl['C'], y_ref=ctrl['y_ref'], H=ctrl['H_model'], z_ref=ctrl['z_ref'],
                              rom=None)
    ob = DiscreteLuenbergerObserver(s, None, None, batch=B, L=ctrl['L'])
    ob.K = ctrl['K']
    return ob


def mpc_model(mname):
    """The QP's model: the first table point at dt_mpc with the model's output map."""
    Ad, Bd, dd = cc.tables(mname, cc.DT)
    return types.SimpleNamespace(A_d=np.array(Ad[0]), B_d=np.array(Bd[0]), d_d=np.array(dd[0]), H=cc.model(mname)['H'])


def advance_loop(case):
    """The loop of an ADVANCE row (no target: its own solve is not what the advance and chain cases are about)."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    name, mname, B, ny, dt_sim, nk, dist, noise, with_H, mode, seed = case
    if ('adv', name) not in _cache:
        c = rc.advance_case(case)
        m = c['uopt'].shape[2]
        cost = QuadraticCost(Q=np.diag([0, 0, 0, 100., 100., 0]), R=1e-5 * np.eye(m))
        _cache[('adv', name)] = ROMPCClosedLoopBatch(observer(c['ctrl'], B), mpc_model(mname), cc.N, cc.DT, cost, plant(mname, mode), dt_sim, nk)
    return _cache[('adv', name)]


# whole loops on the g6 problem (targets, cost and input box of tests/golden/g6_gusto.npz): name -> (dt_sim, n_replan, n_y, terminal cost and
# input target)
LOOPS = {'frac': (0.03, 10, 30, False), 'zf-u': (0.01, 10, 3, True)}
PERIODS = 4


def loop_inputs(name, B):
    dt_sim, nk, ny, full = LOOPS[name]
    inp = cc.loop_inputs(B, nk)
    rng = np.random.default_rng(91)
    inp['x_hat0'] = inp['x0'] + 2e-4 * rng.standard_normal((max(B, 3), 8))[:B]
    inp['V'] = 1e-4 * rng.standard_normal((PERIODS, nk, max(B, 3), ny))[:, :, :B]
    return inp


def make_loop(name, B, member=None, max_steps_per_run=None):
    """(loop, inputs) of LOOPS[name] with B members; member = b: the B = 1 loop of member b of the three-member batch."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    dt_sim, nk, ny, full = LOOPS[name]
    g = cc.g6()
    inp = loop_inputs(name, max(B, 3) if member is not None else B)
    if member is not None:
        s = slice(member, member + 1)
        inp = dict(inp, x0=inp['x0'][s], x_hat0=inp['x_hat0'][s], phase=inp['phase'][s], W=np.ascontiguousarray(inp['W'][:, :, s]),
                   V=np.ascontiguousarray(inp['V'][:, :, s]))
    ctrl = rc.controller('g6', ny, dt_sim, True)
    cost = QuadraticCost(Q=g['Qz'], R=g['R'], Qf=2.0 * g['Qz'] if full else None)
    cl = ROMPCClosedLoopBatch(observer(ctrl, B), mpc_model('g6'), cc.N, cc.DT, cost, plant('g6'), dt_sim, nk, t=g['t'], z=g['zt'],
                              u=inp['ut'] if full else None, phase=inp['phase'], U=Poly(g['U_A'], g['U_b']), max_steps_per_run=max_steps_per_run)
    return cl, inp


def same(a, b, what=''):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg='%s %s' % (what, f))


def cat(rs):
    """Records of consecutive runs as one: the first row of a later run repeats the last row of the one before."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCLoopResult
    for a, b in zip(rs[:-1], rs[1:]):
        for f in ('x', 'x_hat', 'z', 'x_bar'):
            np.testing.assert_array_equal(getattr(a, f)[:, -1], getattr(b, f)[:, 0], err_msg=f)
        assert a.t[-1] == pytest.approx(b.t[0], abs=1e-12)
    rows1 = lambda f: np.concatenate([getattr(rs[0], f)] + [getattr(r, f)[:, 1:] for r in rs[1:]], axis=1)
    rows = lambda f: np.concatenate([getattr(r, f) for r in rs], axis=1)
    per = lambda f: np.concatenate([getattr(r, f) for r in rs])
    return ROMPCLoopResult(rows1('x'), rows1('x_hat'), rows('y'), rows1('z'), rows('u'), rows('u_bar'), rows1('x_bar'), per('iters'), per('status'),
                           per('J'), np.concatenate([rs[0].t] + [r.t[1:] for r in rs[1:]]))


def second_plan_solve(cl, li):
    """slocp_plan_solve on a second plan of the loop's problem and batch, fed the loop's own inputs: x, u, J, status, iters."""
    from sofacontrol_amd import _lib
    B, N, n, m = cl.B, cl.N, cl.n_x, cl.n_u
    L = _lib.lib()
    plan = C.c_void_p()
    _lib.check(L.slocp_plan_create(C.byref(plan), C.byref(cl.problem()), C.c_int64(B)), 'slocp_plan_create')
    try:
        tile = lambda a: _lib.f64(np.broadcast_to(np.asarray(a), (B, N) + np.shape(a)))
        mm = cl.mpc_model
        Ad, Bd, dd = tile(mm.A_d), tile(mm.B_d), tile(np.ravel(mm.d_d))
        x, u, s = np.empty((B, N + 1, n)), np.empty((B, N, m)), np.empty((B, N + 1))
        J, st, it = np.empty(B), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        zero = np.zeros(B)
        _lib.check(L.slocp_plan_solve(plan, _lib.dptr(Ad), _lib.dptr(Bd), _lib.dptr(dd), _lib.dptr(_lib.f64(li['x0'])), None, _lib.dptr(zero),
                                      _lib.dptr(zero), _lib.dptr(li['z']), _lib.dptr(li['zf']), _lib.dptr(li['u']), _lib.dptr(x), _lib.dptr(u),
                                      _lib.dptr(s), _lib.dptr(J), _lib.iptr(st), _lib.iptr(it)), 'slocp_plan_solve')
    finally:
        L.slocp_plan_destroy(plan)
    return x, u, J, st, it


# ---------------------------------------------------------------------------------------------------------------- preparation, solve
@pytest.mark.parametrize('name', list(LOOPS))
def test_preparation_and_solve(name):
    from sofacontrol_amd.scp.closed_loop import schedule
    from test_gusto_loop_gpu import check_window
    dt_sim, nk, ny, full = LOOPS[name]
    g = cc.g6()
    cl, inp = make_loop(name, 3)
    t_start, N = 0.1, cc.N
    cl.reset(inp['x0'], inp['x_hat0'], t_start)
    r0 = cl.step(W=inp['W'][:1], V=inp['V'][:1])
    li0, (xo0, uo0) = cl.last_inputs(), cl.last_plan()
    np.testing.assert_array_equal(li0['x0'], inp['x_hat0'])
    np.testing.assert_array_equal(r0.x[:, 0], inp['x0']); np.testing.assert_array_equal(r0.x_hat[:, 0], inp['x_hat0'])
    np.testing.assert_array_equal(r0.x_bar[:, 0], inp['x_hat0'])
    check_window('z, period 0', li0['z'], g['t'], g['zt'], t_start + inp['phase'], N + 1)
    assert (t_start + inp['phase'][0] < g['t'][0]) and (t_start + inp['phase'][2] + cc.DT * N > g['t'][-1])      # both clamped ends
    r1 = cl.step(W=inp['W'][1:2], V=inp['V'][1:2])
    li1, (xo1, uo1) = cl.last_inputs(), cl.last_plan()
    s1 = schedule(N, cc.DT, dt_sim, nk, t_start, 1)
    np.testing.assert_array_equal(li1['x0'], r0.x_bar[:, -1])
    np.testing.assert_array_equal(r1.x_bar[:, 0], r0.x_bar[:, -1])
    assert r1.t[0] == s1.t_k
    check_window('z, period 1', li1['z'], g['t'], g['zt'], s1.t_k + inp['phase'], N + 1)
    for li in (li0, li1):
        if full:
            np.testing.assert_array_equal(li['zf'], li['z'][:, -1])
        else:
            assert li['zf'] is None and li['u'] is None
    if full:
        check_window('u_des, period 1', li1['u'], g['t'], inp['ut'], s1.t_k + inp['phase'], N)
    # the loop's plan of a period = slocp_plan_solve on a second plan fed the loop's inputs, behind the chain's row-0 overwrite
    for p, (li, xo, uo, r) in enumerate(((li0, xo0, uo0, r0), (li1, xo1, uo1, r1))):
        x, u, J, st, it = second_plan_solve(cl, li)
        print('period %d: status %s, iterations %s' % (p, st, it))
        assert not st.any()
        np.testing.assert_array_equal(r.status[0], st); np.testing.assert_array_equal(r.iters[0], it); np.testing.assert_array_equal(r.J[0], J)
        np.testing.assert_array_equal(xo[:, 1:], x[:, 1:]); np.testing.assert_array_equal(xo[:, 0], li['x0']); np.testing.assert_array_equal(uo, u)
        e = cr.err(x[:, 0], li['x0'])
        print('period %d: the QP\'s own row 0 against x0: %.3e' % (p, e))
        assert e <= cr.TOL_FLOOR
    # z = H x of the records
    H = rc.controller('g6', ny, dt_sim, True)['H']
    e = cr.err(r1.z, np.einsum('ij,bsj->bsi', H.astype(cr.LD), r1.x.astype(cr.LD)))
    print('recorded z against H x: %.3e' % e)
    assert e <= cr.TOL_FLOOR


def test_member_of_a_batch_equals_the_member_alone():
    name = 'frac'
    cl, inp = make_loop(name, 3)
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    rb = cl.run(2, W=inp['W'][:2], V=inp['V'][:2])
    assert not rb.status.any()
    for b in range(3):
        one, i1 = make_loop(name, 1, member=b)
        one.reset(i1['x0'], i1['x_hat0'], 0.1)
        r = one.run(2, W=i1['W'][:2], V=i1['V'][:2])
        for f in FIELDS:
            got = getattr(rb, f)
            np.testing.assert_array_equal(got[:, b:b + 1] if f in ('iters', 'status', 'J') else got[b:b + 1], getattr(r, f), err_msg='member %d %s' % (b, f))
    assert not np.array_equal(rb.u[0], rb.u[1])


# ---------------------------------------------------------------------------------------------------------------- chain alone
@pytest.mark.parametrize('case', [c for c in rc.ADVANCE if c[0] in ('g6-knots-1', 'g6-knots-max', 'g6-5-10', 'g6-5-max', 'g6-frac-10', 'r36-5-10',
                                                                   'm8-frac-10')], ids=lambda c: c[0])
def test_chain_alone(case):
    name, mname, B, ny, dt_sim, nk = case[:6]
    cl = advance_loop(case)
    N, n, m = cc.N, cl.n_x, cl.n_u
    c = rc.chain_case(B, N, n, m, case[-1])
    assert c['status'][1] != 0 and c['status'][0] == 0
    j_end, th_end = rr.end_point(N, cc.DT, dt_sim, nk)
    for first in (True, False):
        xo, uo, xn = cl._chain(c['xsol'], c['usol'], c['x0'], c['status'], None if first else c['xprev'], None if first else c['uprev'], first=first)
        worst, worst_o = 0.0, 0.0
        for b in range(B):
            ref = rr.chain(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, j_end, th_end, cr.LD)
            f64 = rr.chain(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, j_end, th_end, np.float64)
            # copies, the row-0 overwrite and the failure shift are exact
            np.testing.assert_array_equal(xo[b], f64[0]); np.testing.assert_array_equal(uo[b], f64[1])
            np.testing.assert_array_equal(xo[b, 0], c['x0'][b])
            if c['status'][b] != 0 and first:
                assert (xo[b] == c['x0'][b]).all() and not uo[b].any()
            elif c['status'][b] != 0:
                np.testing.assert_array_equal(xo[b, 1:-1], c['xprev'][b, 2:]); np.testing.assert_array_equal(xo[b, -1], c['xprev'][b, -1])
                np.testing.assert_array_equal(uo[b, :-1], c['uprev'][b, 1:]); np.testing.assert_array_equal(uo[b, -1], c['uprev'][b, -1])
            else:
                np.testing.assert_array_equal(xo[b, 1:], c['xsol'][b, 1:]); np.testing.assert_array_equal(uo[b], c['usol'][b])
            worst_o = max(worst_o, cr.err(f64[2], ref[2])); worst = max(worst, cr.err(xn[b], ref[2]))
        print('%s first %s: (j, theta) = (%d, %.17g), request state e_oracle %.3e, device %.3e, tolerance %.3e'
              % (name, first, j_end, th_end, worst_o, worst, cr.tolerance(worst_o)))
        assert worst_o <= cr.E_ORACLE_MAX
        assert worst <= cr.tolerance(worst_o)


def short_loop():
    """The g6 loop with targets at N = 1 -- the shortest horizon slocp_plan_create accepts (scp_host.h: N >= 1) -- B = 2, and
    n_replan dt_sim = 5 * 0.01 = N dt_mpc: the next request's state is read at (j, theta) = (N - 1, 1), rows N - 1 and N of the plan."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    if 'short' not in _cache:
        g = cc.g6()
        _cache['short'] = ROMPCClosedLoopBatch(observer(rc.controller('g6', 3, 0.01, True), 2), mpc_model('g6'), 1, cc.DT,
                                               QuadraticCost(Q=g['Qz'], R=g['R']), plant('g6'), 0.01, 5, t=g['t'], z=g['zt'],
                                               U=Poly(g['U_A'], g['U_b']))
    assert rr.end_point(1, cc.DT, 0.01, 5) == (0, 1.0)
    return _cache['short']


def test_chain_alone_at_the_shortest_horizon():
    """N = 1, one member solved and one failed, first and later period: min(k + 1, N - 1) = 0 for the one input row, min(k + 1, N) = N for
    the last state row, and the request's rows j_end + 1 = N at theta == 1."""
    cl = short_loop()
    N, n, m = 1, cl.n_x, cl.n_u
    c = rc.chain_case(2, N, n, m, 77)
    assert c['status'][0] == 0 and c['status'][1] != 0
    j_end, th_end = rr.end_point(N, cc.DT, 0.01, 5)
    for first in (True, False):
        xo, uo, xn = cl._chain(c['xsol'], c['usol'], c['x0'], c['status'], None if first else c['xprev'], None if first else c['uprev'], first=first)
        worst, worst_o = 0.0, 0.0
        for b in range(2):
            ref = rr.chain(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, j_end, th_end, cr.LD)
            f64 = rr.chain(c['xsol'][b], c['usol'][b], c['x0'][b], c['status'][b], c['xprev'][b], c['uprev'][b], first, j_end, th_end, np.float64)
            np.testing.assert_array_equal(xo[b], f64[0]); np.testing.assert_array_equal(uo[b], f64[1])
            np.testing.assert_array_equal(xo[b, 0], c['x0'][b])
            if b == 1 and first:
                assert (xo[b] == c['x0'][b]).all() and not uo[b].any()
            elif b == 1:           # one row up with the last row held: the only later state row and the only input row are the last ones
                np.testing.assert_array_equal(xo[b, 1], c['xprev'][b, 1]); np.testing.assert_array_equal(uo[b, 0], c['uprev'][b, 0])
            else:
                np.testing.assert_array_equal(xo[b, 1], c['xsol'][b, 1]); np.testing.assert_array_equal(uo[b], c['usol'][b])
            worst_o = max(worst_o, cr.err(f64[2], ref[2])); worst = max(worst, cr.err(xn[b], ref[2]))
        print('N = 1, first %s: request state e_oracle %.3e, device %.3e, tolerance %.3e' % (first, worst_o, worst, cr.tolerance(worst_o)))
        assert worst_o <= cr.E_ORACLE_MAX
        assert worst <= cr.tolerance(worst_o)


def test_run_shifts_in_place_as_the_chain_alone():
    """Inside a run the shift kernel's output is the array the solve wrote (xsol is xout).  The same N = 1 loop with member 1 forced to
    fail -- its first estimate is not a number, which the interior point reports (ipm_rule.h: verdict_failed) and the request carries into
    the next period -- and member 0 solved: the plan and the next request behind each of two periods equal the stand-alone entry's
    answer, which writes into a third array, for the same inputs."""
    cl = short_loop()
    inp = loop_inputs('zf-u', 2)
    xh0 = inp['x_hat0'].copy()
    xh0[1] = np.nan
    cl.reset(inp['x0'], xh0, 0.1)
    xprev = uprev = None
    for p in range(2):
        r = cl.step()
        li, (xo, uo) = cl.last_inputs(), cl.last_plan()
        xs, us, J, st, it = second_plan_solve(cl, li)
        print('period %d: status %s' % (p, st))
        assert st[0] == 0 and st[1] != 0
        np.testing.assert_array_equal(r.status[0], st)
        ax, au, an = cl._chain(xs, us, li['x0'], st, xprev, uprev, first=p == 0)
        np.testing.assert_array_equal(xo, ax); np.testing.assert_array_equal(uo, au); np.testing.assert_array_equal(r.x_bar[:, -1], an)
        np.testing.assert_array_equal(xo[0, 1], xs[0, 1]); np.testing.assert_array_equal(xo[:, 0], li['x0'])
        assert np.isnan(xo[1]).all() and np.isfinite(xo[0]).all()
        xprev, uprev = xo, uo


# ---------------------------------------------------------------------------------------------------------------- advance alone
@pytest.mark.parametrize('case', rc.ADVANCE, ids=lambda c: c[0])
def test_advance_alone(case):
    name, mname, B, ny, dt_sim, nk, dist, noise, with_H, mode, seed = case
    c = rc.advance_case(case)
    cl = advance_loop(case)
    e_oracle, ref, f64 = rc.e_oracle(case)
    tol = cr.tolerance(e_oracle)
    got = cl._advance(c['xopt'], c['uopt'], c['x'], c['x_hat'], W=c['W'], V=c['V'], X_plant=c['X_plant'])
    errs = {k: cr.err(got[k], ref[k]) for k in rc.RECORDS}
    print('%s: e_oracle %.3e, tolerance %.3e, device %s' % (name, e_oracle, tol, ', '.join('%s %.3e' % kv for kv in errs.items())))
    assert e_oracle <= cr.E_ORACLE_MAX
    for k in rc.RECORDS:
        assert got[k].shape == ref[k].shape, k
        assert errs[k] <= tol, (k, errs[k], tol)
    if mode == 'replay':
        np.testing.assert_array_equal(got['X'], c['X_plant'][:, 1:])
    if B == 260:
        assert len({got['U'][b].tobytes() for b in range(B)}) == B


# ---------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize('name', list(LOOPS))
def test_composition(name):
    dt_sim, nk, ny, full = LOOPS[name]
    cl, inp = make_loop(name, 3)
    W, V = inp['W'], inp['V']
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    whole = cl.run(PERIODS, W=W, V=V)
    assert cl.stats() == {'steps': PERIODS, 'waits_last_run': 1}
    assert whole.x.shape == (3, PERIODS * nk + 1, 8) and whole.y.shape == (3, PERIODS * nk, ny) and whole.J.shape == (PERIODS, 3)
    print('%s: status %s, iterations %s' % (name, whole.status.ravel(), whole.iters.ravel()))
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    same(cat([cl.step(W=W[p:p + 1], V=V[p:p + 1]) for p in range(PERIODS)]), whole, 'four steps')
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    same(cat([cl.run(2, W=W[:2], V=V[:2]), cl.run(2, W=W[2:], V=V[2:])]), whole, 'two runs of two')
    assert cl.stats() == {'steps': PERIODS, 'waits_last_run': 1}
    # W = 0 equals W = None
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    a = cl.run(2, W=np.zeros_like(W[:2]), V=V[:2])
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    b = cl.run(2, V=V[:2])
    same(a, b, 'W = 0')
    nox = cl.run(1, V=V[2:3], record_x=False)
    assert nox.x is None and nox.z.shape == (3, nk + 1, 6)
    # run = the host-driven composition of its own arrows: last_inputs -> plan solve -> _chain -> _advance
    cl.reset(inp['x0'], inp['x_hat0'], 0.1)
    x, xh = inp['x0'], inp['x_hat0']
    xprev = uprev = None
    for p in range(PERIODS):
        r = cl.step(W=W[p:p + 1], V=V[p:p + 1])
        li = cl.last_inputs()
        xs, us, J, st, it = second_plan_solve(cl, li)
        xo, uo, xn = cl._chain(xs, us, li['x0'], st, xprev, uprev, first=p == 0)
        adv = cl._advance(xo, uo, x, xh, W=W[p], V=V[p])
        for f, k in (('x', 'X'), ('x_hat', 'XH'), ('z', 'Z')):
            np.testing.assert_array_equal(getattr(r, f)[:, 1:], adv[k], err_msg='period %d %s' % (p, f))
        for f, k in (('y', 'Y'), ('u', 'U'), ('u_bar', 'Ubar')):
            np.testing.assert_array_equal(getattr(r, f), adv[k], err_msg='period %d %s' % (p, f))
        np.testing.assert_array_equal(r.x_bar[:, :-1], adv['Xbar']); np.testing.assert_array_equal(r.x_bar[:, -1], xn)
        np.testing.assert_array_equal(r.J[0], J); np.testing.assert_array_equal(r.status[0], st)
        x, xh, xprev, uprev = adv['X'][:, -1], adv['XH'][:, -1], xo, uo
    # refusals that need the handle
    with pytest.raises(RuntimeError, match='exceeds max_steps_per_run'):
        cl.run(17)
    fresh, _ = make_loop(name, 3)
    with pytest.raises(RuntimeError, match='call reset first'):
        fresh.run(1)


def test_failed_solves_go_on():
    """An input box no input satisfies: every QP reports a non-zero status, the status is recorded and the loop goes on -- period 0 on
    the request state and zero inputs, later periods on the plan moved up."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    g = cc.g6()
    inp = loop_inputs('frac', 3)
    ctrl = rc.controller('g6', 30, 0.03, True)
    box = Poly(np.vstack((np.eye(3), -np.eye(3))), np.concatenate((np.full(3, -1.0), np.full(3, -1.0))))       # u <= -1 and u >= 1
    cl = ROMPCClosedLoopBatch(observer(ctrl, 3), mpc_model('g6'), cc.N, cc.DT, QuadraticCost(Q=g['Qz'], R=g['R']), plant('g6'), 0.03, 10, t=g['t'],
                              z=g['zt'], U=box)
    cl.reset(inp['x0'], inp['x_hat0'])
    r = cl.run(2)
    print('infeasible box: status %s' % r.status.ravel())
    assert r.status.all()
    xo, uo = cl.last_plan()
    assert not uo.any() and not r.u_bar.any()
    assert (xo == inp['x_hat0'][:, None]).all() and (r.x_bar == inp['x_hat0'][:, None]).all()
    assert np.isfinite(r.x).all() and np.isfinite(r.x_hat).all()


# ---------------------------------------------------------------------------------------------------------------- the reference's trace
@pytest.mark.parametrize('tag', ['tr_', 'hw_'])
def test_reference_trace(golden, tag):
    """The imported reference's ROMPC.evaluate runs replayed through the loop (B = 1, plant=None, X_plant = the reduced states of the
    recorded plant from the first active step on).  Inputs and nominal inputs are held to check_trace's 1e-6 bounds; request states and
    estimates to 10 times the distance of the host-driven ROMPC(solver_node=...) from the golden on the same trace (floor 1e-12).
    Measured on an MI355X (max|a - b|, loop / host-driven): tr_ (4 periods) request states 1.124e-15 / 1.152e-15, estimates 1.987e-14 /
    2.220e-15, u 6.9e-13 of 11.7, u_bar 1.7e-14 of 8.3; hw_ (21 periods) request states 8.604e-16 / 8.327e-16, estimates 5.151e-14 /
    2.359e-15 (above ten times the host-driven distance, inside the 1e-12 floor), u 1.6e-13 of 9.8, u_bar 2.4e-14 of 8.3.  Beside the
    summation order, the loop forms y = C x + y_ref from the reduced state where the host-driven path is handed Cf x_f: 1.4e-14 apart here."""
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    from sofacontrol_amd.utils import QuadraticCost
    from test_rompc_gpu import lin_rom, run_trace
    g = golden('g23_rompc')
    dt, nk = float(g[tag + 'dt']), int(g[tag + 'N_replan'])
    n_start = int(round(float(g[tag + 'delay']) / dt))
    model = lin_rom(g, dt)
    xr = (g[tag + 'xf'] - model.rom.x_ref) @ model.rom.V
    periods = (xr.shape[0] - n_start - 1) // nk
    S = periods * nk
    Xp = xr[None, n_start:n_start + S + 1]
    ob = DiscreteLuenbergerObserver(model, None, None, batch=1, L=g['L' if tag == 'tr_' else 'L_hw'])
    ob.K = g['K' if tag == 'tr_' else 'K_hw']
    cl = ROMPCClosedLoopBatch(ob, lin_rom(g, float(g['qp_dt'])), int(g['qp_N']), float(g['qp_dt']), QuadraticCost(Q=g['qp_Q'], R=g['qp_R']), None,
                              dt, nk, t=g['qp_t'], z=g['qp_z'], U=Poly(g['qp_UA'], g['qp_Ub']), max_steps_per_run=S)
    cl.reset(Xp[:, 0], Xp[:, 0], 0.0)
    r = cl.run(periods, X_plant=Xp)
    assert cl.stats()['waits_last_run'] == 1 and not r.status.any()
    # the parent's path on the same trace
    c, us, xs = run_trace(g, tag, 'solver_node')
    req_x_host = np.stack([q[1] for q in c.requests])
    act = slice(n_start, n_start + S)
    np.testing.assert_allclose(r.t[::nk], g[tag + 'req_t'][:periods + 1], rtol=0, atol=1e-9)
    req_x = r.x_bar[0, ::nk]                                                    # the request state of every period, and the next one's
    d_req_host = np.abs(req_x_host[:periods + 1] - g[tag + 'req_x0'][:periods + 1]).max()
    d_req = np.abs(req_x - g[tag + 'req_x0'][:periods + 1]).max()
    d_xh_host = np.abs(xs[act] - g[tag + 'xhat'][act]).max()
    d_xh = np.abs(r.x_hat[0, 1:] - g[tag + 'xhat'][act]).max()
    e_u, e_ub = np.abs(r.u[0] - g[tag + 'u'][act]).max(), np.abs(r.u_bar[0] - g[tag + 'u_opt'][:S]).max()
    print('trace %s: %d periods; u %.3e of %.3e, u_bar %.3e of %.3e; request states: loop %.3e, host-driven %.3e; estimates: loop %.3e, '
          'host-driven %.3e' % (tag, periods, e_u, np.abs(g[tag + 'u']).max(), e_ub, np.abs(g[tag + 'u_opt']).max(), d_req, d_req_host, d_xh,
                                d_xh_host))
    assert e_u <= 1e-6 * np.abs(g[tag + 'u']).max()
    assert e_ub <= 1e-6 * np.abs(g[tag + 'u_opt']).max()
    assert d_req <= max(10.0 * d_req_host, 1e-12)
    assert d_xh <= max(10.0 * d_xh_host, 1e-12)


# ---------------------------------------------------------------------------------------------------------------- the example
def test_batch_example_runs():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'diamond_rompc_closed_loop_batch.py'), '--loops', '8', '--periods', '6'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'tip error' in r.stdout and 'waits_last_run 1' in r.stdout, r.stdout[-2000:]
