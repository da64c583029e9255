"""GPU: the chained policy of the batched closed loop -- ClosedLoopBatch(..., mpc=False), the reference's default
(tpwl/controllers.py:236, 269-274): loop_chain_kernel of csrc/gusto_loop.hip and what it feeds, without and with an observer.

The plain loops are LOOPS of tests/cl_cases.py (the g6 problem, N = 12, B = 3, PERIODS = 4), the observed loop the g6 loop of
tests/test_gusto_loop_observer_gpu.py; the kernel alone runs on the synthetic plans of every ADVANCE row.  Comparisons between two
runs of the same kernels on the same bits are exact; comparisons with the long-double statement (tests/cl_chain_reference.py) use the
project's rule tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), every figure printed before it is asserted.

The observed advance by hand (sgusto_loop_advance_observed) starts the filters from Sigma0, so it can stand for period 0 alone; the
later periods of the observed loop are checked through a fresh filter fed the recorded u and y, bit for bit."""
import types

import numpy as np
import pytest

import cl_cases as cc
import cl_chain_reference as ch
import cl_reference as cr
import test_gusto_loop_gpu as tg
import test_gusto_loop_observer_gpu as tob

pytestmark = pytest.mark.gpu

T_START = 0.1
REC = ('x', 'z', 'u', 'x_bar', 'u_bar')
PER = ('iters', 'status', 'J')


class Plain:
    """The plain loop LOOPS[name]: members (0, 1, 2), one of them alone, or the first B of 260."""
    observed = False

    def __init__(self, name='frac'):
        self.name = name
        self.dt_sim, self.n_keep, self.full = cc.LOOPS[name]
        self.rec, self.per = REC, PER

    def make(self, members=(0, 1, 2), **kw):
        from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
        g, B = cc.g6(), len(members)
        inp = cc.loop_inputs(max(B, 3), self.n_keep)
        if B < 3:
            b = members[0]
            inp = dict(inp, x0=inp['x0'][b:b + 1], phase=inp['phase'][b:b + 1], W=inp['W'][:, :, b:b + 1])
        tp, gm = tg.planner('g6')
        gu = tg.g6_gusto(B, self.full, inp['x0'])
        kw = dict(dict(mpc=False, record_tape=True), **kw)
        cl = ClosedLoopBatch(gu, tp, self.dt_sim, self.n_keep, t=g['t'], z=g['zt'], u=inp['ut'] if self.full else None, phase=inp['phase'],
                             K=inp['K'], **kw)
        return cl, gu, inp

    def reset(self, cl, inp):
        cl.reset(inp['x0'], T_START)

    def run(self, cl, inp, k0, k1, scale=1.0, **kw):
        return cl.run(k1 - k0, W=scale * inp['W'][k0:k1], **kw)


class Observed:
    """The observed g6 loop of tests/test_gusto_loop_observer_gpu.py (filter model mismatched, wrong first estimate)."""
    observed = True
    name = 'observed'

    def __init__(self):
        self.dt_sim, self.n_keep, _, self.same = tob.LOOPS['g6']
        self.full = False
        self.rec, self.per = REC + ('x_hat', 'y'), PER + ('ekf_status',)

    def make(self, members=(0, 1, 2), **kw):
        from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
        g, B = cc.g6(), len(members)
        inp = tob.loop_inputs('g6', members)
        tp, gm = tob.planner('g6')
        gu = tob.make_gusto('g6', B, inp['x0'])
        kw = dict(dict(mpc=False, record_tape=True), **kw)
        cl = ClosedLoopBatch(gu, tp, self.dt_sim, self.n_keep, t=g['t'], z=g['zt'], phase=inp['phase'], K=inp['K'],
                             observer=tob.make_observer('g6', self.same, B), **kw)
        return cl, gu, inp

    def reset(self, cl, inp):
        cl.reset_observed(inp['x0'], inp['x_hat0'], T_START)

    def run(self, cl, inp, k0, k1, scale=1.0, **kw):
        return cl.run_observed(k1 - k0, W=scale * inp['W'][k0:k1], V=scale * inp['V'][k0:k1], **kw)


KINDS = {'frac': Plain('frac'), 'zf-u': Plain('zf-u'), 'observed': Observed()}
_runs = {}


@pytest.fixture(params=list(KINDS))
def kind(request):
    return KINDS[request.param]


@pytest.fixture(params=['frac', 'observed'])
def kind2(request):
    return KINDS[request.param]


def run4(kind):
    """(loop, gusto, inputs, run(PERIODS) of the three-member loop with disturbance and noise), made once per kind."""
    if kind.name not in _runs:
        cl, gu, inp = kind.make()
        kind.reset(cl, inp)
        _runs[kind.name] = (cl, gu, inp, kind.run(cl, inp, 0, cc.PERIODS))
    return _runs[kind.name]


def same(kind, a, b, members=slice(None)):
    for f in kind.rec:
        np.testing.assert_array_equal(getattr(a, f)[members], getattr(b, f), err_msg=f)
    for f in kind.per:
        np.testing.assert_array_equal(getattr(a, f)[:, members], getattr(b, f), err_msg=f)


def cat(kind, rs):
    """Records of consecutive runs as one.  Row 0 of a later run repeats the last row of the run before -- of x_bar too (the old plan's
    end) --; the last u_bar row of a run gives way to row 0 of the next (the new plan's first input)."""
    out = types.SimpleNamespace()
    for f in kind.rec:
        parts = [getattr(r, f) for r in rs]
        if f == 'u_bar':
            v = np.concatenate([p[:, :-1] for p in parts[:-1]] + [parts[-1]], axis=1)
        elif f in ('u', 'y'):
            v = np.concatenate(parts, axis=1)
        else:
            for a, b in zip(parts[:-1], parts[1:]):
                np.testing.assert_array_equal(a[:, -1], b[:, 0], err_msg=f)
            v = np.concatenate([parts[0]] + [p[:, 1:] for p in parts[1:]], axis=1)
        setattr(out, f, v)
    for f in kind.per:
        setattr(out, f, np.concatenate([getattr(r, f) for r in rs]))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize('case', cc.ADVANCE, ids=[c[0] for c in cc.ADVANCE])
def test_chain_kernel_against_the_long_double_reference(case):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch, schedule_end
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    tp, gm = tg.planner(mname)
    c = cc.advance_case(case)
    cl = ClosedLoopBatch(tg.plain_gusto(mname, B), tp, dt_sim, n_keep, K=None, mpc=False)
    xn, xb, ub = cl._chain(c['xopt'], c['uopt'])
    assert xn.shape == (B, gm.n_x) and xb.shape == (B, n_keep + 1, gm.n_x) and ub.shape == (B, n_keep + 1, gm.n_u)
    je, te = schedule_end(cc.N, cc.DT, dt_sim, n_keep)
    lj, lt = _lib.gusto_loop_end_row(cc.N, cc.DT, dt_sim, n_keep)
    dj, dth = ch.direct_end(cc.N, cc.DT, dt_sim, n_keep)
    assert je == lj == dj and np.float64(te).tobytes() == np.float64(lt).tobytes() == np.float64(dth).tobytes()
    ref, f64 = ch.chain_case(case, cr.LD), ch.chain_case(case, np.float64)
    e_oracle = max(cr.err(f64[0], ref[0]), cr.err(f64[1], ref[1]))
    tol = cr.tolerance(e_oracle)
    ex, eu, en = cr.err(xb, ref[0]), cr.err(ub, ref[1]), cr.err(xn, ref[0][:, -1])
    print('%s: e_oracle %.3e, tolerance %.3e | x_bar rows %.3e, u_bar rows %.3e, chain point %.3e (j_end %d, theta_end %.17g)'
          % (name, e_oracle, tol, ex, eu, en, je, te))
    assert e_oracle <= cr.E_ORACLE_MAX
    assert ex <= tol and eu <= tol and en <= tol
    np.testing.assert_array_equal(xn, xb[:, -1])                              # the next start state IS the tape's end row
    np.testing.assert_array_equal(xb[:, 0], c['xopt'][:, 0])                  # theta = 0: the plan's own row
    # the tape rows have the bits the advance kernel forms: without gains its u is u_bar
    X, Z, U, ip, ig = cl._advance(c['xopt'], c['uopt'], c['x'], c['W'])
    np.testing.assert_array_equal(U, ub[:, :n_keep])


# ---------------------------------------------------------------------------------------------------------------- 2. preparation
def test_preparation(kind):
    from sofacontrol_amd.scp.closed_loop import schedule, schedule_end
    from sofacontrol_amd.scp.standalone import GuSTOSolverNode
    g, N, B, nk = cc.g6(), cc.N, 3, kind.n_keep
    cl, gu, inp = kind.make()
    kind.reset(cl, inp)
    first = inp['x_hat0'] if kind.observed else inp['x0']
    je, te = schedule_end(N, cc.DT, kind.dt_sim, nk)
    _, _, j, theta = cc.direct_schedule(N, cc.DT, kind.dt_sim, nk, 0.0, 0)
    rs, gap = [], 0.0
    for k in range(cc.PERIODS):
        prev = cl.last_plan() if k else None
        rs.append(cl.step())
        li, r = cl.last_inputs(), rs[-1]
        assert r.x_bar.shape == (B, nk + 1, 8) and r.u_bar.shape == (B, nk + 1, 3)
        xo, uo = cl.last_plan()
        np.testing.assert_array_equal(r.x[:, 0], inp['x0'] if k == 0 else rs[-2].x[:, -1])        # row 0 of the records: the plant
        s = schedule(N, cc.DT, kind.dt_sim, nk, T_START, k)
        tg.check_window('z, period %d' % k, li['z'], g['t'], g['zt'], s.t_k + inp['phase'], N + 1)
        if kind.full:
            np.testing.assert_array_equal(li['zf'], li['z'][:, -1])
            tg.check_window('u_des, period %d' % k, li['u'], g['t'], inp['ut'], s.t_k + inp['phase'], N)
        gap = max(gap, float(np.abs(xo[:, 0] - li['x0']).max()))
        if k == 0:
            np.testing.assert_array_equal(li['x0'], first)
            assert not li['u_init'].any()
            np.testing.assert_array_equal(r.x_bar[:, 0], xo[:, 0])
            continue
        # x0 is the previous plan at tau_end: row k n_keep of the tape, bit for bit, and the reference's chain point
        np.testing.assert_array_equal(li['x0'], rs[-2].x_bar[:, -1])
        np.testing.assert_array_equal(r.x_bar[:, 0], rs[-2].x_bar[:, -1])
        rows = {dt: [ch.period_rows(prev[0][b], prev[1][b], j, theta, je, te, dt) for b in range(B)] for dt in (cr.LD, np.float64)}
        pts = {dt: np.stack([v[0][-1] for v in rows[dt]]) for dt in rows}
        e_oracle = cr.err(pts[np.float64], pts[cr.LD])
        e = cr.err(li['x0'], pts[cr.LD])
        print('%s period %d: chain point e_oracle %.3e, device %.3e, tolerance %.3e' % (kind.name, k, e_oracle, e, cr.tolerance(e_oracle)))
        assert e_oracle <= cr.E_ORACLE_MAX and e <= cr.tolerance(e_oracle)
        assert not np.array_equal(li['x0'], r.x[:, 0])                                            # ... and not the plant state
        if kind.observed:
            assert not np.array_equal(li['x0'], r.x_hat[:, 0])                                    # ... nor the estimate
        assert 0 < s.idx0 <= N
        for b in range(B):
            node = types.SimpleNamespace(topt=np.arange(N + 1.0), xopt=prev[0][b], uopt=prev[1][b], N=N)
            u_ws, x_ws = GuSTOSolverNode._warm_start(node, float(s.idx0))
            np.testing.assert_array_equal(li['u_init'][b], u_ws)
            np.testing.assert_array_equal(li['x_init'][b], x_ws)
    # the junction knot: the law reads row 0 of the new plan where the reference's tape holds the old plan's end, the new plan's x0
    print('%s: max |xopt[0] - x0| over %d periods: %.3e (%s)' % (kind.name, cc.PERIODS, gap, 'bit for bit' if gap == 0.0 else 'NOT bit for bit'))
    assert gap == 0.0          # gusto_write_out copies the accepted iterate, whose row 0 the QP kernels copy from x0: the law's read at a junction
                               # is the tape's row, so the current plan stands for the tape on EVERY row


# ---------------------------------------------------------------------------------------------------------------- 3. solve
@pytest.mark.parametrize('name', list(cc.LOOPS))
def test_every_solve_equals_a_second_plan_fed_the_loops_inputs(name):
    kind = KINDS[name]
    cl, gu, inp = kind.make()
    g2 = tg.g6_gusto(3, kind.full, inp['x0'])
    g2.max_gusto_iters = gu.max_gusto_iters
    kind.reset(cl, inp)
    total = 0
    for k in range(cc.PERIODS):
        r = cl.step()
        li = cl.last_inputs()
        xo, uo = cl.last_plan()
        x2, u2, _ = g2.solve_batch(li['x0'], li['u_init'], li['x_init'], z=li['z'], zf=li['zf'], u=li['u'])
        np.testing.assert_array_equal(xo, x2); np.testing.assert_array_equal(uo, u2)
        np.testing.assert_array_equal(r.iters[0], g2.iters); np.testing.assert_array_equal(r.status[0], g2.status)
        np.testing.assert_array_equal(r.J[0], g2.costs)
        total += int(r.iters.sum())
    print('%s: %d GuSTO iterations over %d periods' % (name, total, cc.PERIODS))
    assert total > cc.PERIODS * 3          # the solves iterate: more than one SCP step each on average


# ---------------------------------------------------------------------------------------------------------------- 4. the defining property
def stepped(kind, scale, **kw):
    """The periods one by one with the noise scaled: (records, the plan of every period)."""
    cl, gu, inp = kind.make(**kw)
    kind.reset(cl, inp)
    rs, plans = [], []
    for k in range(cc.PERIODS):
        rs.append(kind.run(cl, inp, k, k + 1, scale=scale))
        plans.append(cl.last_plan())
    return rs, plans


def test_plans_do_not_depend_on_the_plant(kind2):
    kind = kind2
    (ra, pa), (rb, pb) = stepped(kind, 1.0), stepped(kind, -3.0)
    for k in range(cc.PERIODS):
        for f in PER[:3] + ('x_bar', 'u_bar'):
            np.testing.assert_array_equal(getattr(ra[k], f), getattr(rb[k], f), err_msg='%s of period %d' % (f, k))
        np.testing.assert_array_equal(pa[k][0], pb[k][0]); np.testing.assert_array_equal(pa[k][1], pb[k][1])
        assert not np.array_equal(ra[k].x[:, 1:], rb[k].x[:, 1:])                     # the plants went different ways
        assert not np.array_equal(ra[k].u, rb[k].u)                                   # ... and the law answered
    # the same pair under mpc=True: the plans part from period 1 on (the case above is not vacuous)
    (_, pa), (_, pb) = stepped(kind, 1.0, mpc=True, record_tape=False), stepped(kind, -3.0, mpc=True, record_tape=False)
    np.testing.assert_array_equal(pa[0][0], pb[0][0])
    for k in range(1, cc.PERIODS):
        assert not np.array_equal(pa[k][0], pb[k][0]) and not np.array_equal(pa[k][1], pb[k][1]), k


# ---------------------------------------------------------------------------------------------------------------- 5. advance
def test_advance_of_a_chained_period_equals_the_kernel_by_hand():
    kind = KINDS['frac']
    cl, gu, inp = kind.make()
    kind.reset(cl, inp)
    rs, plans = [], []
    for k in range(cc.PERIODS):
        rs.append(kind.run(cl, inp, k, k + 1))
        plans.append(cl.last_plan())
    for k in range(cc.PERIODS):
        X, Z, U, ip, ig = cl._advance(plans[k][0], plans[k][1], rs[k].x[:, 0], inp['W'][k])
        np.testing.assert_array_equal(X, rs[k].x[:, 1:], err_msg='x of period %d' % k)
        np.testing.assert_array_equal(Z, rs[k].z[:, 1:], err_msg='z of period %d' % k)
        np.testing.assert_array_equal(U, rs[k].u, err_msg='u of period %d' % k)
        # the tape of the period is the kernel's on the period's plan
        xn, xb, ub = cl._chain(plans[k][0], plans[k][1])
        np.testing.assert_array_equal(xb[:, 1:], rs[k].x_bar[:, 1:]); np.testing.assert_array_equal(ub, rs[k].u_bar)


def test_observed_advance_of_a_chained_loop():
    kind = KINDS['observed']
    cl, gu, inp, r = run4(kind)
    nk = kind.n_keep
    # the later periods: the recorded estimates are those of a fresh filter fed the recorded u and y
    fresh = tob.make_observer('g6', kind.same, 3)
    fresh.initialize(inp['x_hat0'])
    for s in range(cc.PERIODS * nk):
        fresh.update(r.u[:, s], r.y[:, s], kind.dt_sim)
        np.testing.assert_array_equal(fresh.x, r.x_hat[:, s + 1], err_msg='sub-step %d' % s)
    assert (r.ekf_status == 0).all()
    # period 0 by hand
    cl2, _, _ = kind.make()
    kind.reset(cl2, inp)
    r0 = kind.run(cl2, inp, 0, 1)
    xo, uo = cl2.last_plan()
    got = cl2._advance_observed(xo, uo, inp['x0'], inp['x_hat0'], inp['W'][0], inp['V'][0])
    for f, want in (('X', r0.x[:, 1:]), ('Z', r0.z[:, 1:]), ('U', r0.u), ('Xhat', r0.x_hat[:, 1:]), ('Y', r0.y)):
        np.testing.assert_array_equal(got[f], want, err_msg=f)
    for f in kind.rec:                              # (the one-period run is the first period of the run of four)
        rows = nk if f in ('u', 'y', 'u_bar') else nk + 1
        np.testing.assert_array_equal(getattr(r0, f)[:, :rows], getattr(r, f)[:, :rows], err_msg=f)
    # the law of every sub-step of every period from the tape: u = u_bar + K[i] (x_hat - x_bar), i = the planner's point nearest x_bar
    planner = cc.table_dict('g6')
    worst = 0.0
    for b in range(3):
        for s in range(cc.PERIODS * nk):
            k, i = divmod(s, nk)
            xbar = r.x_bar[b, s].astype(cr.LD)
            if i == 0 and k > 0:
                continue                                    # junction: the kernel read the new plan's row 0 (= this row, see test_preparation)
            gidx, _ = cr.nearest_with_margin(planner['q'], planner['v'], planner['w_q'], planner['w_v'], xbar, cr.LD)
            u = r.u_bar[b, s].astype(cr.LD) + inp['K'][gidx].astype(cr.LD) @ (r.x_hat[b, s].astype(cr.LD) - xbar)
            worst = max(worst, cr.err(r.u[b, s], u))
    print('observed: recorded u against u_bar + K (x_hat - x_bar) from the tape: %.3e' % worst)
    assert worst <= cr.TOL_FLOOR                     # the floor of the rule: one sum of n_x products against long double


# ---------------------------------------------------------------------------------------------------------------- 6. composition
def test_run_equals_steps_and_split_runs(kind2):
    kind = kind2
    cl, gu, inp, r4 = run4(kind)
    S = cc.PERIODS * kind.n_keep
    assert r4.x_bar.shape == (3, S + 1, 8) and r4.u_bar.shape == (3, S + 1, 3) and r4.u.shape == (3, S, 3)
    assert all(np.isfinite(getattr(r4, f)).all() for f in kind.rec)
    kind.reset(cl, inp)
    same(kind, cat(kind, [kind.run(cl, inp, 0, 2), kind.run(cl, inp, 2, 4)]), r4)
    assert cl.stats()['steps'] == 4
    kind.reset(cl, inp)
    same(kind, cat(kind, [kind.run(cl, inp, k, k + 1) for k in range(cc.PERIODS)]), r4)
    # step(): no disturbance
    kind.reset(cl, inp)
    r4n = cl.run(cc.PERIODS)
    kind.reset(cl, inp)
    same(kind, cat(kind, [cl.step() for _ in range(cc.PERIODS)]), r4n)
    np.testing.assert_array_equal(r4n.x_bar, r4.x_bar)                    # the tape does not feel the disturbance
    assert not np.array_equal(r4n.x, r4.x)                                # the plant does
    assert len({r4.x_bar[b].tobytes() for b in range(3)}) == 3            # the members differ
    # one wait per run, with and without the state record; the tape on its own switch
    kind.reset(cl, inp)
    r = kind.run(cl, inp, 0, cc.PERIODS, record_x=False)
    assert cl.stats() == {'steps': 4, 'waits_last_run': 1} and r.x is None
    np.testing.assert_array_equal(r.x_bar, r4.x_bar); np.testing.assert_array_equal(r.u, r4.u)
    cl.set_record_tape(False)
    kind.reset(cl, inp)
    r = kind.run(cl, inp, 0, cc.PERIODS)
    cl.set_record_tape(True)
    assert r.x_bar is None and r.u_bar is None and cl.stats() == {'steps': 4, 'waits_last_run': 1}
    np.testing.assert_array_equal(r.x, r4.x); np.testing.assert_array_equal(r.J, r4.J)
    # a reset drops the chain: period 0 again starts from the plant state (the estimate)
    kind.reset(cl, inp)
    cl.step()
    np.testing.assert_array_equal(cl.last_inputs()['x0'], inp['x_hat0'] if kind.observed else inp['x0'])


def test_batch_members_equal_their_single_loops(kind2):
    kind = kind2
    _, _, inp, r4 = run4(kind)
    for b in range(3):
        cl1, _, inp1 = kind.make(members=(b,))
        np.testing.assert_array_equal(inp1['x0'][0], inp['x0'][b])
        kind.reset(cl1, inp1)
        same(kind, r4, kind.run(cl1, inp1, 0, cc.PERIODS), members=slice(b, b + 1))


def test_first_members_of_260_equal_the_batch_of_three(kind2):
    kind = kind2
    _, _, inp, r4 = run4(kind)
    cl, gu, big = kind.make(members=tuple(range(260)))
    np.testing.assert_array_equal(big['x0'][:3], inp['x0'])
    kind.reset(cl, big)
    r = kind.run(cl, big, 0, cc.PERIODS)
    same(kind, r, r4, members=slice(0, 3))
    assert len({r.x_bar[b].tobytes() for b in range(260)}) == 260


# ---------------------------------------------------------------------------------------------------------------- 7. mpc=True untouched
def test_mpc_true_is_the_default_and_untouched():
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    kind = KINDS['zf-u']
    g = cc.g6()
    cl, gu, inp = kind.make(mpc=True, record_tape=False)
    kind.reset(cl, inp)
    r = kind.run(cl, inp, 0, cc.PERIODS)
    assert r.x_bar is None and r.u_bar is None and cl.mpc is True
    tp, gm = tg.planner('g6')
    dflt = ClosedLoopBatch(tg.g6_gusto(3, True, inp['x0']), tp, kind.dt_sim, kind.n_keep, t=g['t'], z=g['zt'], u=inp['ut'], phase=inp['phase'], K=inp['K'])
    assert dflt.mpc is True and dflt.record_tape is False
    dflt.reset(inp['x0'], T_START)
    tg.same(dflt.run(cc.PERIODS, W=inp['W']), r)
    np.testing.assert_array_equal(dflt.last_inputs()['x0'], r.x[:, 3 * kind.n_keep])      # re-planned from the plant
    # ... and the chained loop on the same inputs is another loop from period 1 on
    ch_cl, _, _ = kind.make()
    kind.reset(ch_cl, inp)
    rc = kind.run(ch_cl, inp, 0, cc.PERIODS)
    np.testing.assert_array_equal(rc.J[0], r.J[0])
    assert not np.array_equal(rc.J[1:], r.J[1:])


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    import ctypes as C
    kind = KINDS['frac']
    cl, gu, inp = kind.make()
    with pytest.raises(RuntimeError, match='record_tape=True needs mpc=False'):
        kind.make(mpc=True, record_tape=True)
    mp, _, _ = kind.make(mpc=True, record_tape=False)
    with pytest.raises(RuntimeError, match='record_tape=True needs mpc=False'):
        mp.set_record_tape(True)
    mp.reset(inp['x0'])
    with pytest.raises(RuntimeError, match=r'sgusto_loop_run_tape: the loop re-plans from the plant \(mpc=True\)'):
        mp.record_tape = True                   # past the Python check: the library refuses too
        mp.run(1)
    mp.record_tape = False
    assert mp.run(1).x_bar is None              # the refused call left the loop as it was
    with pytest.raises(RuntimeError, match=r'sgusto_loop_set_chained: 1 period\(s\) have run since the last reset'):
        mp._call('_set_chained', C.c_int(1))
    mp.reset(inp['x0'])
    mp._call('_set_chained', C.c_int(1))        # in front of the first period it is taken
    mp._call('_set_chained', C.c_int(0))
    with pytest.raises(RuntimeError, match='sgusto_loop_reset'):
        cl.run(1)
    with pytest.raises(RuntimeError, match=r'_chain: xopt must have shape \(B, N \+ 1, n_x\) = \(3, 13, 8\) and uopt \(B, N, n_u\) = \(3, 12, 3\), got '
                                           r'\(3, 12, 8\) and \(3, 12, 3\)'):
        cl._chain(np.zeros((3, 12, 8)), np.zeros((3, 12, 3)))
    with pytest.raises(RuntimeError, match=r'_chain: xopt must have shape'):
        cl._chain(np.zeros((3, 13, 8)), np.zeros((2, 12, 3)))
    small, _, _ = kind.make(max_steps_per_run=30)
    small.reset(inp['x0'])
    with pytest.raises(RuntimeError, match=r'periods \* n_keep = 40 exceeds max_steps_per_run = 30'):
        small.run(4)
    r = small.run(3)
    assert r.x_bar.shape == (3, 31, 8) and small.stats()['steps'] == 3
