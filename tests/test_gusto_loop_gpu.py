"""GPU: the batched closed loop (csrc/gusto_loop.hip, scp/closed_loop.py), every arrow of a period.

Preparation (x0, first guess, shift, target window), solve (the loop's solve against a second GuSTO fed with the loop's own inputs),
advance (loop_advance_kernel alone on the seeded plans of tests/cl_cases.py) and their composition.  Comparisons between two runs of
the same kernel on the same bits are exact; comparisons with the long-double reference (tests/cl_reference.py) use the project's rule
tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the float64 statement's own error on the same case
(asserted <= 1e-11), every figure printed before it is asserted."""
import types

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
from helpers import product_tpwl, Poly

pytestmark = pytest.mark.gpu

DT_SIMS = (0.05, 0.01, 0.03)
_cache = {}


def planner(mname):
    """The product's TPWL model with the CPU tables of cl_cases installed at every time step the cases use (so the reference reads the
    tables the kernels read), and its GuSTO adapter."""
    if ('tp', mname) not in _cache:
        from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
        m = cc.model(mname)
        tp = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        for dt in DT_SIMS:
            tp.handle_for(dt, tables=cc.tables(mname, dt))
        _cache[('tp', mname)] = (tp, TPWLGuSTO(tp))
    return _cache[('tp', mname)]


def plain_gusto(mname, B):
    """A resident plan of the model for the advance cases (no target: its own solve is not what they are about)."""
    if ('gu', mname, B) not in _cache:
        from sofacontrol_amd.scp.gusto import GuSTO
        tp, gm = planner(mname)
        n, m = gm.n_x, gm.n_u
        x0 = np.zeros((B, n)); u_init = np.zeros((B, cc.N, m))
        x_init, _ = gm.rollout(x0, u_init, cc.DT)
        xc, fc = gm.get_characteristic_vals()
        Qz = np.diag([0, 0, 0, 100., 100., 0]); R = 1e-5 * np.eye(m)
        _cache[('gu', mname, B)] = GuSTO(gm, cc.N, cc.DT, Qz, R, x0, u_init, x_init, x_char=xc, f_char=fc, convg_thresh=1e-3, batch=B,
                                         first_solve_cap=1, max_trace=0)
    return _cache[('gu', mname, B)]


def g6_gusto(B, terminal, x0):
    """The g6 problem of tests/test_gusto_gpu.py (cost, input box, characteristic values of the golden file) as a plan of B rollouts."""
    from sofacontrol_amd.scp.gusto import GuSTO
    g = cc.g6()
    tp, gm = planner('g6')
    u_init = np.zeros((B, cc.N, 3))
    x_init, _ = gm.rollout(x0, u_init, cc.DT)
    kw = dict(Qzf=2.0 * g['Qz']) if terminal else {}
    return GuSTO(gm, cc.N, cc.DT, g['Qz'], g['R'], x0, u_init, x_init, x_char=g['x_char'], f_char=g['f_char'], convg_thresh=1e-3,
                 U=Poly(g['U_A'], g['U_b']), batch=B, first_solve_cap=1, **kw)


def make_loop(name, B, member=None, max_steps_per_run=None):
    """(loop, gusto, inputs) of LOOPS[name] with B members; member = b: the B = 1 loop of member b of the three-member batch."""
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    dt_sim, n_keep, full = cc.LOOPS[name]
    g = cc.g6()
    inp = cc.loop_inputs(max(B, 3) if member is not None else B, n_keep)
    if member is not None:
        inp = dict(inp, x0=inp['x0'][member:member + 1], phase=inp['phase'][member:member + 1], W=inp['W'][:, :, member:member + 1])
    tp, gm = planner('g6')
    gu = g6_gusto(B, full, inp['x0'])
    cl = ClosedLoopBatch(gu, tp, dt_sim, n_keep, t=g['t'], z=g['zt'], u=inp['ut'] if full else None, phase=inp['phase'], K=inp['K'],
                         max_steps_per_run=max_steps_per_run)
    return cl, gu, inp


def same(a, b):
    for f in ('x', 'z', 'u', 'iters', 'status', 'J'):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def cat(rs):
    """Records of consecutive runs as one: the first row of a later run repeats the last row of the one before."""
    from sofacontrol_amd.scp.closed_loop import ClosedLoopResult
    for a, b in zip(rs[:-1], rs[1:]):
        np.testing.assert_array_equal(a.x[:, -1], b.x[:, 0]); np.testing.assert_array_equal(a.z[:, -1], b.z[:, 0])
        assert a.t[-1] == pytest.approx(b.t[0], abs=1e-12)
    return ClosedLoopResult(np.concatenate([rs[0].x] + [r.x[:, 1:] for r in rs[1:]], axis=1),
                            np.concatenate([rs[0].z] + [r.z[:, 1:] for r in rs[1:]], axis=1), np.concatenate([r.u for r in rs], axis=1),
                            np.concatenate([r.iters for r in rs]), np.concatenate([r.status for r in rs]), np.concatenate([r.J for r in rs]),
                            np.concatenate([rs[0].t] + [r.t[1:] for r in rs[1:]]))


def check_window(what, got, table_t, table_y, t0s, rows):
    worst = 0.0
    for b, t0 in enumerate(t0s):
        ref, f64 = cr.window(table_t, table_y, t0, cc.DT, rows, cr.LD), cr.window(table_t, table_y, t0, cc.DT, rows, np.float64)
        e_oracle = cr.err(f64, ref)
        e = cr.err(got[b], ref)
        print('%s member %d: e_oracle %.3e, device %.3e, tolerance %.3e' % (what, b, e_oracle, e, cr.tolerance(e_oracle)))
        assert e_oracle <= cr.E_ORACLE_MAX
        assert e <= cr.tolerance(e_oracle)


# ---------------------------------------------------------------------------------------------------------------- 3. preparation
@pytest.mark.parametrize('name', list(cc.LOOPS))
def test_preparation(name):
    from sofacontrol_amd.scp.closed_loop import schedule
    from sofacontrol_amd.scp.standalone import GuSTOSolverNode
    dt_sim, n_keep, full = cc.LOOPS[name]
    g = cc.g6()
    cl, gu, inp = make_loop(name, 3)
    tp, gm = planner('g6')
    t_start, B, N = 0.1, 3, cc.N
    cl.reset(inp['x0'], t_start)
    r0 = cl.step()
    li = cl.last_inputs()
    np.testing.assert_array_equal(li['x0'], inp['x0'])
    np.testing.assert_array_equal(r0.x[:, 0], inp['x0'])
    assert not li['u_init'].any()
    x_roll, _ = gm.rollout(inp['x0'], np.zeros((B, N, 3)), cc.DT)
    np.testing.assert_array_equal(li['x_init'], x_roll)
    check_window('z, period 0', li['z'], g['t'], g['zt'], t_start + inp['phase'], N + 1)
    assert (t_start + inp['phase'][0] < g['t'][0]) and (t_start + inp['phase'][2] + cc.DT * N > g['t'][-1])      # both clamped ends
    xo, uo = cl.last_plan()
    r1 = cl.step()
    li = cl.last_inputs()
    s1 = schedule(N, cc.DT, dt_sim, n_keep, t_start, 1)
    assert 0 < s1.idx0 <= N
    for b in range(B):
        node = types.SimpleNamespace(topt=np.arange(N + 1.0), xopt=xo[b], uopt=uo[b], N=N)
        u_ws, x_ws = GuSTOSolverNode._warm_start(node, float(s1.idx0))
        np.testing.assert_array_equal(li['u_init'][b], u_ws)
        np.testing.assert_array_equal(li['x_init'][b], x_ws)
    np.testing.assert_array_equal(li['x0'], r0.x[:, -1])
    np.testing.assert_array_equal(r1.x[:, 0], r0.x[:, -1])
    check_window('z, period 1', li['z'], g['t'], g['zt'], s1.t_k + inp['phase'], N + 1)
    if full:
        np.testing.assert_array_equal(li['zf'], li['z'][:, -1])
        check_window('u_des, period 1', li['u'], g['t'], inp['ut'], s1.t_k + inp['phase'], N)
    else:
        assert li['zf'] is None and li['u'] is None
    # z = H x of the records, the sum of zopt = H xopt
    H = np.asarray(tp.H)
    e = cr.err(r1.z, np.einsum('ij,bsj->bsi', H.astype(cr.LD), r1.x.astype(cr.LD)))
    print('recorded z against H x: %.3e' % e)
    assert e <= cr.TOL_FLOOR


# ---------------------------------------------------------------------------------------------------------------- 4. solve
@pytest.mark.parametrize('name', list(cc.LOOPS))
def test_every_solve_equals_a_second_plan_fed_the_loops_inputs(name):
    dt_sim, n_keep, full = cc.LOOPS[name]
    cl, gu, inp = make_loop(name, 3)
    g2 = g6_gusto(3, full, inp['x0'])
    g2.max_gusto_iters = gu.max_gusto_iters
    cl.reset(inp['x0'], 0.1)
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
    assert total > cc.PERIODS * 3          # the solves iterate: more than one SCP step each on average


# ---------------------------------------------------------------------------------------------------------------- 5. advance
@pytest.mark.parametrize('case', cc.ADVANCE, ids=[c[0] for c in cc.ADVANCE])
def test_advance_kernel_against_the_long_double_reference(case):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    tp, gm = planner(mname)
    c = cc.advance_case(case)
    cl = ClosedLoopBatch(plain_gusto(mname, B), tp, dt_sim, n_keep, K=c['K'])
    X, Z, U, ip, ig = cl._advance(c['xopt'], c['uopt'], c['x'], c['W'])
    H = np.asarray(tp.H)
    ref, f64 = cc.advance_reference(case, cr.LD, H=H), cc.advance_reference(case, np.float64, H=H)
    e_oracle = max(cr.err(f64[i], ref[i]) for i in range(3))
    tol = cr.tolerance(e_oracle)
    print('%s: e_oracle %.3e, least margin %.3e, tolerance %.3e' % (name, e_oracle, ref[5], tol))
    assert e_oracle <= cr.E_ORACLE_MAX and ref[5] >= cr.MARGIN
    np.testing.assert_array_equal(ip, ref[3])
    np.testing.assert_array_equal(ig, ref[4])
    worst = {}
    for what, got, want in (('x', X, ref[0]), ('u', U, ref[1]), ('z', Z, ref[2])):
        errs = [cr.err(got[:, s], want[:, s]) for s in range(n_keep)]
        worst[what] = max(errs)
        print('  %s: worst error over the sub-steps %.3e (sub-step %d)' % (what, max(errs), int(np.argmax(errs))))
    for what, e in worst.items():
        assert e <= tol, (what, e, tol)


# ---------------------------------------------------------------------------------------------------------------- 6. composition
@pytest.fixture(scope='module')
def frac_run4():
    """run(4) of the three-member 'frac' loop: (loop, gusto, inputs, result)."""
    cl, gu, inp = make_loop('frac', 3)
    cl.reset(inp['x0'], 0.1)
    return cl, gu, inp, cl.run(cc.PERIODS, W=inp['W'])


def test_run_equals_steps_and_split_runs(frac_run4):
    cl, gu, inp, r4 = frac_run4
    assert r4.x.shape == (3, 41, 8) and r4.z.shape == (3, 41, 6) and r4.u.shape == (3, 40, 3) and r4.J.shape == (4, 3)
    assert np.isfinite(r4.x).all() and np.isfinite(r4.J).all()
    np.testing.assert_allclose(r4.t, 0.1 + 0.03 * np.arange(41), rtol=0, atol=1e-12)
    cl.reset(inp['x0'], 0.1)
    same(cat([cl.run(2, W=inp['W'][:2]), cl.run(2, W=inp['W'][2:])]), r4)
    assert cl.stats()['steps'] == 4
    # step() carries no disturbance: compare without one
    cl.reset(inp['x0'], 0.1)
    r4n = cl.run(cc.PERIODS)
    cl.reset(inp['x0'], 0.1)
    same(cat([cl.step() for _ in range(cc.PERIODS)]), r4n)
    assert not np.array_equal(r4n.x, r4.x)                   # the disturbance is felt
    assert len({r4.x[b].tobytes() for b in range(3)}) == 3   # the members differ


def test_batch_members_equal_their_single_loops(frac_run4):
    _, _, inp, r4 = frac_run4
    for b in range(3):
        cl1, _, inp1 = make_loop('frac', 1, member=b)
        np.testing.assert_array_equal(inp1['x0'][0], inp['x0'][b])
        cl1.reset(inp1['x0'], 0.1)
        r1 = cl1.run(cc.PERIODS, W=inp1['W'])
        for f in ('x', 'z', 'u'):
            np.testing.assert_array_equal(getattr(r1, f)[0], getattr(r4, f)[b], err_msg='%s of member %d' % (f, b))
        for f in ('iters', 'status', 'J'):
            np.testing.assert_array_equal(getattr(r1, f)[:, 0], getattr(r4, f)[:, b], err_msg='%s of member %d' % (f, b))


def test_first_members_of_260_equal_the_batch_of_three(frac_run4):
    _, _, inp, r4 = frac_run4
    cl, gu, big = make_loop('frac', 260)
    np.testing.assert_array_equal(big['x0'][:3], inp['x0'])
    cl.reset(big['x0'], 0.1)
    r = cl.run(cc.PERIODS, W=big['W'])
    for f in ('x', 'z', 'u'):
        np.testing.assert_array_equal(getattr(r, f)[:3], getattr(r4, f), err_msg=f)
    for f in ('iters', 'status', 'J'):
        np.testing.assert_array_equal(getattr(r, f)[:, :3], getattr(r4, f), err_msg=f)
    assert len(np.unique(r.iters)) > 1          # (the key of the plan's ordered launch is not constant)


# ---------------------------------------------------------------------------------------------------------------- 7. waits
def test_one_wait_per_run_and_no_state_record(frac_run4):
    cl, gu, inp, r4 = frac_run4
    cl.reset(inp['x0'], 0.1)
    r = cl.run(cc.PERIODS, W=inp['W'], record_x=False)
    assert cl.stats() == {'steps': 4, 'waits_last_run': 1}
    assert r.x is None
    np.testing.assert_array_equal(r.z, r4.z); np.testing.assert_array_equal(r.u, r4.u)
    np.testing.assert_array_equal(r.iters, r4.iters); np.testing.assert_array_equal(r.J, r4.J)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    g = cc.g6()
    tp, gm = planner('g6')
    inp = cc.loop_inputs(3, 10)
    # a GuSTO that runs the host loop (input-rate rows on a TPWL model)
    x0 = np.zeros(8); u_init = np.zeros((cc.N, 3))
    x_init, _ = gm.rollout(x0, u_init, cc.DT)
    host = GuSTO(gm, cc.N, cc.DT, g['Qz'], g['R'], x0, u_init, x_init, x_char=g['x_char'], f_char=g['f_char'], first_solve_cap=0,
                 dU=Poly(g['U_A'], 1e3 * np.ones(6)))
    assert not host._fused
    with pytest.raises(RuntimeError, match='fused resident plan'):
        ClosedLoopBatch(host, tp, 0.01, 10)
    with pytest.raises(RuntimeError, match='fused resident plan'):
        ClosedLoopBatch(types.SimpleNamespace(_fused=True, _ssm=True), tp, 0.01, 10)
    gu = g6_gusto(3, False, inp['x0'])
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.61 exceeds the horizon N \* dt = 0\.6'):
        ClosedLoopBatch(gu, tp, 0.01, 61)
    other, _ = planner('m8')
    with pytest.raises(RuntimeError, match=r'the plant has n_x = 12, n_u = 8, the plan n_x = 8, n_u = 3'):
        ClosedLoopBatch(gu, other, 0.01, 10)
    cl = ClosedLoopBatch(gu, tp, 0.01, 10, t=g['t'], z=g['zt'], max_steps_per_run=30)
    with pytest.raises(RuntimeError, match='sgusto_loop_reset'):
        cl.run(1)
    with pytest.raises(RuntimeError, match='no period has run'):
        cl.last_inputs()
    cl.reset(inp['x0'])
    with pytest.raises(RuntimeError, match=r'periods \* n_keep = 40 exceeds max_steps_per_run = 30'):
        cl.run(4)
    r = cl.run(3)                                # the refused call left the loop as it was
    assert r.u.shape == (3, 30, 3) and cl.stats()['steps'] == 3
