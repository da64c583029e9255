"""GPU: the observed closed loop (csrc/gusto_loop.hip with a batched filter of csrc/observer.hip inside; scp/closed_loop.py
ClosedLoopBatch(observer=...)) at n_x = 8, 60 and 72 -- the filter's VALU, MFMA <60> and wide kernels.

  - advance chain: sgusto_loop_advance_observed on the seeded cases of tests/clobs_cases.py against the long-double statement of
    tests/clobs_reference.py: the three points of every sub-step equal, X, Z, U, Xhat, Y within tol = max(100 e_oracle, 1e-13) on
    max|a - b| / max(1, max|b|), e_oracle measured per case (asserted <= 1e-11 with the margins in tests/test_clobs_reference_cpu.py);
  - wiring: the solver's x0 is the recorded estimate at every period boundary, and the recorded estimates are those of a fresh
    DiscreteEKFObserverBatch fed the recorded u and y -- both bit for bit;
  - exact model: plant = filter model, x_hat0 = x0, no disturbance, no noise: x_hat stays on x within the rule;
  - composition, bit for bit, with disturbance and noise: run(P) = P x run(1) = run(P/2); run(P/2); members of B = 3 = their B = 1 loops;
    the first three members of B = 260 = the B = 3 run;
  - one host wait per run; refusals with their messages.
Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import cl_cases as cc
import clobs_cases as oc
import clobs_reference as cor
import ekf_cases as ec
from helpers import product_tpwl, Poly

pytestmark = pytest.mark.gpu

DT_SIMS = (0.05, 0.01, 0.03)
# loops: model -> (dt_sim, n_keep, periods, filter model is the plant's)
LOOPS = {'g6': (0.03, 3, 4, False), 'r30': (0.01, 3, 2, True), 'r36': (0.03, 3, 2, False)}
_cache = {}
RATIOS = {}


@pytest.fixture(scope='module', autouse=True)
def smallest_ratio():
    yield
    for name, r in sorted(RATIOS.items()):
        print('\nobserved advance %-18s: smallest tolerance / error %.1f' % (name, r), end='')
    print()


def planner(mname):
    """The product's TPWL model with the CPU tables of cl_cases installed at every time step in use, and its GuSTO adapter."""
    if ('tp', mname) not in _cache:
        from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
        m = cc.model(mname)
        tp = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        for dt in DT_SIMS:
            tp.handle_for(dt, tables=cc.tables(mname, dt))
        _cache[('tp', mname)] = (tp, TPWLGuSTO(tp))
    return _cache[('tp', mname)]


def filter_model(mname, same):
    """The product model the filters run on -- the planner's own, or the mismatched copy of clobs_cases -- with the measurement model."""
    if ('ftp', mname, same) not in _cache:
        if same:
            tp = planner(mname)[0]
        else:
            m = cc.model(mname)
            tp = product_tpwl(oc.mismatched_model(mname), m['U'], m['q_ref'], m['v_ref'], m['Hf'])
            for dt in DT_SIMS:
                t = oc.filter_tables(mname, False, dt)
                tp.handle_for(dt, tables=(t['A_d'], t['B_d'], t['d_d']))
        ms = oc.measurement(mname)
        tp.C, tp.y_ref, tp.meas_dim = ms['C'], ms['y_ref'], ms['ny']
        _cache[('ftp', mname, same)] = tp
    return _cache[('ftp', mname, same)]


def make_observer(mname, same, B):
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    ms = oc.measurement(mname)
    return DiscreteEKFObserverBatch(filter_model(mname, same), B, Sigma0=ms['Sigma0'], W=ms['W'], V=ms['V'])


def make_gusto(mname, B, x0):
    """g6: the problem of tests/test_gusto_gpu.py (cost, input box, targets come with the loop); the larger models: a plain plan with the
    iteration cap at 2 (the loop around the solve is what these tests are about)."""
    from sofacontrol_amd.scp.gusto import GuSTO
    tp, gm = planner(mname)
    n, m = gm.n_x, gm.n_u
    u_init = np.zeros((B, cc.N, m))
    x_init, _ = gm.rollout(x0, u_init, cc.DT)
    if mname == 'g6':
        g = cc.g6()
        return GuSTO(gm, cc.N, cc.DT, g['Qz'], g['R'], x0, u_init, x_init, x_char=g['x_char'], f_char=g['f_char'], convg_thresh=1e-3,
                     U=Poly(g['U_A'], g['U_b']), batch=B, first_solve_cap=1)
    xc, fc = gm.get_characteristic_vals()
    gu = GuSTO(gm, cc.N, cc.DT, np.diag([0, 0, 0, 100., 100., 0]), 1e-5 * np.eye(m), x0, u_init, x_init, x_char=xc, f_char=fc,
               convg_thresh=1e-3, batch=B, first_solve_cap=1, max_trace=0)
    gu.max_gusto_iters = 2
    return gu


def loop_inputs(mname, members):
    """x0, x_hat0 (B, n), K (P, m, n), W (periods, n_keep, B, n), V (periods, n_keep, B, n_y), phase (B): drawn per member, so a member
    has the same numbers in every batch it appears in."""
    dt_sim, n_keep, periods, same = LOOPS[mname]
    r, m, P = cc.MODELS[mname][:3]
    n, ny = 2 * r, oc.N_Y[mname]
    scale = np.abs(cc.model(mname)['model']['q']).max()
    amp = 1e-3 if mname == 'g6' else 0.05 * scale
    x0, xh0, W, V, phase = [], [], [], [], []
    for b in members:
        rng = np.random.default_rng(9000 + b)
        x0.append(amp * rng.standard_normal(n))
        xh0.append(x0[-1] + 0.3 * amp * rng.standard_normal(n))
        W.append(0.01 * amp * rng.standard_normal((periods, n_keep, n)))
        V.append(0.05 * amp * rng.standard_normal((periods, n_keep, ny)))
        phase.append(rng.uniform(-0.2, 0.4))
    K = (20.0 if mname == 'g6' else 5.0 / np.sqrt(n)) * np.random.default_rng(8999).standard_normal((P, m, n))
    return dict(x0=np.stack(x0), x_hat0=np.stack(xh0), K=K, W=np.ascontiguousarray(np.stack(W, axis=2)),
                V=np.ascontiguousarray(np.stack(V, axis=2)), phase=np.array(phase))


def make_loop(mname, members, same=None):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    dt_sim, n_keep, periods, loop_same = LOOPS[mname]
    same = loop_same if same is None else same
    inp = loop_inputs(mname, members)
    B = len(members)
    tp, gm = planner(mname)
    gu = make_gusto(mname, B, inp['x0'])
    obs = make_observer(mname, same, B)
    kw = dict(t=cc.g6()['t'], z=cc.g6()['zt'], phase=inp['phase']) if mname == 'g6' else {}
    cl = ClosedLoopBatch(gu, tp, dt_sim, n_keep, K=inp['K'], observer=obs, **kw)
    return cl, inp


FIELDS = ('x', 'z', 'u', 'iters', 'status', 'J', 'x_hat', 'y', 'ekf_status')


def same_records(a, b, members=slice(None)):
    for f in FIELDS:
        ga, gb = getattr(a, f), getattr(b, f)
        if f in ('iters', 'status', 'J', 'ekf_status'):
            np.testing.assert_array_equal(ga[:, members], gb, err_msg=f)
        else:
            np.testing.assert_array_equal(ga[members], gb, err_msg=f)


def cat(rs):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopResult
    for a, b in zip(rs[:-1], rs[1:]):
        np.testing.assert_array_equal(a.x[:, -1], b.x[:, 0]); np.testing.assert_array_equal(a.x_hat[:, -1], b.x_hat[:, 0])
    row = lambda f: np.concatenate([getattr(rs[0], f)] + [getattr(r, f)[:, 1:] for r in rs[1:]], axis=1)
    col = lambda f, ax: np.concatenate([getattr(r, f) for r in rs], axis=ax)
    return ClosedLoopResult(row('x'), row('z'), col('u', 1), col('iters', 0), col('status', 0), col('J', 0), None, x_hat=row('x_hat'),
                            y=col('y', 1), ekf_status=col('ekf_status', 0))


def loop3_of(mname):
    """(model name, loop of three members, inputs, the record of run_observed(periods) with disturbance and noise), made once."""
    if ('loop3', mname) not in _cache:
        cl, inp = make_loop(mname, (0, 1, 2))
        cl.reset_observed(inp['x0'], inp['x_hat0'], 0.1)
        r = cl.run_observed(LOOPS[mname][2], W=inp['W'], V=inp['V'])
        for f in ('x', 'x_hat', 'y', 'u', 'J'):
            assert np.isfinite(getattr(r, f)).all(), f
        assert (r.ekf_status == 0).all()
        _cache[('loop3', mname)] = (mname, cl, inp, r)
    return _cache[('loop3', mname)]


@pytest.fixture(scope='module', params=list(LOOPS))
def loop3(request):
    return loop3_of(request.param)


# ---------------------------------------------------------------------------------------------------------------- advance chain
@pytest.mark.parametrize('cs', oc.CASES, ids=oc.IDS)
def test_observed_advance_chain_against_the_long_double_reference(cs):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    name, mname, same, dt_sim, n_keep, gains, dist, noise, seed = cs
    tp, gm = planner(mname)
    c = oc.case(cs)
    obs = make_observer(mname, same, oc.B)
    cl = ClosedLoopBatch(make_gusto(mname, oc.B, np.zeros((oc.B, gm.n_x))), tp, dt_sim, n_keep, K=c['K'], observer=obs)
    got = cl._advance_observed(c['xopt'], c['uopt'], c['x'], c['x_hat'], c['W'], c['V'])
    ref, e_oracle = oc.measured(cs, H=np.asarray(tp.H))
    tol = ec.tolerance(e_oracle)
    print('%s: e_oracle %.3e, least margin %.3e, tolerance %.3e, filter kernel %s' % (name, e_oracle, ref['margin'], tol, obs.kernel_plan()['kernel']))
    assert ref['margin'] >= ec.MARGIN
    for k in ('idx_plant', 'idx_gain', 'idx_filter'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert (got['ekf_status'] == 0).all()
    worst = {}
    for k in oc.FIELDS:
        errs = [cor.err(got[k][:, s], ref[k][:, s]) for s in range(n_keep)]
        worst[k] = max(errs)
        print('  %-4s: worst error over the sub-steps %.3e (sub-step %d)' % (k, max(errs), int(np.argmax(errs))))
    RATIOS[name] = tol / max(max(worst.values()), 1e-300)
    for k, e in worst.items():
        assert e <= tol, (k, e, tol)
    with pytest.raises(RuntimeError, match='sgusto_loop_reset_observed'):          # the hook used the filters: the loop needs a reset
        cl.run_observed(1)


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_plans_start_from_the_estimate_and_the_estimate_is_the_filters(loop3):
    mname, cl, inp, r = loop3
    dt_sim, n_keep, periods, same = LOOPS[mname]
    cl.reset_observed(inp['x0'], inp['x_hat0'], 0.1)
    rs = []
    for k in range(periods):
        rs.append(cl.run_observed(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1]))
        np.testing.assert_array_equal(cl.last_inputs()['x0'], rs[-1].x_hat[:, 0])
        np.testing.assert_array_equal(rs[-1].x_hat[:, 0], r.x_hat[:, k * n_keep])
    np.testing.assert_array_equal(r.x_hat[:, 0], inp['x_hat0'])
    np.testing.assert_array_equal(r.x[:, 0], inp['x0'])
    assert not np.array_equal(r.x_hat, r.x)
    fresh = make_observer(mname, same, 3)
    fresh.initialize(inp['x_hat0'])
    for s in range(periods * n_keep):
        fresh.update(r.u[:, s], r.y[:, s], dt_sim)
        np.testing.assert_array_equal(fresh.x, r.x_hat[:, s + 1], err_msg='sub-step %d' % s)
    # y = C x + y_ref + v of the records
    ms = oc.measurement(mname)
    y = np.einsum('ij,bsj->bsi', ms['C'].astype(cor.LD), r.x[:, 1:].astype(cor.LD)) + ms['y_ref'] + np.moveaxis(inp['V'].reshape(-1, 3, ms['ny']), 0, 1)
    e = cor.err(r.y, y)
    print('%s: recorded y against C x + y_ref + v: %.3e' % (mname, e))
    assert e <= ec.tolerance(0.0)                 # the floor of the rule: a sum of n_x products against long double


# ---------------------------------------------------------------------------------------------------------------- exact model
@pytest.mark.parametrize('mname', list(LOOPS))
def test_exact_model_keeps_the_estimate_on_the_state(mname):
    dt_sim, n_keep, periods, _ = LOOPS[mname]
    cl, inp = make_loop(mname, (0, 1, 2), same=True)
    cl.reset_observed(inp['x0'], None, 0.1)
    r = cl.run_observed(periods)
    assert (r.ekf_status == 0).all()
    # e_oracle of this run: the float64 filter statement against the long-double one on the recorded u and y
    ms, filt = oc.measurement(mname), oc.filter_tables(mname, True, dt_sim)
    e_oracle = 0.0
    for b in range(3):
        xl, Sl, xd, Sd = inp['x0'][b].astype(cor.LD), ms['Sigma0'].astype(cor.LD), inp['x0'][b].copy(), ms['Sigma0'].copy()
        for s in range(periods * n_keep):
            xl, Sl, fl, margin = cor.filter_step(filt, ms['C'], ms['y_ref'], ms['W'], ms['V'], xl, Sl, r.u[b, s].astype(cor.LD), r.y[b, s].astype(cor.LD), cor.LD)
            xd, Sd, fd, _ = cor.filter_step(filt, ms['C'], ms['y_ref'], ms['W'], ms['V'], xd, Sd, r.u[b, s], r.y[b, s], np.float64)
            assert fl == fd and margin >= ec.MARGIN
            e_oracle = max(e_oracle, cor.err(xd, xl))
    tol = ec.tolerance(e_oracle)
    e = max(cor.err(r.x_hat[:, s], r.x[:, s]) for s in range(periods * n_keep + 1))
    print('%s exact model: x_hat against x %.3e | e_oracle %.3e tol %.3e' % (mname, e, e_oracle, tol))
    assert e <= tol


# ---------------------------------------------------------------------------------------------------------------- composition
def test_run_equals_single_periods_and_split_runs(loop3):
    mname, cl, inp, r = loop3
    periods, half = LOOPS[mname][2], LOOPS[mname][2] // 2
    S = periods * LOOPS[mname][1]
    assert r.x_hat.shape == r.x.shape == (3, S + 1, cl.n_x) and r.y.shape == (3, S, cl.n_y) and r.ekf_status.shape == (periods, 3)
    cl.reset_observed(inp['x0'], inp['x_hat0'], 0.1)
    same_records(cat([cl.run_observed(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1]) for k in range(periods)]), r)
    cl.reset_observed(inp['x0'], inp['x_hat0'], 0.1)
    same_records(cat([cl.run_observed(half, W=inp['W'][:half], V=inp['V'][:half]), cl.run_observed(periods - half, W=inp['W'][half:], V=inp['V'][half:])]), r)
    assert cl.stats()['steps'] == periods
    # step() and run() go through the observed loop without noise; reset() starts the estimates on the states
    cl.reset(inp['x0'], 0.1)
    rn = cl.run(periods)
    cl.reset(inp['x0'], 0.1)
    same_records(cat([cl.step() for _ in range(periods)]), rn)
    np.testing.assert_array_equal(rn.x_hat[:, 0], inp['x0'])
    assert not np.array_equal(rn.x, r.x)                                  # the disturbance, the noise and the wrong estimate are felt
    assert len({r.x_hat[b].tobytes() for b in range(3)}) == 3             # the members differ


def test_batch_members_equal_their_single_loops(loop3):
    mname, _, inp, r = loop3
    for b in range(3):
        cl1, inp1 = make_loop(mname, (b,))
        np.testing.assert_array_equal(inp1['x_hat0'][0], inp['x_hat0'][b])
        cl1.reset_observed(inp1['x0'], inp1['x_hat0'], 0.1)
        r1 = cl1.run_observed(LOOPS[mname][2], W=inp1['W'], V=inp1['V'])
        same_records(r, r1, members=slice(b, b + 1))


def test_first_members_of_260_equal_the_batch_of_three():
    """On the small model, as in tests/test_gusto_loop_gpu.py (260 filters and loops: more workgroups than CUs in every kernel of the chain)."""
    mname, _, inp, r = loop3_of('g6')
    cl, big = make_loop(mname, tuple(range(260)))
    cl.reset_observed(big['x0'], big['x_hat0'], 0.1)
    rb = cl.run_observed(LOOPS[mname][2], W=big['W'], V=big['V'])
    same_records(rb, r, members=slice(0, 3))
    assert (rb.ekf_status == 0).all()


# ---------------------------------------------------------------------------------------------------------------- waits
def test_one_wait_per_observed_run(loop3):
    mname, cl, inp, r = loop3
    cl.reset_observed(inp['x0'], inp['x_hat0'], 0.1)
    rr = cl.run_observed(LOOPS[mname][2], W=inp['W'], V=inp['V'], record_x=False)
    assert cl.stats() == {'steps': LOOPS[mname][2], 'waits_last_run': 1}
    assert rr.x is None
    np.testing.assert_array_equal(rr.x_hat, r.x_hat); np.testing.assert_array_equal(rr.y, r.y)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    tp, gm = planner('g6')
    inp = loop_inputs('g6', (0, 1, 2))
    gu = make_gusto('g6', 3, inp['x0'])
    with pytest.raises(RuntimeError, match=r'the observer has batch = 2, n_x = 8, n_u = 3; the loop needs batch = 3, n_x = 8, n_u = 3'):
        ClosedLoopBatch(gu, tp, 0.03, 3, observer=make_observer('g6', True, 2))
    with pytest.raises(RuntimeError, match=r'the observer has batch = 3, n_x = 60, n_u = 4; the loop needs batch = 3, n_x = 8, n_u = 3'):
        ClosedLoopBatch(gu, tp, 0.03, 3, observer=make_observer('r30', True, 3))
    obs = make_observer('g6', True, 3)
    cl = ClosedLoopBatch(gu, tp, 0.03, 3, observer=obs)
    with pytest.raises(RuntimeError, match='sgusto_loop_reset_observed'):
        cl.run_observed(1)
    with pytest.raises(RuntimeError, match='sgusto_loop_reset_observed'):
        cl.run(1)
    cl.reset_observed(inp['x0'], inp['x_hat0'])
    with pytest.raises(RuntimeError, match=r'V must have shape \(periods, n_keep, B, n_y\) = \(2, 3, 3, 6\), got \(2, 3, 3, 8\)'):
        cl.run_observed(2, V=np.zeros((2, 3, 3, 8)))
    with pytest.raises(RuntimeError, match=r'x_hat0 must have shape \(B, n_x\) = \(3, 8\)'):
        cl.reset_observed(inp['x0'], np.zeros((2, 8)))
    with pytest.raises(RuntimeError, match='bound to dt = 0.03 by a closed loop'):
        obs.update(np.zeros((3, 3)), np.zeros((3, 6)), 0.01)
    plain = ClosedLoopBatch(gu, tp, 0.03, 3)
    with pytest.raises(RuntimeError, match='the loop has no observer'):
        plain.run_observed(1)
    with pytest.raises(RuntimeError, match='the loop has no observer'):
        plain.reset_observed(inp['x0'])
    r = cl.run_observed(1)                      # the refused calls left the loop as it was
    assert r.x_hat.shape == (3, 4, 8) and r.ekf_status.shape == (1, 3)
