"""GPU: the SSM closed loop on a TPWL plant (csrc/gusto_ssm_loop.hip: ssm_loop_advance_tpwl_kernel, SSMClosedLoopBatch.on_plant).

Advance: the kernel alone on the seeded cases of tests/ssm_loop_tpwl_cases.py against the long-double chain of
tests/ssm_loop_tpwl_reference.py -- the project's rule tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the float64
chain's own error on the same case (asserted <= 1e-11), every figure printed before it is asserted; the points picked are the
reference's exactly -- and, bit for bit, against the plant states and inputs of scp.closed_loop's stand-alone advance without gains (the
step rule is one rule).  Whole loops: the hardware driver's planner (n_x = 6, n_u = 4, cubic / quadratic, be, N = 3, dt = 0.02, U box,
max_gusto_iters = 0) on the r36 plant (n_p = 72) at dt_sim = 0.01, n_keep = 2, measured through a seeded C (6 x 72), 4 periods; comparisons
between two runs of the same kernels on the same bits are exact."""
import ctypes as C

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import ssm_cases as sc
import ssm_loop_tpwl_cases as stc
import ssm_reference as sr
from oracle import ssm as ossm
from oracle import tpwl as otpwl
from helpers import golden_problem, product_tpwl
from test_ssm_gpu import product_ssm

pytestmark = pytest.mark.gpu

PERIODS = 4
T_START = 0.1
SHAPE, SEED, METHOD, N, DT, DT_SIM, NK = (6, 4, 3, 2), 96, 'be', 3, 0.02, 0.01, 2
PLANT = 'r36'
_cache = {}


def tpwl_plant(mname):
    import test_gusto_loop_gpu as tl
    return tl.planner(mname)[0]


def observer(shape):
    if ('obs', shape) not in _cache:
        _cache[('obs', shape)] = product_ssm(sc.oracle_model(stc.observer_model(shape)), discr='fe')
    return _cache[('obs', shape)]


# ---------------------------------------------------------------------------------------------------------------- 1. advance
@pytest.mark.parametrize('pair', stc.PAIRS, ids=[stc.case_id(p) for p in stc.PAIRS])
def test_advance_kernel_against_the_long_double_chain(pair):
    """Measured on the MI355X: the figures are in DESIGN.md section 44."""
    from sofacontrol_amd.scp import closed_loop_ssm
    i, r = stc.inputs(pair), stc.reference(pair)
    got = closed_loop_ssm.advance_tpwl(tpwl_plant(i['model']), i['C'], i['y_ref'], observer(pair[1]), i['dt_sim'], i['N'], i['j'], i['theta'],
                                       i['uopt'], i['x'], W=i['W'], V=i['V'])
    eo = max(r['e_oracle'].values())
    print('%s: e_oracle %.3e, least margin %.3e' % (stc.case_id(pair), eo, r['margin']))
    assert r['margin'] > cr.MARGIN
    for f in stc.FIELDS:
        assert r['e_oracle'][f] <= cr.E_ORACLE_MAX, (f, r['e_oracle'][f])
    assert got['idx'].dtype == np.int32
    np.testing.assert_array_equal(got['idx'], r['picks'])
    worst = {}
    for f in stc.FIELDS:
        tol = cr.tolerance(r['e_oracle'][f])
        errs = [cr.err(got[f][:, q], r['ref'][f][:, q]) for q in range(i['n_keep'])]
        worst[f] = (max(errs), tol)
        print('  %s: e_oracle %.3e, worst error over the sub-steps %.3e (sub-step %d), tolerance %.3e' % (f, r['e_oracle'][f], max(errs),
                                                                                                       int(np.argmax(errs)), tol))
    for f, (e, tol) in worst.items():
        assert e <= tol, (f, e, tol)
    np.testing.assert_array_equal(got['Y'], (got['Z'] + i['y_ref']) + i['V'].transpose(1, 0, 2))


CL_CASES = sorted({p[0] for p in stc.PAIRS}, key=[c[0] for c in cc.ADVANCE].index)


@pytest.mark.parametrize('name', CL_CASES)
def test_plant_states_and_inputs_equal_the_tpwl_loops_advance_without_gains(name):
    """The step rule shared: X and U are, bit for bit, those of loop_advance_kernel (scp.closed_loop) with K = None on the same inputs."""
    import test_gusto_loop_gpu as tl
    from sofacontrol_amd.scp import closed_loop_ssm
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    pair = [p for p in stc.PAIRS if p[0] == name][0]
    i = stc.inputs(pair)
    c = cc.advance_case(stc.cl_case(pair))
    tp = tpwl_plant(i['model'])
    got = closed_loop_ssm.advance_tpwl(tp, i['C'], i['y_ref'], observer(pair[1]), i['dt_sim'], i['N'], i['j'], i['theta'], i['uopt'], i['x'],
                                       W=i['W'], V=i['V'])
    cl = ClosedLoopBatch(tl.plain_gusto(i['model'], i['B']), tp, i['dt_sim'], i['n_keep'])
    X, Z, U, ip, ig = cl._advance(c['xopt'], c['uopt'], c['x'], c['W'])
    assert np.isfinite(X).all() and U.any()
    np.testing.assert_array_equal(got['X'], X)
    np.testing.assert_array_equal(got['U'], U)
    np.testing.assert_array_equal(got['idx'], ip)
    assert (ig == -1).all()


# ---------------------------------------------------------------------------------------------------------------- 2. whole loops
def models():
    """(oracle model dict of the planner, planner SSMDynamics, the TPWL plant with its tables at DT_SIM)."""
    if 'm' not in _cache:
        model = ossm.synthetic(*SHAPE, seed=SEED)
        _cache['m'] = (model, product_ssm(model, discr=METHOD), tpwl_plant(PLANT))
    return _cache['m']


def inputs(B):
    """x0 (B, 72), v0 (B, 6), phase (B,), W (PERIODS, NK, B, 72), V (PERIODS, NK, B, 6), C (6, 72), y_ref (6), the tables t, zt (T, 6):
    members 0..2 are the same for every B >= 3 and differ; member 0 asks for targets before t[0], member 2 behind t[-1]."""
    model = models()[0]
    n, n_p, big = SHAPE[0], 2 * cc.MODELS[PLANT][0], 260
    mdl = cc.model(PLANT)['model']
    rng = np.random.default_rng(5200 + SEED)
    scale = np.abs(mdl['q']).max()
    pts = rng.integers(0, mdl['q'].shape[0], big)
    x0 = np.concatenate((0.05 * scale * rng.standard_normal((big, n_p // 2)), mdl['q'][pts] + 0.1 * scale * rng.standard_normal((big, n_p // 2))), axis=1)
    Cm = rng.standard_normal((n, n_p))
    Cm *= 0.05 / np.abs(x0[:3] @ Cm.T).max()
    y_ref = model['z_ref'] + 0.01 * rng.standard_normal(n)
    v0 = 1e-3 * rng.standard_normal((big, n))
    phase = np.concatenate([[-0.5, 0.2, 1.2], rng.uniform(0.0, 0.8, big - 3)])
    W = 1e-3 * scale * rng.standard_normal((PERIODS, NK, big, n_p)); V = 1e-3 * rng.standard_normal((PERIODS, NK, big, n))
    t = np.linspace(0.0, 1.0, 31)
    zt = np.zeros((31, n)); zt[:, 0] = 0.02 * np.sin(2 * np.pi * t); zt[:, 1] = -0.01 * np.cos(2 * np.pi * t); zt[:, 2] = 0.015 * t
    zt = zt + ossm.observe(model, np.zeros(n))
    return dict(x0=x0[:B], v0=v0[:B], phase=phase[:B], W=np.ascontiguousarray(W[:, :, :B]), V=np.ascontiguousarray(V[:, :, :B]), C=Cm, y_ref=y_ref,
                t=t, zt=zt)


def make_gusto(B, keep=False, dU=None):
    """make_gusto('hw', ...) of tests/test_gusto_ssm_loop_gpu.py, re-stated: the hardware driver's plan."""
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import HyperRectangle
    n, m = SHAPE[:2]
    model, planner, _ = models()
    x0 = np.zeros((B, n))
    u_init = np.zeros((B, N, m))
    x_init, _ = planner.rollout(x0, u_init, DT)
    z = np.tile(ossm.observe(model, np.zeros(n)), (B, N + 1, 1))
    Qz = np.zeros((n, n)); Qz[0, 0] = Qz[1, 1] = Qz[2, 2] = 100.0
    g = GuSTO(SSMGuSTO(planner), N, DT, Qz, 1e-3 * np.eye(m), x0, u_init, x_init, z=z, verbose=0, max_gusto_iters=0, batch=B, first_solve_cap=1,
              max_trace=0, keep_solver_state=keep, dU=dU, U=HyperRectangle([3.0] * m, [-1.0] * m), convg_thresh=1e-5)
    assert g._ssm
    return g


def make_loop(B, member=None, max_steps_per_run=None):
    """(loop, gusto, inputs) with B members; member = b: the B = 1 loop of member b of the three-member batch."""
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    inp = inputs(max(B, 3) if member is not None else B)
    if member is not None:
        sl = slice(member, member + 1)
        inp = dict(inp, x0=inp['x0'][sl], v0=inp['v0'][sl], phase=inp['phase'][sl], W=np.ascontiguousarray(inp['W'][:, :, sl]),
                   V=np.ascontiguousarray(inp['V'][:, :, sl]))
    gu = make_gusto(B)
    cl = SSMClosedLoopBatch.on_plant(gu, models()[2], DT_SIM, NK, t=inp['t'], z=inp['zt'], phase=inp['phase'], max_steps_per_run=max_steps_per_run,
                                     C=inp['C'], y_ref=inp['y_ref'])
    return cl, gu, inp


FIELDS = ('x', 'z', 'u', 'y', 'x_hat', 'iters', 'status', 'J')


def same(a, b, fields=FIELDS):
    for f in fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def cat(rs):
    """Records of consecutive runs as one: the first row of a later run repeats the last row of the one before."""
    from sofacontrol_amd.scp.closed_loop import ClosedLoopResult
    for a, b in zip(rs[:-1], rs[1:]):
        for f in ('x', 'z', 'y', 'x_hat'):
            np.testing.assert_array_equal(getattr(a, f)[:, -1], getattr(b, f)[:, 0], err_msg=f)
        assert a.t[-1] == pytest.approx(b.t[0], abs=1e-12)
    rows = lambda f: np.concatenate([getattr(rs[0], f)] + [getattr(r, f)[:, 1:] for r in rs[1:]], axis=1)
    return ClosedLoopResult(rows('x'), rows('z'), np.concatenate([r.u for r in rs], axis=1), np.concatenate([r.iters for r in rs]),
                            np.concatenate([r.status for r in rs]), np.concatenate([r.J for r in rs]),
                            np.concatenate([rs[0].t] + [r.t[1:] for r in rs[1:]]), x_hat=rows('x_hat'), y=rows('y'))


@pytest.fixture(scope='module')
def run4():
    """run(4) of the three-member loop with W and V: (loop, gusto, inputs, result)."""
    cl, gu, inp = make_loop(3)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    return cl, gu, inp, cl.run(PERIODS, W=inp['W'], V=inp['V'])


def test_every_solve_equals_a_second_plan_and_starts_from_the_last_estimate():
    from test_gusto_ssm_loop_gpu import plan_costs
    cl, gu, inp = make_loop(3)
    g2 = make_gusto(3)
    g2.max_gusto_iters = gu.max_gusto_iters
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    prev = None
    for k in range(PERIODS):
        r = cl.run(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1])
        li = cl.last_inputs()
        xo, uo = cl.last_plan()
        # the plans start from the estimate: the reset's first one, then the one the period before ended with
        np.testing.assert_array_equal(li['x0'], r.x_hat[:, 0])
        if prev is not None:
            np.testing.assert_array_equal(li['x0'], prev.x_hat[:, -1])
        x2, u2, _ = g2.solve_batch(li['x0'], li['u_init'], li['x_init'], z=li['z'], u=li['u'])
        np.testing.assert_array_equal(xo, x2); np.testing.assert_array_equal(uo, u2)
        np.testing.assert_array_equal(r.iters[0], g2.iters); np.testing.assert_array_equal(r.status[0], g2.status)
        np.testing.assert_array_equal(r.J[0], plan_costs(g2))
        prev = r


def test_row_0_is_the_resets_first_observer_update(run4):
    cl, gu, inp, r4 = run4
    _, planner, _ = models()
    assert r4.x.shape == (3, 9, 72) and r4.z.shape == (3, 9, 6) and r4.y.shape == (3, 9, 6) and r4.x_hat.shape == (3, 9, 6)
    assert r4.u.shape == (3, 8, 4) and r4.J.shape == (4, 3)
    assert all(np.isfinite(getattr(r4, f)).all() for f in FIELDS)
    np.testing.assert_allclose(r4.t, T_START + DT_SIM * np.arange(9), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(r4.x[:, 0], inp['x0'])
    e = sr.err(r4.z[:, 0], inp['x0'] @ inp['C'].T)
    print('row 0 of z against C x0: %.3e' % e)
    assert e <= cr.TOL_FLOOR
    np.testing.assert_array_equal(r4.y[:, 0], (r4.z[:, 0] + inp['y_ref']) + inp['v0'])
    # every row: z = C x, y = (z + y_ref) + v, x_hat = W_map(y - z_ref) of the controller's model
    e = sr.err(r4.z, r4.x @ inp['C'].T)
    print('z against C x (all rows): %.3e' % e)
    assert e <= cr.TOL_FLOOR
    np.testing.assert_array_equal(r4.y[:, 1:], (r4.z[:, 1:] + inp['y_ref']) + inp['V'].reshape(PERIODS * NK, 3, 6).transpose(1, 0, 2))
    for rows in (0, slice(None)):
        y = r4.y[:, rows].reshape(-1, 6)
        e = sr.err(r4.x_hat[:, rows].reshape(-1, 6), planner.observed_to_reduced((y - planner.z_ref).T).T)
        print('x_hat against W_map of y (rows %s): %.3e' % (rows, e))
        assert e <= cr.TOL_FLOOR
    assert len({r4.x[b].tobytes() for b in range(3)}) == 3 and r4.u.any()


def test_run_equals_steps_and_split_runs(run4):
    cl, gu, inp, r4 = run4
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    same(cat([cl.run(2, W=inp['W'][:2], V=inp['V'][:2]), cl.run(2, W=inp['W'][2:], V=inp['V'][2:])]), r4)
    assert cl.stats()['steps'] == 4
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    same(cat([cl.run(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1]) for k in range(PERIODS)]), r4)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    r4n = cl.run(PERIODS)
    assert not np.array_equal(r4n.x, r4.x) and not np.array_equal(r4n.y, r4.y)      # disturbance and noise are felt


def test_batch_members_equal_their_single_loops(run4):
    _, _, inp, r4 = run4
    for b in range(3):
        cl1, _, inp1 = make_loop(1, member=b)
        np.testing.assert_array_equal(inp1['x0'][0], inp['x0'][b])
        cl1.reset(inp1['x0'], T_START, v0=inp1['v0'])
        r1 = cl1.run(PERIODS, W=inp1['W'], V=inp1['V'])
        for f in ('x', 'z', 'u', 'y', 'x_hat'):
            np.testing.assert_array_equal(getattr(r1, f)[0], getattr(r4, f)[b], err_msg='%s of member %d' % (f, b))
        for f in ('iters', 'status', 'J'):
            np.testing.assert_array_equal(getattr(r1, f)[:, 0], getattr(r4, f)[:, b], err_msg='%s of member %d' % (f, b))


def test_first_members_of_260_equal_the_batch_of_three(run4):
    _, _, inp, r4 = run4
    cl, gu, big = make_loop(260)
    np.testing.assert_array_equal(big['x0'][:3], inp['x0'])
    cl.reset(big['x0'], T_START, v0=big['v0'])
    r = cl.run(PERIODS, W=big['W'], V=big['V'])
    for f in ('x', 'z', 'u', 'y', 'x_hat'):
        np.testing.assert_array_equal(getattr(r, f)[:3], getattr(r4, f), err_msg=f)
    for f in ('iters', 'status', 'J'):
        np.testing.assert_array_equal(getattr(r, f)[:, :3], getattr(r4, f), err_msg=f)


def test_one_wait_per_run(run4):
    cl, gu, inp, r4 = run4
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    r = cl.run(PERIODS, W=inp['W'], V=inp['V'], record_x=False)
    assert cl.stats() == {'steps': 4, 'waits_last_run': 1}
    assert r.x is None
    same(r, r4, fields=[f for f in FIELDS if f != 'x'])


def test_interleaved_ssm_plant_and_tpwl_plant_loops_equal_each_loop_alone():
    """Both plant kinds are one handle type on one host shell: an SSM-plant loop and a TPWL-plant loop driven in turn give the records,
    bit for bit, of the same runs of each loop alone."""
    import test_gusto_ssm_loop_gpu as ts

    def on_ssm():
        cl, _, inp = ts.make_loop('frac', 3)
        cl.reset(inp['x0'], T_START, v0=inp['v0'])
        return cl, lambda k: cl.run(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1])

    def on_tpwl():
        cl, _, inp = make_loop(3)
        cl.reset(inp['x0'], T_START, v0=inp['v0'])
        return cl, lambda k: cl.run(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1])

    (cs, rs), (ct, rt) = on_ssm(), on_tpwl()
    alone_s, alone_t = [rs(0), rs(1)], [rt(0), rt(1)]
    (cs, rs), (ct, rt) = on_ssm(), on_tpwl()
    mixed = [rs(0), rt(0), rs(1), rt(1)]
    assert cs.stats() == {'steps': 2, 'waits_last_run': 1} and ct.stats() == {'steps': 2, 'waits_last_run': 1}
    for k in range(2):
        ts.same(mixed[2 * k], alone_s[k])
        same(mixed[2 * k + 1], alone_t[k])
    assert not np.array_equal(alone_s[0].x, alone_s[1].x) and not np.array_equal(alone_t[0].x, alone_t[1].x)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def big_plant():
    """A nearest-point TPWL model of n_p = 128 states and eight inputs with its tables at 0.01."""
    if 'big' not in _cache:
        mdl, U, q_ref, v_ref, Hf = golden_problem(64, 8, 3, 30, 57, q_scale=0.1)
        tp = product_tpwl(mdl, U, q_ref, v_ref, Hf)
        tp.handle_for(0.01, tables=otpwl.pre_discretize(mdl, 0.01, 'zoh'))
        _cache['big'] = tp
    return _cache['big']


def test_refusals_on_the_device():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp import closed_loop_ssm
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    lib = _lib.lib()
    inp = inputs(3)
    _, planner, plant = models()
    gu = make_gusto(3)
    # LDS: the panel of an n_p = 128 plant (131 KB) with a 12 x 90 observer and C 12 x 128
    big, obs = big_plant(), observer((12, 8, 2, 2))
    assert big.get_state_dim() == 128
    j, theta = np.zeros(2, dtype=np.int32), np.array([0.0, 0.5])
    with pytest.raises(RuntimeError, match=r'sgusto_ssm_loop_advance_tpwl: the advance kernel needs 168496 bytes of LDS .*n_x = 128.*12 x 90.*163840 available'):
        closed_loop_ssm.advance_tpwl(big, np.zeros((12, 128)), np.zeros(12), obs, 0.01, 3, j, theta, np.zeros((1, 3, 8)), np.zeros((1, 128)))
    # the same plant under a small observer fits, and runs
    small = observer((10, 8, 3, 2))
    got = closed_loop_ssm.advance_tpwl(big, np.zeros((10, 128)), np.zeros(10), small, 0.01, 3, j, theta, np.zeros((1, 3, 8)), np.zeros((1, 128)))
    assert np.isfinite(got['X']).all() and got['X'].shape == (1, 2, 128)
    # a plant that is not discretised at dt_sim: the continuous handle
    h = C.c_void_p()
    Cm, yr = _lib.f64(inp['C']), _lib.f64(inp['y_ref'])
    rc = lib.sgusto_ssm_loop_create_tpwl(C.byref(h), gu.plan, planner.handle, plant.handle_for(None), _lib.dptr(Cm), _lib.dptr(yr), C.c_int(6),
                                         C.c_double(DT_SIM), C.c_int(NK), C.c_int64(32))
    assert rc == -1 and b'sgusto_ssm_loop_create_tpwl: the plant has not been pre-discretised at dt_sim' in lib.srh_last_error() and not h
    # n_u: the g6 plant has three inputs, the plan four
    g6 = tpwl_plant('g6')
    rc = lib.sgusto_ssm_loop_create_tpwl(C.byref(h), gu.plan, planner.handle, g6.handle_for(0.01), _lib.dptr(Cm), _lib.dptr(yr), C.c_int(6),
                                         C.c_double(DT_SIM), C.c_int(NK), C.c_int64(32))
    assert rc == -1 and b'the plant has n_u = 3, the planner\'s model n_u = 4' in lib.srh_last_error() and not h
    # C's rows against the planner model's n_o, and n_keep dt_sim > N dt
    rc = lib.sgusto_ssm_loop_create_tpwl(C.byref(h), gu.plan, planner.handle, plant.handle_for(DT_SIM), _lib.dptr(Cm), _lib.dptr(yr), C.c_int(5),
                                         C.c_double(DT_SIM), C.c_int(NK), C.c_int64(32))
    assert rc == -1 and b'C has n_o = 5 rows, the planner\'s model measures n_o = 6 outputs' in lib.srh_last_error() and not h
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.07 exceeds the horizon N \* dt = 0\.06'):
        SSMClosedLoopBatch.on_plant(gu, plant, DT_SIM, 7, C=inp['C'], y_ref=inp['y_ref'])
    # the loop itself: run before reset, and over the cap
    cl = SSMClosedLoopBatch.on_plant(gu, plant, DT_SIM, NK, t=inp['t'], z=inp['zt'], max_steps_per_run=6, C=inp['C'], y_ref=inp['y_ref'])
    with pytest.raises(RuntimeError, match='sgusto_ssm_loop_reset'):
        cl.run(1)
    cl.reset(inp['x0'])
    with pytest.raises(RuntimeError, match=r'periods \* n_keep = 8 exceeds max_steps_per_run = 6'):
        cl.run(4)
    r = cl.run(3)                                # the refused call left the loop as it was
    assert r.x.shape == (3, 7, 72) and r.u.shape == (3, 6, 4) and cl.stats()['steps'] == 3
