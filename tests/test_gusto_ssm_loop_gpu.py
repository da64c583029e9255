"""GPU: the batched SSM closed loop (csrc/gusto_ssm_loop.hip, scp/closed_loop_ssm.py), every arrow of a period.

Preparation (x0, first guess, shift, target window), solve (the loop's solve against a second GuSTO fed the loop's own inputs through
solve_batch), advance (ssm_loop_advance_kernel alone on the seeded cases of tests/ssm_loop_cases.py) and their composition.  Comparisons
between two runs of the same kernel on the same bits are exact; comparisons with the long-double reference (tests/ssm_loop_reference.py,
tests/cl_reference.py) use the project's rule tol = max(100 e_oracle, 1e-13) on max|a - b| / max(1, max|b|), e_oracle = the float64
statement's own error on the same case (asserted <= 1e-11), every figure printed before it is asserted.

Two loops, 4 periods.  `hw`: the hardware driver's shape (n_x = 6, n_u = 4, cubic / quadratic, be, N = 3, dt = dt_sim = 0.02, n_keep = 2,
three weighted outputs, U box, max_gusto_iters = 0: the dense one-wave QP), plant = planner, phases before t[0] and behind t[-1].  `frac`:
n_x = 4, n_u = 2, fe, N = 8, dt = 0.02, dt_sim = 0.012, n_keep = 5, U box and a state polyhedron (qp::solve), max_gusto_iters = 3, an input
target, a perturbed plant stepped in be, disturbances and measurement noise."""
import ctypes as C

import numpy as np
import pytest

import cl_reference as cr
import ssm_cases as sc
import ssm_loop_cases as slc
import ssm_reference as sr
from oracle import ssm as ossm
from test_ssm_gpu import product_ssm

pytestmark = pytest.mark.gpu

PERIODS = 4
T_START = 0.1
# name -> (shape, seed, planner method, N, dt, dt_sim, n_keep, max_gusto_iters)
LOOPS = {'hw': ((6, 4, 3, 2), 96, 'be', 3, 0.02, 0.02, 2, 0), 'frac': ((4, 2, 3, 2), 81, 'fe', 8, 0.02, 0.012, 5, 3)}
_cache = {}


def models(name):
    """(oracle model dict of the planner, planner SSMDynamics, plant SSMDynamics): hw's plant is the planner itself, frac's is the
    planner with its nonlinear R columns and its W moved 2 % towards the model of seed + 100, stepped in be."""
    if ('m', name) not in _cache:
        (n, m, ro, so), seed, method = LOOPS[name][:3]
        model = ossm.synthetic(n, m, ro, so, seed=seed)
        planner = product_ssm(model, discr=method)
        plant = planner
        if name == 'frac':
            other = ossm.synthetic(n, m, ro, so, seed=seed + 100)
            pm = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in model.items()}
            pm['R'][:, n:] += 0.02 * (other['R'][:, n:] - model['R'][:, n:])
            pm['W'] += 0.02 * (other['W'] - model['W'])
            plant = product_ssm(pm, discr='be')
        _cache[('m', name)] = (model, planner, plant)
    return _cache[('m', name)]


def inputs(name, B):
    """x0 (B, n), v0 (B, n), phase (B,), W, V (PERIODS, n_keep, B, n), the tables t, zt (T, n), ut (T, m): members 0..2 are the same for
    every B >= 3 and differ; member 0 asks for targets before t[0], member 2 behind t[-1] (the clamped ends of the table)."""
    (n, m, _, _), seed, _, N, dt, dt_sim, nk, _ = LOOPS[name]
    rng = np.random.default_rng(4000 + seed)
    big = 260
    x0 = 0.05 * rng.standard_normal((big, n)); v0 = 1e-3 * rng.standard_normal((big, n))
    phase = np.concatenate([[-0.5, 0.2, 1.2], rng.uniform(0.0, 0.8, big - 3)])
    W = 1e-3 * rng.standard_normal((PERIODS, nk, big, n)); V = 1e-3 * rng.standard_normal((PERIODS, nk, big, n))
    t = np.linspace(0.0, 1.0, 31)
    zt = np.zeros((31, n)); zt[:, 0] = 0.02 * np.sin(2 * np.pi * t); zt[:, 1] = -0.01 * np.cos(2 * np.pi * t); zt[:, 2] = 0.015 * t
    zt = zt + ossm.observe(models(name)[0], np.zeros(n))
    ut = 0.1 * np.sin(2 * np.pi * t)[:, None] * np.linspace(1.0, 0.5, m)[None, :]
    return dict(x0=x0[:B], v0=v0[:B], phase=phase[:B], W=np.ascontiguousarray(W[:, :, :B]), V=np.ascontiguousarray(V[:, :, :B]), t=t, zt=zt, ut=ut)


def make_gusto(name, B, x0, keep=False, dU=None):
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import HyperRectangle, Polyhedron
    (n, m, _, _), _, _, N, dt, _, _, cap = LOOPS[name]
    model, planner, _ = models(name)
    u_init = np.zeros((B, N, m))
    x_init, _ = planner.rollout(x0, u_init, dt)
    z = np.tile(ossm.observe(model, np.zeros(n)), (B, N + 1, 1))
    if name == 'hw':
        Qz = np.zeros((n, n)); Qz[0, 0] = Qz[1, 1] = Qz[2, 2] = 100.0
        kw = dict(R=1e-3 * np.eye(m), U=HyperRectangle([3.0] * m, [-1.0] * m), convg_thresh=1e-5)
    else:
        Qz = np.diag([10., 10., 1., 1.])
        kw = dict(R=1e-2 * np.eye(m), U=HyperRectangle([2.0] * m, [-2.0] * m), convg_thresh=1e-4,
                  X=Polyhedron(np.array([[1.0, 0, 0, 0], [-1.0, 0, 0, 0]]), np.array([0.5, 0.5])))
    R = kw.pop('R')
    g = GuSTO(SSMGuSTO(planner), N, dt, Qz, R, x0, u_init, x_init, z=z, verbose=0, max_gusto_iters=cap, batch=B, first_solve_cap=1, max_trace=0,
              keep_solver_state=keep, dU=dU, **kw)
    assert g._ssm
    return g


def make_loop(name, B, member=None, keep=False, observe=True, max_steps_per_run=None):
    """(loop, gusto, inputs) of LOOPS[name] with B members; member = b: the B = 1 loop of member b of the three-member batch."""
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    dt_sim, nk = LOOPS[name][5:7]
    inp = inputs(name, max(B, 3) if member is not None else B)
    if member is not None:
        sl = slice(member, member + 1)
        inp = dict(inp, x0=inp['x0'][sl], v0=inp['v0'][sl], phase=inp['phase'][sl], W=np.ascontiguousarray(inp['W'][:, :, sl]),
                   V=np.ascontiguousarray(inp['V'][:, :, sl]))
    gu = make_gusto(name, B, inp['x0'], keep=keep)
    cl = SSMClosedLoopBatch(gu, models(name)[2], dt_sim, nk, t=inp['t'], z=inp['zt'], u=inp['ut'] if name == 'frac' else None, phase=inp['phase'],
                            observe=observe, max_steps_per_run=max_steps_per_run)
    return cl, gu, inp


def plan_costs(g):
    """Jopt of a plan's last solve (sgusto_ssm_plan_costs_dev into a device buffer on the null stream)."""
    from sofacontrol_amd import _lib
    buf = _lib.DeviceBuffer(8 * g.batch)
    _lib.check(_lib.lib().sgusto_ssm_plan_costs_dev(g.plan, buf.ptr, None), 'sgusto_ssm_plan_costs_dev')
    _lib.sync()
    return buf.to_array((g.batch,))


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


def check_window(what, got, table_t, table_y, t0s, dt, rows):
    for b, t0 in enumerate(t0s):
        ref, f64 = cr.window(table_t, table_y, t0, dt, rows, cr.LD), cr.window(table_t, table_y, t0, dt, rows, np.float64)
        e_oracle = cr.err(f64, ref)
        e = cr.err(got[b], ref)
        print('%s member %d: e_oracle %.3e, device %.3e, tolerance %.3e' % (what, b, e_oracle, e, cr.tolerance(e_oracle)))
        assert e_oracle <= cr.E_ORACLE_MAX
        assert e <= cr.tolerance(e_oracle)


# ---------------------------------------------------------------------------------------------------------------- 1. preparation
@pytest.mark.parametrize('observe', [True, False], ids=['estimate', 'state'])
@pytest.mark.parametrize('name', list(LOOPS))
def test_preparation(name, observe):
    from sofacontrol_amd.scp.closed_loop import schedule
    (n, m, _, _), _, _, N, dt, dt_sim, nk, _ = LOOPS[name]
    cl, gu, inp = make_loop(name, 3, observe=observe)
    _, planner, _ = models(name)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    r0 = cl.step()
    li = cl.last_inputs()
    start = lambda r: r.x_hat if observe else r.x
    np.testing.assert_array_equal(r0.x[:, 0], inp['x0'])
    np.testing.assert_array_equal(li['x0'], start(r0)[:, 0])
    assert not li['u_init'].any()
    x_roll, _ = planner.rollout(li['x0'], np.zeros((3, N, m)), dt)
    np.testing.assert_array_equal(li['x_init'], x_roll)
    check_window('z, period 0', li['z'], inp['t'], inp['zt'], T_START + inp['phase'], dt, N + 1)
    assert (T_START + inp['phase'][0] < inp['t'][0]) and (T_START + inp['phase'][2] + dt * N > inp['t'][-1])      # both clamped ends
    xo, uo = cl.last_plan()
    r1 = cl.step()
    li = cl.last_inputs()
    s1 = schedule(N, dt, dt_sim, nk, T_START, 1)
    assert 0 < s1.idx0 <= N
    for b in range(3):
        u_ws, x_ws = cr.shift(xo[b], uo[b], s1.idx0)
        np.testing.assert_array_equal(li['u_init'][b], u_ws)
        np.testing.assert_array_equal(li['x_init'][b], x_ws)
    np.testing.assert_array_equal(li['x0'], start(r0)[:, -1])
    for f in ('x', 'z', 'y', 'x_hat'):
        np.testing.assert_array_equal(getattr(r1, f)[:, 0], getattr(r0, f)[:, -1], err_msg=f)
    check_window('z, period 1', li['z'], inp['t'], inp['zt'], s1.t_k + inp['phase'], dt, N + 1)
    if name == 'frac':
        check_window('u_des, period 1', li['u'], inp['t'], inp['ut'], s1.t_k + inp['phase'], dt, N)
    else:
        assert li['u'] is None


# ---------------------------------------------------------------------------------------------------------------- 2. solve
@pytest.mark.parametrize('name', list(LOOPS))
def test_every_solve_equals_a_second_plan_fed_the_loops_inputs(name):
    cl, gu, inp = make_loop(name, 3)
    g2 = make_gusto(name, 3, inp['x0'])
    g2.max_gusto_iters = gu.max_gusto_iters
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    for k in range(PERIODS):
        r = cl.step()
        li = cl.last_inputs()
        xo, uo = cl.last_plan()
        x2, u2, _ = g2.solve_batch(li['x0'], li['u_init'], li['x_init'], z=li['z'], u=li['u'])
        np.testing.assert_array_equal(xo, x2); np.testing.assert_array_equal(uo, u2)
        np.testing.assert_array_equal(r.iters[0], g2.iters); np.testing.assert_array_equal(r.status[0], g2.status)
        np.testing.assert_array_equal(r.J[0], plan_costs(g2))
        assert np.isfinite(r.J).all() and (r.iters >= 1).all()


# ---------------------------------------------------------------------------------------------------------------- 3. advance
@pytest.mark.parametrize('case', slc.ADVANCE, ids=[slc.case_id(c) for c in slc.ADVANCE])
def test_advance_kernel_against_the_long_double_chain(case):
    """Measured on the MI355X: the figures are in DESIGN.md section 28."""
    from sofacontrol_amd.scp import closed_loop_ssm
    s, method, dt_sim, dt, N, nk = case
    planner = product_ssm(sc.oracle_model(sc.model(s)), discr='fe')
    pm = sc.oracle_model(slc.plant_model(s))
    plant = product_ssm(pm, discrete=True) if method == 'map' else product_ssm(pm, discr=method)
    i = slc.inputs(case)
    got = closed_loop_ssm.advance(plant, planner, dt_sim, N, i['j'], i['theta'], i['uopt'], i['x'], W=i['W'], V=i['V'])
    ref, e_oracle = slc.reference(case)
    eo = max(e_oracle.values())
    tol = sc.tolerance(eo)
    print('%s: e_oracle %.3e, tolerance %.3e' % (slc.case_id(case), eo, tol))
    worst = {}
    for f in slc.FIELDS:
        errs = [sr.err(got[f][:, q], ref[f][:, q]) for q in range(nk)]
        worst[f] = max(errs)
        print('  %s: worst error over the sub-steps %.3e (sub-step %d), tolerance / error %s' %
              (f, max(errs), int(np.argmax(errs)), '%.1f' % (tol / max(errs)) if max(errs) > 0 else 'inf'))
    for f, e in worst.items():
        assert e <= tol, (f, e, tol)
    np.testing.assert_array_equal(got['Y'], (got['Z'] + slc.plant_model(s)['z_ref']) + i['V'].transpose(1, 0, 2))


# ---------------------------------------------------------------------------------------------------------------- 4. composition
@pytest.fixture(scope='module')
def frac_run4():
    """run(4) of the three-member 'frac' loop with W and V: (loop, gusto, inputs, result)."""
    cl, gu, inp = make_loop('frac', 3)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    return cl, gu, inp, cl.run(PERIODS, W=inp['W'], V=inp['V'])


def test_run_equals_steps_and_split_runs(frac_run4):
    cl, gu, inp, r4 = frac_run4
    assert r4.x.shape == (3, 21, 4) and r4.z.shape == (3, 21, 4) and r4.y.shape == (3, 21, 4) and r4.x_hat.shape == (3, 21, 4)
    assert r4.u.shape == (3, 20, 2) and r4.J.shape == (4, 3)
    assert all(np.isfinite(getattr(r4, f)).all() for f in FIELDS)
    np.testing.assert_allclose(r4.t, T_START + 0.012 * np.arange(21), rtol=0, atol=1e-12)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    same(cat([cl.run(2, W=inp['W'][:2], V=inp['V'][:2]), cl.run(2, W=inp['W'][2:], V=inp['V'][2:])]), r4)
    assert cl.stats()['steps'] == 4
    # step() carries neither disturbance nor noise: compare without them
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    r4n = cl.run(PERIODS)
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    same(cat([cl.step() for _ in range(PERIODS)]), r4n)
    assert not np.array_equal(r4n.x, r4.x) and not np.array_equal(r4n.y, r4.y)      # disturbance and noise are felt
    assert len({r4.x[b].tobytes() for b in range(3)}) == 3                           # the members differ
    assert (r4.iters >= 1).all()


@pytest.mark.parametrize('keep', [False, True], ids=['cold', 'keep_solver_state'])
def test_batch_members_equal_their_single_loops(frac_run4, keep):
    _, _, inp, r4 = frac_run4
    if keep:
        cl3, _, _ = make_loop('frac', 3, keep=True)
        cl3.reset(inp['x0'], T_START, v0=inp['v0'])
        r4 = cl3.run(PERIODS, W=inp['W'], V=inp['V'])
    for b in range(3):
        cl1, _, inp1 = make_loop('frac', 1, member=b, keep=keep)
        np.testing.assert_array_equal(inp1['x0'][0], inp['x0'][b])
        cl1.reset(inp1['x0'], T_START, v0=inp1['v0'])
        r1 = cl1.run(PERIODS, W=inp1['W'], V=inp1['V'])
        for f in ('x', 'z', 'u', 'y', 'x_hat'):
            np.testing.assert_array_equal(getattr(r1, f)[0], getattr(r4, f)[b], err_msg='%s of member %d' % (f, b))
        for f in ('iters', 'status', 'J'):
            np.testing.assert_array_equal(getattr(r1, f)[:, 0], getattr(r4, f)[:, b], err_msg='%s of member %d' % (f, b))


def test_first_members_of_260_equal_the_batch_of_three(frac_run4):
    _, _, inp, r4 = frac_run4
    cl, gu, big = make_loop('frac', 260)
    np.testing.assert_array_equal(big['x0'][:3], inp['x0'])
    cl.reset(big['x0'], T_START, v0=big['v0'])
    r = cl.run(PERIODS, W=big['W'], V=big['V'])
    for f in ('x', 'z', 'u', 'y', 'x_hat'):
        np.testing.assert_array_equal(getattr(r, f)[:3], getattr(r4, f), err_msg=f)
    for f in ('iters', 'status', 'J'):
        np.testing.assert_array_equal(getattr(r, f)[:, :3], getattr(r4, f), err_msg=f)
    assert all(np.isfinite(getattr(r, f)).all() for f in FIELDS)


# ---------------------------------------------------------------------------------------------------------------- 5. waits and records
def test_one_wait_per_run_records_and_the_first_estimate(frac_run4):
    cl, gu, inp, r4 = frac_run4
    cl.reset(inp['x0'], T_START, v0=inp['v0'])
    r = cl.run(PERIODS, W=inp['W'], V=inp['V'], record_x=False)
    assert cl.stats() == {'steps': 4, 'waits_last_run': 1}
    assert r.x is None
    same(r, r4, fields=[f for f in FIELDS if f != 'x'])
    # row 0: the reference's first observer.update -- y0 = (C_plant(x0) + z_ref_plant) + v0, x_hat0 = W_map(y0 - z_ref) of the controller's model
    _, planner, plant = models('frac')
    np.testing.assert_array_equal(r4.x[:, 0], inp['x0'])
    np.testing.assert_array_equal(r4.y[:, 0], (r4.z[:, 0] + plant.z_ref) + inp['v0'])
    e = sr.err(r4.z[:, 0], plant.x_to_zy(inp['x0'].T).T)
    print('row 0 of z against C_map of the plant: %.3e' % e)
    assert e <= cr.TOL_FLOOR
    for rows in (0, slice(None)):
        y = r4.y[:, rows].reshape(-1, 4)
        e = sr.err(r4.x_hat[:, rows].reshape(-1, 4), planner.observed_to_reduced((y - planner.z_ref).T).T)
        print('x_hat against W_map of y (rows %s): %.3e' % (rows, e))
        assert e <= cr.TOL_FLOOR


# ---------------------------------------------------------------------------------------------------------------- 6. two units, one host shell
def test_interleaved_tpwl_and_ssm_loops_equal_each_loop_alone():
    """Both units run on the host shell of csrc/gusto_loop_host.h: a TPWL loop and an SSM loop driven in turn, with disturbance and noise,
    give the records, bit for bit, of the same two runs of each loop alone -- nothing of a handle lives in a static or a shared block."""
    import test_gusto_loop_gpu as tl

    def tpwl():
        cl, _, inp = tl.make_loop('frac', 3)
        cl.reset(inp['x0'], T_START)
        return cl, lambda k: cl.run(1, W=inp['W'][k:k + 1])

    def ssm():
        cl, _, inp = make_loop('frac', 3)
        cl.reset(inp['x0'], T_START, v0=inp['v0'])
        return cl, lambda k: cl.run(1, W=inp['W'][k:k + 1], V=inp['V'][k:k + 1])

    (ct, rt), (cs, rs) = tpwl(), ssm()
    alone_t, alone_s = [rt(0), rt(1)], [rs(0), rs(1)]
    (ct, rt), (cs, rs) = tpwl(), ssm()
    mixed = [rt(0), rs(0), rt(1), rs(1)]
    assert ct.stats() == {'steps': 2, 'waits_last_run': 1} and cs.stats() == {'steps': 2, 'waits_last_run': 1}
    for k in range(2):
        tl.same(mixed[2 * k], alone_t[k])
        same(mixed[2 * k + 1], alone_s[k])
        np.testing.assert_array_equal(mixed[2 * k].t, alone_t[k].t); np.testing.assert_array_equal(mixed[2 * k + 1].t, alone_s[k].t)
    assert not np.array_equal(alone_t[0].x, alone_t[1].x) and not np.array_equal(alone_s[0].x, alone_s[1].x)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    from sofacontrol_amd.utils import HyperRectangle
    inp = inputs('hw', 3)
    _, planner, _ = models('hw')
    gu = make_gusto('hw', 3, inp['x0'])
    cl = SSMClosedLoopBatch(gu, planner, 0.02, 2, t=inp['t'], z=inp['zt'], max_steps_per_run=6)
    with pytest.raises(RuntimeError, match='sgusto_ssm_loop_reset'):
        cl.run(1)
    with pytest.raises(RuntimeError, match='no period has run'):
        cl.last_inputs()
    cl.reset(inp['x0'])
    with pytest.raises(RuntimeError, match=r'periods \* n_keep = 8 exceeds max_steps_per_run = 6'):
        cl.run(4)
    r = cl.run(3)                                # the refused call left the loop as it was
    assert r.u.shape == (3, 6, 4) and cl.stats()['steps'] == 3
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.08 exceeds the horizon N \* dt = 0\.06'):
        SSMClosedLoopBatch(gu, planner, 0.02, 4)
    with pytest.raises(RuntimeError, match=r'the plant has n_x = 4, n_u = 2, n_o = 4, the planner\'s model n_x = 6, n_u = 4, n_o = 6'):
        SSMClosedLoopBatch(gu, models('frac')[1], 0.02, 2)
    with pytest.raises(RuntimeError, match='the plant has no discrete map'):
        SSMClosedLoopBatch(gu, types_plant_without_map(), 0.02, 2)
    # a plan with rate rows: refused by the class, and by the library itself
    rated = make_gusto('hw', 3, inp['x0'], dU=HyperRectangle([0.5] * 4, [-0.5] * 4))
    assert rated._ssm and rated._rate_rows == 8
    with pytest.raises(RuntimeError, match=r'8 input-rate rows \(dU\)'):
        SSMClosedLoopBatch(rated, planner, 0.02, 2)
    h = C.c_void_p()
    lib = _lib.lib()
    assert lib.sgusto_ssm_loop_create(C.byref(h), rated.plan, planner.handle, planner.handle, C.c_int(2), C.c_double(0.02), C.c_int(2), C.c_int(1),
                                      C.c_int64(32)) == -1
    assert b'8 input-rate rows (dU)' in lib.srh_last_error() and not h


def types_plant_without_map():
    """The hw model without rd_coeff / Bd, flagged discrete: the mode that asks for the discrete map."""
    from sofacontrol_amd import _lib
    model, planner, _ = models('hw')
    p = product_ssm(model, discrete=True)
    lib = _lib.lib()
    _lib.check(lib.sssm_destroy(p._h), 'sssm_destroy')
    p._h = C.c_void_p()
    f = lambda a: _lib.dptr(_lib.f64(a))
    _lib.check(lib.sssm_create(C.byref(p._h), C.c_int(6), C.c_int(4), C.c_int(6), C.c_int(3), C.c_int(2), f(model['R']), f(model['B']), None, None,
                               f(model['W']), f(model['V']), f(model['z_ref'])), 'sssm_create')
    return p
