"""GPU: the measurement re-projection inside the batched SSM closed loops -- set_reproject(Y) of an SSMClosedLoopBatch on either plant
kind, the <true> instantiations of ssm_loop_advance_kernel and ssm_loop_advance_tpwl_kernel
(csrc/gusto_ssm_loop.hip) calling the one-wave projection unit csrc/poly_dev.h between the measurement and the estimate.

One launch, on shapes of tests/ssm_loop_cases.py (SSM plant) and tests/ssm_loop_tpwl_cases.py (TPWL plant): plant states, outputs, inputs
and raw measurements keep the bits of the launch without Y; where proj == 0 y_used has the bits of y and x_hat those of the launch
without Y; where proj == 1 y_used has the bits of Polyhedron.project_to_polyhedron(y); every x_hat row agrees with the long-double
estimate V phi(y_used - z_ref) of tests/ssm_reference.py within the project's rule max(100 e_oracle, 1e-13), e_oracle the float64
oracle's own error on the same y_used.
Whole loops, both plants: the same per row; last_inputs()['x0'] at a period start has the bits of the estimate; a Y that contains every
sample and an empty Y (proj == -1 everywhere) give the run without Y bit for bit; a NaN in one member's V gives that sample -2 and
leaves the other members alone; a member of a batch equals the member run alone.
Y is built from the CPU chains (one launch) or from the first measurement computed on the CPU (loops) so that samples fall on both
sides; that no raw sample lies within 1e-9 scale of a face is asserted on the device's record."""
import numpy as np
import pytest

import cl_reference as cr
import koopman_reproject_cases as rc
import ssm_cases as sc
import ssm_loop_cases as slc
import ssm_loop_tpwl_cases as stc
import ssm_reference as sr
import test_gusto_ssm_loop_gpu as tg
import test_gusto_ssm_loop_tpwl_gpu as tt
from oracle import ssm as ossm
from test_ssm_gpu import product_ssm

pytestmark = pytest.mark.gpu

PERIODS = 3
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def Ypoly(A, b):
    from sofacontrol_amd.utils import Polyhedron
    return Polyhedron(A, b, with_reproject=True)


def straddling(samples, wide=0.5, tight=True):
    """(A, b) of a box and one oblique facet in the samples' space: every coordinate bounded `wide` beyond the samples, except the upper
    bound of coordinate 0 (their median) and, where tight and beyond one dimension, the lower bound of the last one (their lower
    quartile); the facet sum(y) / sqrt(n) <= the 70 % quantile of the samples' (tight) or their largest."""
    flat = np.reshape(samples, (-1, np.shape(samples)[-1]))
    no = flat.shape[1]
    lo, hi = flat.min(axis=0) - wide, flat.max(axis=0) + wide
    hi[0] = np.median(flat[:, 0]) + 1e-5
    if no > 1 and tight:
        lo[-1] = np.quantile(flat[:, -1], 0.25) - 1e-5
    A = np.kron(np.eye(no), np.array([[1.0], [-1.0]]))
    b = np.ravel(np.stack([hi, -lo], axis=1))
    a = np.ones(no) / np.sqrt(no)
    return np.vstack([A, a[None]]), np.append(b, np.quantile(flat @ a, 0.7 if tight else 1.0) + 1e-5)


def ld_model(d):
    """The long-double model of an oracle model dict (oracle.ssm.make_model) or of coefficient arrays (ssm_cases.model)."""
    if 'rom_order' in d:
        return sc.reference_model(d)
    n = d['n']
    orders = [int(E.sum(axis=1).max()) for E in (d['Er'], d['Es'])]
    return sr.make_model(n, d['m'], n, orders[0], orders[1], d['R'], d['B'], d['W'], d['V'], d['z_ref'])


def check_rows(what, A, b, y, y_used, proj, x_hat, oracle_planner, ld_planner):
    """The per-row properties of a record (any leading shape) of raw samples, used samples, status words and estimates."""
    P = Ypoly(A, b)
    no, n = y.shape[-1], x_hat.shape[-1]
    y, y_used, proj, x_hat = y.reshape(-1, no), y_used.reshape(-1, no), proj.reshape(-1), x_hat.reshape(-1, n)
    share = rc.check_sides(A, b, y)                        # the condition on closeness to a face, on the device's raw record
    ref, f64 = [], []
    for k in range(len(y)):
        out = rc.side(A, b, y[k]) > 0.0
        assert proj[k] == (1 if out else 0), (what, k, proj[k])
        np.testing.assert_array_equal(bits(y_used[k]), bits(P.project_to_polyhedron(y[k]) if out else y[k]), err_msg='%s row %d' % (what, k))
        ref.append(sr.reduce(ld_planner, y_used[k])); f64.append(ossm.reduce(oracle_planner, y_used[k]))
    ref, f64 = np.stack(ref), np.stack(f64)
    e_oracle, e = sr.err(f64, ref), sr.err(x_hat, ref)
    tol = sc.tolerance(e_oracle)
    print('%s: %d rows, %.0f%% outside Y; x_hat against the long-double estimate of y_used - z_ref: %.3e (e_oracle %.3e, tolerance %.3e)'
          % (what, len(y), 100 * share, e, e_oracle, tol))
    assert e_oracle <= cr.E_ORACLE_MAX
    assert e <= tol, (what, e, tol)
    return share


# ------------------------------------------------------------------------------------------------------------- one launch
SSM_CASES = [c for c in slc.ADVANCE if c[0] in ((1, 1, 7, 7), (2, 3, 4, 1), (16, 4, 2, 1), (10, 8, 3, 2)) or (c[0] == (6, 4, 3, 2) and c[5] == 3)]


@pytest.mark.parametrize('case', SSM_CASES, ids=[slc.case_id(c) for c in SSM_CASES])
def test_one_launch_ssm_plant(case):
    from sofacontrol_amd.scp import closed_loop_ssm
    s, method, dt_sim, dt, N, nk = case
    planner = product_ssm(sc.oracle_model(sc.model(s)), discr='fe')
    pm = sc.oracle_model(slc.plant_model(s))
    plant = product_ssm(pm, discrete=True) if method == 'map' else product_ssm(pm, discr=method)
    i = slc.inputs(case)
    A, b = straddling(np.asarray(slc.reference(case)[0]['Y'], dtype=np.float64))
    run = lambda Y: closed_loop_ssm.advance(plant, planner, dt_sim, N, i['j'], i['theta'], i['uopt'], i['x'], W=i['W'], V=i['V'], Y=Y)
    base, got = run(None), run(Ypoly(A, b))
    for f in ('X', 'Z', 'U', 'Y'):
        np.testing.assert_array_equal(bits(got[f]), bits(base[f]), err_msg=f)
    assert got['proj'].dtype == np.int32 and got['proj'].shape == (slc.B, nk) and got['Y_used'].shape == got['Y'].shape
    share = check_rows(slc.case_id(case), A, b, got['Y'], got['Y_used'], got['proj'], got['Xhat'], sc.oracle_model(sc.model(s)),
                       sc.reference_model(sc.model(s)))
    assert 0.0 < share < 1.0
    inside = got['proj'] == 0
    np.testing.assert_array_equal(bits(got['Xhat'][inside]), bits(base['Xhat'][inside]))
    assert not np.array_equal(got['Xhat'][~inside], base['Xhat'][~inside])


TPWL_PAIRS = [p for p in stc.SMALL if p[0] in ('g6-knots-1', 'g6-frac-10', 'g6-single', 'r36-knots-max', 'm8-frac-10')]


@pytest.mark.parametrize('pair', TPWL_PAIRS, ids=[stc.case_id(p) for p in TPWL_PAIRS])
def test_one_launch_tpwl_plant(pair):
    from sofacontrol_amd.scp import closed_loop_ssm
    i, r = stc.inputs(pair), stc.reference(pair)
    A, b = straddling(np.asarray(r['ref']['Y'], dtype=np.float64))
    args = (tt.tpwl_plant(i['model']), i['C'], i['y_ref'], tt.observer(pair[1]), i['dt_sim'], i['N'], i['j'], i['theta'], i['uopt'], i['x'])
    base = closed_loop_ssm.advance_tpwl(*args, W=i['W'], V=i['V'])
    got = closed_loop_ssm.advance_tpwl_reprojected(*args, Ypoly(A, b), W=i['W'], V=i['V'])
    for f in ('X', 'Z', 'U', 'Y', 'idx'):
        np.testing.assert_array_equal(got[f], base[f], err_msg=f)
    d = stc.observer_model(pair[1])
    share = check_rows(stc.case_id(pair), A, b, got['Y'], got['Y_used'], got['proj'], got['Xhat'], sc.oracle_model(d), sc.reference_model(d))
    assert (0.0 < share < 1.0) or i['B'] * i['n_keep'] < 3
    inside = got['proj'] == 0
    np.testing.assert_array_equal(bits(got['Xhat'][inside]), bits(base['Xhat'][inside]))


# ------------------------------------------------------------------------------------------------------------- whole loops
KINDS = ('ssm', 'tpwl')
NOISE = 0.01


def loop_inputs(kind):
    """The inputs of the existing whole-loop tests of the plant kind (three members), with a measurement noise of NOISE so that the samples
    straddle a face, and the first measurements y0 on the CPU (float64)."""
    if ('inp', kind) in _cache:
        return _cache[('inp', kind)]
    if kind == 'ssm':
        inp = dict(tg.inputs('hw', 3))
        model, nk = tg.models('hw')[0], tg.LOOPS['hw'][6]
        y0 = np.stack([ossm.observe(model, x) for x in inp['x0']]) + model['z_ref']
    else:
        inp = dict(tt.inputs(3))
        model, nk = tt.models()[0], tt.NK
        y0 = inp['x0'] @ inp['C'].T + inp['y_ref']
    rng = np.random.default_rng(8300 + KINDS.index(kind))
    no = y0.shape[1]
    inp['v0'] = NOISE * rng.standard_normal((3, no))
    inp['V'] = NOISE * rng.standard_normal((tg.PERIODS, nk, 3, no))[:PERIODS]
    inp['W'] = np.ascontiguousarray(inp['W'][:PERIODS])
    inp['y0'] = y0 + inp['v0']
    inp['model'] = model
    _cache[('inp', kind)] = inp
    return inp


def polyhedra(kind):
    """name -> (A, b): 'Y' straddled by the samples, 'all' containing every sample, 'empty'."""
    y0 = loop_inputs(kind)['y0']
    no = y0.shape[1]
    cloud = np.concatenate([y0 + d for d in (-NOISE, 0.0, NOISE)])
    E = np.zeros((2, no)); E[0, 0], E[1, 0] = 1.0, -1.0
    return {'Y': straddling(cloud, tight=False), 'all': wide_box(cloud),'empty': (E, np.array([-1e3, -1e3]))}


def wide_box(cloud):
    no = cloud.shape[1]
    A = np.kron(np.eye(no), np.array([[1.0], [-1.0]]))
    return A, np.ravel(np.stack([cloud.max(axis=0) + 1e3, -(cloud.min(axis=0) - 1e3)], axis=1))


def make_loop(kind, Y, member=None):
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    inp = loop_inputs(kind)
    if member is not None:
        sl = slice(member, member + 1)
        inp = dict(inp, x0=inp['x0'][sl], v0=inp['v0'][sl], phase=inp['phase'][sl], W=np.ascontiguousarray(inp['W'][:, :, sl]),
                   V=np.ascontiguousarray(inp['V'][:, :, sl]))
    B = len(inp['x0'])
    if kind == 'ssm':
        gu = tg.make_gusto('hw', B, inp['x0'])
        dt_sim, nk = tg.LOOPS['hw'][5:7]
        cl = SSMClosedLoopBatch(gu, tg.models('hw')[2], dt_sim, nk, t=inp['t'], z=inp['zt'], phase=inp['phase'])
    else:
        gu = tt.make_gusto(B)
        cl = SSMClosedLoopBatch.on_plant(gu, tt.models()[2], tt.DT_SIM, tt.NK, t=inp['t'], z=inp['zt'], phase=inp['phase'], C=inp['C'],
                                         y_ref=inp['y_ref'])
    return cl.set_reproject(Y), gu, inp


def run_loop(kind, which, member=None, V=None):
    """The records of PERIODS periods run one by one, with last_inputs()['x0'] of every period: (result, [x0 of period p]); cached."""
    key = ('run', kind, which, member)
    if V is None and key in _cache:
        return _cache[key]
    Y = None if which is None else Ypoly(*polyhedra(kind)[which])
    cl, gu, inp = make_loop(kind, Y, member)
    Vn = inp['V'] if V is None else V
    cl.reset(inp['x0'], tg.T_START, v0=inp['v0'])
    rs, x0s = [], []
    for p in range(PERIODS):
        rs.append(cl.run(1, W=inp['W'][p:p + 1], V=Vn[p:p + 1]))
        x0s.append(cl.last_inputs()['x0'].copy())
    out = tg.cat(rs)
    if Y is not None:
        for a, c in zip(rs[:-1], rs[1:]):
            np.testing.assert_array_equal(bits(a.y_used[:, -1]), bits(c.y_used[:, 0])); np.testing.assert_array_equal(a.proj[:, -1], c.proj[:, 0])
        out.y_used = np.concatenate([rs[0].y_used] + [r.y_used[:, 1:] for r in rs[1:]], axis=1)
        out.proj = np.concatenate([rs[0].proj] + [r.proj[:, 1:] for r in rs[1:]], axis=1)
    if V is None:
        _cache[key] = (out, x0s)
    return out, x0s


def same(a, b, what, members=slice(None)):
    for f in tg.FIELDS:
        va, vb = getattr(a, f), getattr(b, f)
        if f in ('iters', 'status', 'J'):
            va, vb = va[:, members], vb[:, members]
        else:
            va, vb = va[members], vb[members]
        np.testing.assert_array_equal(va, vb, err_msg='%s: %s' % (what, f))


@pytest.mark.parametrize('kind', KINDS)
def test_loop_rows_and_period_starts(kind):
    r, x0s = run_loop(kind, 'Y')
    inp = loop_inputs(kind)
    A, b = polyhedra(kind)['Y']
    nk = r.u.shape[1] // PERIODS
    assert r.y_used.shape == r.y.shape and r.proj.shape == r.y.shape[:2] and r.proj.dtype == np.int32
    e = sr.err(r.y[:, 0], inp['y0'])
    print('%s: row 0 of y against the first measurement formed on the CPU: %.3e' % (kind, e))
    assert e <= cr.TOL_FLOOR
    check_rows('%s plant, %d periods' % (kind, PERIODS), A, b, r.y, r.y_used, r.proj, r.x_hat, inp['model'], ld_model(inp['model']))
    print(r.proj)
    assert min((r.proj == 0).sum(), (r.proj == 1).sum()) >= 3, 'the case must hold samples on both sides'
    for p in range(PERIODS):                               # the plans start from the estimate of the used sample
        np.testing.assert_array_equal(bits(x0s[p]), bits(r.x_hat[:, p * nk]), err_msg='period %d' % p)
    base, _ = run_loop(kind, None)
    assert base.y_used is None and base.proj is None
    assert not np.array_equal(base.u, r.u), 'the run with Y and the run without apply the same inputs'


@pytest.mark.parametrize('kind', KINDS)
def test_containing_and_empty_Y_are_neutral(kind):
    base, x0b = run_loop(kind, None)
    for which, word in (('all', 0), ('empty', -1)):
        r, x0s = run_loop(kind, which)
        assert (r.proj == word).all(), (which, r.proj)
        same(r, base, '%s Y' % which)
        np.testing.assert_array_equal(bits(r.y_used), bits(r.y))
        np.testing.assert_array_equal(bits(np.stack(x0s)), bits(np.stack(x0b)))


@pytest.mark.parametrize('kind', KINDS)
def test_nan_sample_is_reported_and_stays_in_its_member(kind):
    ref, _ = run_loop(kind, 'Y')
    V = loop_inputs(kind)['V'].copy()
    nk = V.shape[1]
    V[PERIODS - 1, nk - 1, 1, 0] = np.nan                  # the last sample of member 1
    r, _ = run_loop(kind, 'Y', V=V)
    assert r.proj[1, -1] == -2 and np.isnan(r.y_used[1, -1, 0]) and np.isnan(r.y[1, -1, 0])
    np.testing.assert_array_equal(r.proj[:, :-1], ref.proj[:, :-1])
    for m in (0, 2):
        same(r, ref, 'member %d beside a NaN sample' % m, members=slice(m, m + 1))
        np.testing.assert_array_equal(bits(r.y_used[m]), bits(ref.y_used[m])); np.testing.assert_array_equal(r.proj[m], ref.proj[m])


@pytest.mark.parametrize('kind', KINDS)
def test_member_of_a_batch_equals_the_member_alone(kind):
    batch, _ = run_loop(kind, 'Y')
    alone, _ = run_loop(kind, 'Y', member=1)
    for f in tg.FIELDS:
        va, vb = getattr(alone, f), getattr(batch, f)
        vb = vb[:, 1:2] if f in ('iters', 'status', 'J') else vb[1:2]
        np.testing.assert_array_equal(va, vb, err_msg=f)
    np.testing.assert_array_equal(bits(alone.y_used[0]), bits(batch.y_used[1])); np.testing.assert_array_equal(alone.proj[0], batch.proj[1])


def test_observe_false_with_Y_is_refused():
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    inp = loop_inputs('ssm')
    gu = tg.make_gusto('hw', 3, inp['x0'])
    cl = SSMClosedLoopBatch(gu, tg.models('hw')[2], 0.02, 2, t=inp['t'], z=inp['zt'], observe=False)
    with pytest.raises(RuntimeError, match='SSMClosedLoopBatch: Y together with observe=False is refused'):
        cl.set_reproject(Ypoly(*polyhedra('ssm')['Y']))
    from sofacontrol_amd import _lib                       # and by the library, for a caller of the C entry
    A, b = polyhedra('ssm')['Y']
    assert _lib.lib().sgusto_ssm_loop_set_reproject(cl._h, _lib.dptr(_lib.f64(A)), _lib.dptr(_lib.f64(b)), A.shape[0]) == -1
    assert b'observe = 0' in _lib.lib().srh_last_error()
