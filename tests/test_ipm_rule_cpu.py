"""CPU: the interior point's rule on an inequality row as the seven QP kernels run it (csrc/ipm_rule.h, evaluated on the host by
sqp_ipm_rule_replay) against a numpy transcription of oracle/condensed_ipm.py's own lines (the line numbers below are that file's), and
the stopping ladder against a direct Python statement of it.

Both sides do the same IEEE operations in the same order -- the host build has no fused multiply-add to contract into -- so everything is
compared with ==.  Two expressions are grouped differently in the oracle, and there the kernels' grouping is the statement:
  * the predictor's gradient shift: the oracle writes lambda + (lambda rg - lambda t) / e (l. 284), the kernels D (rg + dreg lambda) with
    D = lambda / e, e = t + dreg lambda -- equal in exact arithmetic (rg - t + e = rg + dreg lambda);
  * the centring parameter: the oracle writes (mu_aff / mu) ** 3 (l. 303: C's pow), the kernels r * r * r with r = mu_aff / mu.  Two
    roundings of 2^-53 against pow's one ulp: the two agree to 2^-51 relative, asserted at 2^-50.
(-rg - a of l. 298 and the kernels' -(rg + a) are the same number: rounding is symmetric.)"""
import collections

import numpy as np
import pytest

from oracle import condensed_ipm as oc

GO_ON = -1
DREG = 1e-8 / 37.5


def replay(phase, rows, par):
    from sofacontrol_amd import _lib
    return _lib.ipm_rule_replay(phase, rows, par)


def rows8(**cols):
    """(n x 8) rows of the replay from named columns: g, t, lam, rg, rc, dt, dl, ad."""
    names = ('g', 't', 'lam', 'rg', 'rc', 'dt', 'dl', 'ad')
    n = len(next(iter(cols.values())))
    out = np.zeros((n, 8))
    for k, v in cols.items():
        out[:, names.index(k)] = v
    return out


def interior_rows(seed, n=257):
    """Rows of an interior-point iterate: slacks and multipliers over twelve decades (active rows: t -> 0, inactive ones: lambda -> 0),
    residuals and directions of both signs, plus hand-written edge rows."""
    rng = np.random.default_rng(seed)
    t = 10.0 ** rng.uniform(-9.0, 3.0, n)
    lam = 10.0 ** rng.uniform(-9.0, 3.0, n)
    g = -t + rng.standard_normal(n) * 10.0 ** rng.uniform(-12.0, 0.0, n)
    ad = rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 2.0, n)
    dt0 = rng.standard_normal(n) * t
    dl0 = rng.standard_normal(n) * lam
    edge = np.array([   # t, lam, g, ad, dt, dl
        [1.0, 1.0, -1.0, 0.0, 0.0, 0.0],            # at rest: no direction, neither bound binds
        [1e-2, 1e-2, -1e-2, 0.0, 0.0, 0.0],         # on the warm floor
        [1e-13, 1e3, 0.0, 1.0, -1e-13, 1.0],        # active row, slack about to vanish
        [1e3, 1e-13, -1e3, -1.0, 1.0, -1e-13],      # inactive row, multiplier about to vanish
        [2.0, 3.0, 5.0, -7.0, -4.0, -9.0],          # violated row, both bounds bind
    ])
    t, lam, g, ad, dt0, dl0 = (np.concatenate([a, edge[:, i]]) for i, a in enumerate((t, lam, g, ad, dt0, dl0)))
    return dict(t=t, lam=lam, g=g, ad=ad, dt=dt0, dl=dl0)


SEEDS = (0, 1, 2)


@pytest.fixture(scope='module')
def seen():
    return collections.Counter()


@pytest.mark.parametrize('seed', SEEDS)
def test_predictor_row(seed):
    r = interior_rows(seed)
    t, lam, g = r['t'], r['lam'], r['g']
    out, _ = replay('pred', rows8(g=g, t=t, lam=lam), [DREG])
    rg = g + t                                      # l. 277
    e = t + DREG * lam                              # l. 280
    D = lam / e                                     # l. 282
    assert (out[:, 0] == rg).all() and (out[:, 1] == D).all()
    assert (out[:, 2] == D * (rg + DREG * lam)).all()          # the kernels' grouping (module docstring)
    # l. 284, for the record: the oracle's grouping cancels lambda against lambda t / e, so the two agree to a few roundings of lambda and rho
    oracle_rho = lam + (lam * rg - lam * t) / e
    assert (np.abs(out[:, 2] - oracle_rho) <= 16 * np.finfo(float).eps * (lam + np.abs(oracle_rho) + np.abs(lam * rg / e))).all()
    assert (out[:, 3] == np.cumsum(lam * t)).all()             # l. 279: mu = (sum lambda t) / ng, summed row by row
    assert (out[:, 4] == np.maximum.accumulate(np.abs(rg))).all()     # l. 287


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('pred', (True, False))
def test_direction_and_step_bounds(seed, pred, seen):
    r = interior_rows(seed)
    t, lam, g, ad = r['t'], r['lam'], r['g'], r['ad']
    rg = g + t
    rc = lam * t + r['dt'] * r['dl'] - 0.3 * 0.7
    out, _ = replay('direction', rows8(t=t, lam=lam, rg=rg, rc=rc, ad=ad), [DREG, float(pred)])
    e = t + DREG * lam
    dl = (-lam * t + lam * (rg + ad)) / e if pred else (-rc + lam * (rg + ad)) / e     # l. 296 / l. 311
    dt = -rg - ad + DREG * dl                                                           # l. 298 / l. 313
    assert (out[:, 0] == dl).all() and (out[:, 1] == dt).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        bt = np.where(dt < 0, -t / dt, 1e300)                                           # l. 271-273: maxstep, row by row
        bl = np.where(dl < 0, -lam / dl, 1e300)
    assert (out[:, 2] == bt).all() and (out[:, 3] == bl).all()
    assert (out[:, 4] == np.minimum.accumulate(np.minimum(bt, bl))).all()
    seen['dt_binds'] += int(((dt < 0) & (bt < bl)).sum())
    seen['dl_binds'] += int(((dl < 0) & (bl < bt)).sum())
    seen['neither_binds'] += int(((dt >= 0) & (dl >= 0)).sum())


@pytest.mark.parametrize('seed', SEEDS)
def test_corrector_row(seed):
    r = interior_rows(seed)
    t, lam, dt, dl = r['t'], r['lam'], r['dt'], r['dl']
    rg = r['g'] + t
    sigma, mu = 0.3, 0.7
    out, _ = replay('corr', rows8(t=t, lam=lam, rg=rg, dt=dt, dl=dl), [DREG, sigma, mu])
    e = t + DREG * lam
    rc = lam * t + dt * dl - sigma * mu             # l. 304
    assert (out[:, 0] == rc).all()
    assert (out[:, 1] == lam + (lam * rg - rc) / e).all()      # l. 306


AMAX = (0.25, 0.999, 1.0, 1.005, 3.0, 1e300)       # 0.99 amax < 1 <= amax at 1.005; amax > 1; no bound at all


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('amax', AMAX)
def test_affine_term_sigma_and_step_lengths(seed, amax, seen):
    r = interior_rows(seed)
    t, lam, dt, dl = r['t'], r['lam'], r['dt'], r['dl']
    ng = len(t)
    for mu in (float(lam @ t) / ng, 0.0):
        out, scal = replay('affine', rows8(t=t, lam=lam, dt=dt, dl=dl), [amax, mu, ng])
        a_aff = min(1.0, amax)                      # l. 301
        a = min(1.0, 0.99 * amax)                   # l. 316
        assert scal[0] == a_aff and scal[1] == a
        term = (lam + a_aff * dl) * (t + a_aff * dt)            # l. 302, row by row
        assert (out[:, 0] == term).all() and (out[:, 1] == np.cumsum(term)).all()
        mu_aff = np.cumsum(term)[-1] / ng
        assert scal[2] == mu_aff
        ratio = mu_aff / mu if mu > 0 else 0.0
        assert scal[3] == (ratio * ratio * ratio if mu > 0 else 0.0)               # the kernels' grouping (module docstring)
        assert abs(scal[3] - (ratio ** 3 if mu > 0 else 0.0)) <= 2.0 ** -50 * abs(scal[3])      # l. 303
        seen['mu_zero'] += mu == 0.0
        seen['amax_above_1'] += amax > 1.0
        seen['step_cut_below_1'] += 0.99 * amax < 1.0
        seen['affine_full_step_cut'] += amax >= 1.0 and 0.99 * amax < 1.0
        out, _ = replay('advance', rows8(t=t, lam=lam, dt=dt, dl=dl), [a])
        assert (out[:, 0] == t + a * dt).all() and (out[:, 1] == lam + a * dl).all()       # l. 319-322


SHIFTS = ((-3.0, 2.5), (-3.0, -0.5), (0.25, 2.5), (0.0, 0.0), (-1e-300, 1e-300))     # (zmin, zmax)


@pytest.mark.parametrize('zmin,zmax', SHIFTS)
def test_cold_start(zmin, zmax, seen):
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.uniform(zmin, zmax, 64), [zmin, zmax]])
    out, scal = replay('init', rows8(g=g), [1.0])
    assert (out[:, 0] == 1.0).all() and (out[:, 1] == g).all() and (out[:, 2] == 0.0).all()       # l. 255-257: unit weights, shifts = row values
    out, _ = replay('init', rows8(g=g), [0.0])
    assert (out[:, 0] == 0.0).all() and (out[:, 1] == g).all()
    out, scal = replay('cold', rows8(g=g), [g.min(), g.max()])
    sh_t = (1.0 + g.max()) if g.max() >= 0 else 0.0            # l. 262
    sh_l = (1.0 - g.min()) if g.min() <= 0 else 0.0            # l. 263
    assert scal[0] == sh_t and scal[1] == sh_l
    assert (out[:, 0] == -g + sh_t).all() and (out[:, 1] == g + sh_l).all()        # l. 264-265
    seen['zmax_ge_0'] += g.max() >= 0
    seen['zmax_lt_0'] += g.max() < 0
    seen['zmin_le_0'] += g.min() <= 0
    seen['zmin_gt_0'] += g.min() > 0


@pytest.mark.parametrize('poison', (False, True))
def test_warm_start(poison, seen):
    rng = np.random.default_rng(6)
    g = np.concatenate([-10.0 ** rng.uniform(-6.0, 2.0, 64), 10.0 ** rng.uniform(-6.0, 2.0, 8), [-oc.WARM_FLOOR, 0.0]])
    lam_prev = np.concatenate([10.0 ** rng.uniform(-9.0, 3.0, 72), [oc.WARM_FLOOR, 0.0]])
    out, scal = replay('warm', rows8(g=g, lam=lam_prev), [float(poison)])
    assert scal[7] == oc.WARM_FLOOR
    assert (out[:, 0] == np.maximum(-g, oc.WARM_FLOOR)).all()                       # l. 250
    if poison:
        assert np.isposinf(out[:, 1]).all()
    else:
        assert (out[:, 1] == np.maximum(lam_prev, oc.WARM_FLOOR)).all()             # l. 251
    seen['poison'] += poison
    seen['t_floor_active'] += int((-g < oc.WARM_FLOOR).sum())
    seen['t_floor_inactive'] += int((-g > oc.WARM_FLOOR).sum())
    seen['lam_floor_active'] += int((lam_prev < oc.WARM_FLOOR).sum())
    seen['lam_floor_inactive'] += int((lam_prev > oc.WARM_FLOOR).sum())


@pytest.mark.parametrize('gmax,ubmax,omega,delta', ((1.0, 1.0, 1.0, 1e4), (37.5, 800.0, 5.0, -3.0), (2.0, 1.0, 1e6, 0.5)))
def test_scales(gmax, ubmax, omega, delta):
    reg = 1e-8
    _, scal = replay('scales', np.zeros((0, 8)), [gmax, ubmax, omega, delta, reg])
    scale_d = max(1.0, omega, gmax)                 # l. 266 (the kernels' maxima start from 1)
    scale_p = max(1.0, abs(delta), ubmax)           # l. 267
    assert scal[0] == scale_d and scal[1] == scale_p and scal[2] == reg / scale_d      # l. 268


def ladder(ok, mu, rd, rp, sd, sp, tol, it, max_iter, near_opt):
    """The predictor's stopping ladder, stated directly: (verdict, near_opt afterwards)."""
    if not ok:
        return (0 if near_opt else 2), near_opt
    if mu != mu:
        return (0 if near_opt else 5), near_opt
    if rd != rd:
        return (0 if near_opt else 6), near_opt
    ltol = max(tol, 1e-9)
    if rd <= ltol * sd and rp <= ltol * sp and mu <= tol:          # l. 290
        return 0, near_opt
    near_opt = rd <= 1e-8 * sd and rp <= 1e-8 * sp and mu <= 1e-8
    if it >= max_iter:
        return 1, near_opt
    return GO_ON, near_opt


def verdict_scripts():
    nan = float('nan')
    far, near = [1.0, 1e-2, 1.0, 1.0], [1.0, 1e-10, 1e-9, 1e-9]       # ok, mu, rd, rp (scales 10 and 100, tol 1e-12)
    done = [1.0, 1e-13, 1e-9, 1e-8]                                   # on the 1e-9 floor of the linear residuals
    for name, bad in (('factor', [0.0, 1e-2, 1.0, 1.0]), ('nan_mu', [1.0, nan, 1.0, 1.0]), ('nan_rd', [1.0, 1e-2, nan, 1.0])):
        yield name + '_far', [far + [0], bad + [1]]
        yield name + '_near_opt', [far + [0], near + [1], bad + [2]]
        yield name + '_near_opt_lost', [near + [0], far + [1], bad + [2]]
    yield 'converges', [far + [0], near + [1], done + [2]]
    yield 'iteration_cap', [far + [i] for i in range(8)]
    yield 'rp_alone_misses', [[1.0, 1e-13, 1e-9, 1e-6, 0]]
    yield 'mu_alone_misses', [[1.0, 1e-11, 1e-9, 1e-8, 0]]
    rng = np.random.default_rng(7)
    for seed in range(4):
        T = 40
        s = np.stack([(rng.random(T) < 0.9).astype(float), 10.0 ** rng.uniform(-14.0, 0.0, T), 10.0 ** rng.uniform(-10.0, 1.0, T),
                      10.0 ** rng.uniform(-9.0, 2.0, T), np.arange(T)], axis=1)
        s[rng.random(T) < 0.05, 1] = nan
        s[rng.random(T) < 0.05, 2] = nan
        yield 'random_%d' % seed, s.tolist()


VERDICTS = list(verdict_scripts())
SD, SP, TOL, MAX_ITER = 10.0, 100.0, 1e-12, 7


@pytest.mark.parametrize('name,script', VERDICTS, ids=[v[0] for v in VERDICTS])
def test_verdict(name, script, seen):
    """Every row is judged (the replay does not stop at a verdict): near_opt carries from row to row as it does from iteration to iteration."""
    rows = np.zeros((len(script), 8))
    rows[:, :5] = script
    rows[:, 5] = np.arange(len(script)) % 3                    # row count of the QP: 0 every third row
    out, _ = replay('verdict', rows, [SD, SP, TOL, MAX_ITER, 0.0])
    near_opt = False
    for i, (ok, mu, rd, rp, it) in enumerate(script):
        before = near_opt
        want, near_opt = ladder(ok != 0.0, mu, rd, rp, SD, SP, TOL, int(it), MAX_ITER, near_opt)
        assert (out[i, 0], out[i, 1]) == (want, float(near_opt)), (name, i)
        assert out[i, 2] == (GO_ON if ok != 0.0 else 2)        # starting and corrector systems: no certificate to fall back on
        assert out[i, 3] == (0 if i % 3 == 0 else GO_ON)       # no rows: the starting system's answer is the minimiser
        seen['status_%d' % want] += 1
        failed = ok == 0.0 or mu != mu or rd != rd
        if failed and before:
            seen['near_opt_saves_%d' % (2 if ok == 0.0 else (5 if mu != mu else 6))] += 1


BRANCHES = ('dt_binds', 'dl_binds', 'neither_binds', 'zmax_ge_0', 'zmax_lt_0', 'zmin_le_0', 'zmin_gt_0', 't_floor_active', 't_floor_inactive',
            'lam_floor_active', 'lam_floor_inactive', 'poison', 'mu_zero', 'amax_above_1', 'step_cut_below_1', 'affine_full_step_cut',
            'status_0', 'status_1', 'status_2', 'status_5', 'status_6', 'status_-1', 'near_opt_saves_2', 'near_opt_saves_5', 'near_opt_saves_6')


def test_inputs_take_every_branch_of_the_rule(seen):
    """Runs the tests above on a counter of its own, so that it holds whichever tests were selected."""
    mine = collections.Counter()
    for seed in SEEDS:
        for pred in (True, False):
            test_direction_and_step_bounds(seed, pred, mine)
        for amax in AMAX:
            test_affine_term_sigma_and_step_lengths(seed, amax, mine)
    for zmin, zmax in SHIFTS:
        test_cold_start(zmin, zmax, mine)
    for poison in (False, True):
        test_warm_start(poison, mine)
    for name, script in VERDICTS:
        test_verdict(name, script, mine)
    print(dict(mine))
    assert all(mine[b] > 0 for b in BRANCHES), {b: mine[b] for b in BRANCHES}
