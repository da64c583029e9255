"""ipm::converged and ipm::may_converge (csrc/ipm_rule.h), the stopping test the lean interior points evaluate before they build a
predictor's Newton system, through the host replay (sqp_ipm_rule_replay, phase 'converged'): against the line of the stopping ladder
they were taken from -- oracle/condensed_ipm.py:290, restated below -- one ulp below, at and above each threshold, with the tolerance
below and above the 1e-9 floor of the linear residuals, and with NaN in every argument (never "converged").  And the ladder itself
(ipm::verdict, now stated through ipm::converged) on the scripts of tests/test_ipm_rule_cpu.py: unchanged."""
import itertools

import numpy as np
import pytest

from test_ipm_rule_cpu import MAX_ITER, SD, SP, TOL, VERDICTS, ladder, replay

NAN = float('nan')


def line_290(mu, rd, rp, sd, sp, tol):
    ltol = max(tol, 1e-9) if tol == tol else 1e-9          # (fmax ignores a NaN)
    return bool(rd <= ltol * sd and rp <= ltol * sp and mu <= tol)


def gate(mu, rp, sp, tol):
    ltol = max(tol, 1e-9) if tol == tol else 1e-9
    return bool(rp <= ltol * sp and mu <= tol)


def around(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def ask(cases, sd, sp, tol):
    rows = np.zeros((len(cases), 8))
    rows[:, 1:4] = cases                                     # mu, rd, rp
    out, _ = replay('converged', rows, [sd, sp, tol])
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize('tol', [1e-12, 1e-10, np.nextafter(1e-9, 0.0), 1e-9, np.nextafter(1e-9, 1.0), 1e-8, 1e-6])
@pytest.mark.parametrize('sd,sp', [(10.0, 100.0), (1.0, 1.0), (3.7e3, 2.9e-2)])
def test_grid_around_each_threshold(tol, sd, sp):
    ltol = max(tol, 1e-9)
    cases = list(itertools.product(around(tol), around(ltol * sd), around(ltol * sp)))           # mu, rd, rp
    conv, may = ask(cases, sd, sp, tol)
    seen = set()
    for i, (mu, rd, rp) in enumerate(cases):
        assert conv[i] == float(line_290(mu, rd, rp, sd, sp, tol)), (mu, rd, rp)
        assert may[i] == float(gate(mu, rp, sp, tol)), (mu, rp)
        assert conv[i] <= may[i]                             # the gate never closes on a converged iterate
        seen.add((conv[i], may[i]))
    assert seen == {(1.0, 1.0), (0.0, 1.0), (0.0, 0.0)}      # rd alone misses; the gate misses; all hold


@pytest.mark.parametrize('where', ['mu', 'rd', 'rp', 'sd', 'sp', 'tol'])
def test_nan_is_not_converged(where):
    good = dict(mu=1e-13, rd=1e-9, rp=1e-8, sd=10.0, sp=100.0, tol=1e-12)
    conv, may = ask([[good['mu'], good['rd'], good['rp']]], good['sd'], good['sp'], good['tol'])
    assert (conv[0], may[0]) == (1.0, 1.0)
    bad = dict(good, **{where: NAN})
    conv, may = ask([[bad['mu'], bad['rd'], bad['rp']]], bad['sd'], bad['sp'], bad['tol'])
    assert conv[0] == 0.0
    assert may[0] == (1.0 if where in ('rd', 'sd') else 0.0)          # the gate reads neither rd nor its scale
    assert conv[0] == float(line_290(**bad)) and may[0] == float(gate(bad['mu'], bad['rp'], bad['sp'], bad['tol']))


@pytest.mark.parametrize('name,script', VERDICTS, ids=[v[0] for v in VERDICTS])
def test_the_ladder_returns_what_it_returned(name, script):
    """ipm::verdict on the scripts of tests/test_ipm_rule_cpu.py, and on every row: verdict 0 from a sound system <=> ipm::converged"""
    rows = np.zeros((len(script), 8))
    rows[:, :5] = script
    out, _ = replay('verdict', rows, [SD, SP, TOL, MAX_ITER, 0.0])
    conv, may = ask([r[1:4] for r in script], SD, SP, TOL)
    near_opt = False
    for i, (ok, mu, rd, rp, it) in enumerate(script):
        want, near_opt = ladder(ok != 0.0, mu, rd, rp, SD, SP, TOL, int(it), MAX_ITER, near_opt)
        assert (out[i, 0], out[i, 1]) == (want, float(near_opt)), (name, i)
        assert conv[i] == float(line_290(mu, rd, rp, SD, SP, TOL)), (name, i)
        if ok != 0.0 and mu == mu and rd == rd:
            assert (want == 0) == bool(conv[i]), (name, i)
        if conv[i]:
            assert may[i] == 1.0 and want in (0, 2), (name, i)          # 2: the breakdown at a converged iterate
