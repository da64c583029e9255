"""No GPU: the certified reference of the polyhedron projection (tests/poly_reference.py) on every case of tests/poly_cases.py.

Every non-failure case is certified, none is left out; on the failure cases the reference reports an empty polyhedron; the
reference equals a brute-force enumeration for n <= 3 and the construction on the constructed families; `kkt_residuals`, the
second opinion of the GPU test, rejects a point that is 1e-12 off at the tolerance that test uses."""
import numpy as np
import pytest

import poly_cases as pc
import poly_reference as pr

CASES = pc.cases()
L = np.longdouble


def dist(p, q):
    d = np.asarray(p, dtype=L) - np.asarray(q, dtype=L)
    return float(np.sqrt((d * d).sum()))


def test_every_case_is_certified_and_none_is_left_out():
    keys = [c.key for c in CASES]
    assert len(set(keys)) == len(keys)
    assert {c.family for c in CASES} == {'limits', 'ladder', 'boundary', 'degenerate', 'scale', 'batch'}
    assert {(n, r) for n in pc.LIMIT_N for r in pc.LIMIT_ROWS} <= {(c.A.shape[1], c.A.shape[0]) for c in CASES if c.family == 'limits'}
    total = 0
    for c in CASES:
        assert 0 < c.A.shape[1] <= 16 and 0 < c.A.shape[0] <= 64 and len(c.X) <= 65
        got = pc.certified(c)                                   # raises NotCertified / Infeasible: no case may
        assert len(got) == len(c.X)
        for x, r in zip(c.X, got):
            tol = pr.CERT * pr.scale_of(c.b, x)
            assert r.violation <= tol and r.min_lam >= -tol and r.margin >= 0
            assert (r.lam[[i for i in range(len(c.b)) if i not in r.W]] == 0).all()
            # stationarity and complementarity of the returned pair, evaluated afresh in long double
            A, b = c.A.astype(L), c.b.astype(L)
            assert float(np.abs(r.p - x.astype(L) + A.T @ r.lam).max()) <= 64 * tol * max(1.0, float(np.abs(c.A).max()))
            assert float(np.abs(r.lam * (b - A @ r.p)).max()) <= 64 * tol * max(1.0, float(r.lam.max()))
            total += 1
    assert total == pc.n_points() and total <= 300
    print('%d cases, %d points certified' % (len(CASES), total))


@pytest.mark.parametrize('name', ['empty', 'empty_in_batch'])
def test_the_reference_reports_an_empty_polyhedron(name):
    A, b, X, _, _ = pc.failure(name)
    for x in X:
        with pytest.raises(pr.Infeasible):
            pr.project(A, b, x)


@pytest.mark.parametrize('name', [f for f in pc.FAILURES if 'nan' in f or 'inf' in f])
def test_the_reference_refuses_non_finite_points(name):
    A, b, X, idx, _ = pc.failure(name)
    for i, x in enumerate(X):
        if i == idx:
            with pytest.raises(ValueError):
                pr.project(A, b, x)
        else:
            pr.project(A, b, x)


def test_the_reference_equals_the_enumeration_up_to_three_dimensions():
    n_checked, worst = 0, 0.0
    for c in CASES:
        if c.A.shape[1] > 3 or len(c.X) > 12:
            continue
        for x, r in zip(c.X, pc.certified(c)):
            want = pr.enumerate_projection(c.A, c.b, x)
            assert want is not None, c.key
            e = dist(r.p, want) / pr.scale_of(c.b, x)
            worst = max(worst, e)
            assert e <= 2.0 ** -60, (c.key, e)              # 1e-18: both are long-double solves of the same equalities
            n_checked += 1
    print('%d points against the enumeration, worst relative distance %.2e' % (n_checked, worst))
    assert n_checked >= 60


def test_the_reference_equals_the_construction():
    """x was formed as p* + A_W^T lam* in float64: p* and lam* are the solution of the rounded x to one float64 rounding of x."""
    for key in ('ladder/box3', 'boundary/outside', 'boundary/on'):
        c = [c for c in CASES if c.key == key][0]
        for i, (x, r) in enumerate(zip(c.X, pc.certified(c))):
            assert dist(r.p, c.p_star[i]) <= 2 * np.finfo(np.float64).eps * pr.scale_of(c.b, x), (key, i)
            if c.lam_star is not None:
                assert float(np.abs(r.lam - c.lam_star[i]).max()) <= 2 * np.finfo(np.float64).eps * pr.scale_of(c.b, x), (key, i)


def test_the_margins_the_ladder_claims_are_the_margins_reported():
    c = [c for c in CASES if c.key == 'ladder/box3'][0]
    got = [r.margin for r in pc.certified(c)]
    print('claimed', c.margin, 'reported', got)
    np.testing.assert_allclose(got, c.margin, rtol=0, atol=2.0 ** -62)
    assert got[len(pc.LADDER) - 1] == 0.0                               # the weakly active corner
    # scale is 2 here (x0 = 2): only lam* = 1 is well separated, every other rung is held to the contract bound
    ws = [g >= pc.WELL_SEPARATED_MARGIN * pr.scale_of(c.b, x) for g, x in zip(got, c.X)]
    assert ws == [True] + [False] * 7


def _well_separated_point():
    c = [c for c in CASES if c.key == 'batch/n5_r13'][0]
    for i in range(1, len(c.X), 2):
        r = pc.certified(c)[i]
        if r.margin >= pc.WELL_SEPARATED_MARGIN * pr.scale_of(c.b, c.X[i]) and 1 <= len(r.W) < c.A.shape[1]:
            return c, i, r
    raise AssertionError('no well-separated outside point with a face to move along')


def test_the_certificate_accepts_the_reference_and_rejects_a_point_1e_12_off():
    c, i, r = _well_separated_point()
    x = c.X[i]
    tol = pc.bound_for(c, i)                                  # the tolerance tests/test_poly_exact_gpu.py uses for this point
    stat, feas, _ = pr.kkt_residuals(c.A, c.b, x, r.p, tol)
    print('reference: stationarity %.2e feasibility %.2e at tolerance %.2e' % (stat, feas, tol))
    assert stat <= tol and feas <= tol
    # along the face: a unit vector orthogonal to every active normal
    _, _, Vt = np.linalg.svd(c.A[r.W])
    t = Vt[-1]
    assert np.abs(c.A[r.W] @ t).max() <= 1e-14
    stat_t, feas_t, _ = pr.kkt_residuals(c.A, c.b, x, r.p + L(1e-12) * t.astype(L), tol)
    # into the interior: against the normal of the first active row
    a = c.A[r.W[0]]
    stat_i, feas_i, _ = pr.kkt_residuals(c.A, c.b, x, r.p - L(1e-12) * (a / np.linalg.norm(a)).astype(L), tol)
    print('moved 1e-12 along the face: stationarity %.2e; into the interior: stationarity %.2e' % (stat_t, stat_i))
    assert tol < 1e-12
    assert stat_t > tol and stat_i > tol
    # out of the polyhedron: infeasible by 1e-12 |a|
    _, feas_o, _ = pr.kkt_residuals(c.A, c.b, x, r.p + L(1e-12) * (a / np.linalg.norm(a)).astype(L), tol)
    assert feas_o > tol


def test_the_certificate_rejects_at_the_contract_bound_what_is_outside_it():
    """At the tolerance of the cases that are not well separated, 1e-9 scale, a point 4e-9 off is refused: the weakly active
    corner of the ladder moved along its face, into the interior and outwards."""
    c = [c for c in CASES if c.key == 'ladder/box3'][0]
    i = len(pc.LADDER) - 1
    r, x = pc.certified(c)[i], c.X[i]
    tol = pr.CONTRACT * pr.scale_of(c.b, x)
    assert pc.bound_for(c, i) == tol
    stat, feas, _ = pr.kkt_residuals(c.A, c.b, x, r.p, tol)
    assert stat <= tol and feas <= tol
    for d in ([0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]):
        s, f, _ = pr.kkt_residuals(c.A, c.b, x, r.p + L(4e-9) * np.array(d, dtype=L), tol)
        assert s > tol, d
    for d in ([1.0, 0, 0], [0, 1.0, 0]):
        s, f, _ = pr.kkt_residuals(c.A, c.b, x, r.p + L(4e-9) * np.array(d, dtype=L), tol)
        assert f > tol, d


def test_kkt_residuals_on_duplicated_and_degenerate_rows():
    for key in ('degenerate/duplicated', 'degenerate/vertex20', 'degenerate/equality'):
        c = [c for c in CASES if c.key == key][0]
        for x, r in zip(c.X, pc.certified(c)):
            tol = 1e-14 * pr.scale_of(c.b, x)
            stat, feas, lam = pr.kkt_residuals(c.A, c.b, x, r.p, tol)
            assert stat <= tol and feas <= tol and (lam >= 0).all(), (key, stat, feas)


def test_the_restated_kernel_reaches_the_iteration_limit_under_the_old_exit_and_not_under_the_certified_one():
    """tests/poly_restatement.py, float64: under the exit the kernel had (feasibility alone after 60 iterations) the 64-row family
    holds points that run to the limit and are accepted there; with the closing step no point comes near it."""
    import poly_restatement as rs
    c = [c for c in CASES if c.key == 'limits/full_n16'][0]
    old = [rs.project(c.A, c.b, x, 'feasible') for x in c.X]
    new = [rs.project(c.A, c.b, x, 'certified') for x in c.X]
    print('iterations, old exit:', [r[2] for r in old], 'certified:', [r[2] for r in new])
    assert max(r[2] for r in old) > 40 and all(r[1] == 0 for r in old)          # accepted at the limit, unchecked
    assert max(r[2] for r in new) <= 40 and all(r[1] == 0 for r in new)


def test_the_restated_kernel_meets_the_bounds_on_every_case():
    """The algorithm, before the device's reduction order: every point within its bound, every failure case reported."""
    import poly_restatement as rs
    worst = 0.0
    for c in CASES:
        for i, (x, r) in enumerate(zip(c.X, pc.certified(c))):
            p, st, it, _ = rs.project(c.A, c.b, x, 'certified')
            assert st == 0, (c.key, i)
            assert dist(p, r.p) <= pc.bound_for(c, i), (c.key, i, dist(p, r.p), pc.bound_for(c, i))
            worst = max(worst, dist(p, r.p) / pr.scale_of(c.b, x))
    print('worst error of the restatement %.2e scale' % worst)
    for name in ('empty', 'empty_in_batch'):
        A, b, X, _, _ = pc.failure(name)
        assert all(rs.project(A, b, x, 'certified')[1] != 0 for x in X)
