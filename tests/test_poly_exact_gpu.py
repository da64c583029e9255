"""GPU: csrc/poly.hip (spoly_project) against the certified long-double reference of tests/poly_reference.py on every family of
tests/poly_cases.py, through ctypes, so that the batch argument, the return code and the message are under test; a few calls go
through Polyhedron.project_to_polyhedron.

For every certified point, with bound = pc.bound_for (1e-9 scale, or the measured well-separated bound where the margin is at least
1e-3 scale; scale = max(1, |x|_inf, |b|_inf)):
    |p - p*|_2 <= bound;  the KKT residuals of p (pr.kkt_residuals at tolerance bound) <= bound;  max(A p - b) <= bound;
    projecting p again moves it by no more than bound;  a point with max(A x - b) <= 0 comes back bit for bit.
A member of a batch equals the same point projected alone bit for bit.  An empty polyhedron and a non-finite point make the call
fail with a message that names the point.  Every output sits between sentinels that are checked after the call.

`pytest -s` prints one line per case and one per family (worst error, the margin it occurred at, the bound): profiles/poly_exact.log
is that output."""
import ctypes as C

import numpy as np
import pytest

import poly_cases as pc
import poly_reference as pr

pytestmark = pytest.mark.gpu

CASES = pc.cases()
SENTINEL = -7.25e77
PAD = 16
L = np.longdouble


def spoly(A, b, X):
    """(rc, message, out) of one spoly_project call; the output between sentinels."""
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    A, b, X = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, X))
    batch, n = X.shape
    buf = np.full(batch * n + 2 * PAD, SENTINEL)
    out = buf[PAD:PAD + batch * n]
    rc = lib.spoly_project(_lib.dptr(A), _lib.dptr(b), C.c_int(A.shape[0]), C.c_int(n), _lib.dptr(X), C.c_int64(batch),
                           out.ctypes.data_as(C.POINTER(C.c_double)))
    msg = lib.srh_last_error().decode(errors='replace') if rc != 0 else ''
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + batch * n:] == SENTINEL).all(), 'write outside the output'
    return rc, msg, out.reshape(batch, n).copy()


def projected(A, b, X):
    rc, msg, out = spoly(A, b, X)
    assert rc == 0, msg
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dist(p, q):
    d = np.asarray(p, dtype=L) - np.asarray(q, dtype=L)
    return float(np.sqrt((d * d).sum()))


_results = {}


def result(case):
    """The kernel's points of a case (one launch), and of those points projected again (a second launch); computed once."""
    if case.key not in _results:
        P = projected(case.A, case.b, case.X)
        _results[case.key] = (P, projected(case.A, case.b, P))
    return _results[case.key]


def measure(case):
    """[(error, margin, bound, scale, stationarity, feasibility, violation, moved)] per point."""
    P, P2 = result(case)
    rows = []
    for i, (x, r) in enumerate(zip(case.X, pc.certified(case))):
        bound, sc = pc.bound_for(case, i), pr.scale_of(case.b, x)
        stat, feas, _ = pr.kkt_residuals(case.A, case.b, x, P[i], bound)
        viol = float((case.A.astype(L) @ P[i].astype(L) - case.b.astype(L)).max())
        rows.append((dist(P[i], r.p), r.margin, bound, sc, stat, feas, viol, dist(P2[i], P[i])))
    return rows


def line(key, rows):
    w = max(rows, key=lambda r: r[0] / r[2])
    return ('%-24s %3d points: worst error %.2e (%.2e of the bound %.2e) at margin %.2e; worst stationarity %.2e, violation %.2e, '
            'moved by a second projection %.2e' % (key, len(rows), w[0], w[0] / w[2], w[2], w[1], max(r[4] for r in rows),
                                                    max(r[6] for r in rows), max(r[7] for r in rows)))


@pytest.mark.parametrize('key', [c.key for c in CASES])
def test_against_the_certified_reference(key):
    case = [c for c in CASES if c.key == key][0]
    P, _ = result(case)
    rows = measure(case)
    print(line(key, rows))
    inside = (case.X @ case.A.T - case.b).max(axis=1) <= 0
    assert np.array_equal(bits(P[inside]), bits(case.X[inside])), 'a point inside the polyhedron was changed'
    for i, (err, margin, bound, sc, stat, feas, viol, moved) in enumerate(rows):
        assert err <= bound, (key, i, 'error', err, 'bound', bound, 'margin', margin)
        assert stat <= bound and feas <= bound, (key, i, 'kkt', stat, feas, bound)
        assert viol <= bound, (key, i, 'violation', viol, bound)
        assert moved <= bound, (key, i, 'second projection moved by', moved, bound)


def test_summary_by_family_and_the_well_separated_measurement():
    fam = {}
    for c in CASES:
        fam.setdefault(c.family, []).extend(measure(c))
    for f, rows in fam.items():
        print(line('family ' + f, rows))
    ws = [r for rows in fam.values() for r in rows if r[1] >= pc.WELL_SEPARATED_MARGIN * r[3]]
    worst = max(r[0] / r[3] for r in ws)
    print('well separated (margin >= %.0e scale): %d points, worst error %.3e scale; asserted %.3e scale (contract %.0e scale)'
          % (pc.WELL_SEPARATED_MARGIN, len(ws), worst, pc.WELL_SEPARATED, pr.CONTRACT))
    rest = [r for rows in fam.values() for r in rows if r[1] < pc.WELL_SEPARATED_MARGIN * r[3]]
    print('the rest (%d points): worst error %.3e scale' % (len(rest), max(r[0] / r[3] for r in rest)))
    assert pc.WELL_SEPARATED <= pr.CONTRACT and worst <= pc.WELL_SEPARATED
    assert len(ws) >= 60 and len(rest) >= 40


def test_points_on_the_boundary_come_back_bit_for_bit():
    """On a face, at a vertex, inside, with -0.0 coordinates: viol == 0, the output is the input with its signs of zero."""
    case = [c for c in CASES if c.key == 'boundary/on'][0]
    P, P2 = result(case)
    assert np.array_equal(bits(P), bits(case.X)) and np.array_equal(bits(P2), bits(case.X))
    assert np.signbit(P[3, 1]) and np.signbit(P[4]).all()


@pytest.mark.parametrize('count', [1, 64, 65])
def test_a_batch_member_equals_the_point_projected_alone(count):
    case = [c for c in CASES if c.key == 'batch/n5_r13'][0]
    X = case.X[1:2] if count == 1 else case.X[:count]                  # the single point is an outside one
    P = projected(case.A, case.b, X)
    for i in range(len(X)):
        alone = projected(case.A, case.b, X[i:i + 1])
        assert np.array_equal(bits(P[i]), bits(alone[0])), i
    inside = (X @ case.A.T - case.b).max(axis=1) <= 0
    assert inside.sum() == (0 if count == 1 else (count + 1) // 2)
    assert np.array_equal(bits(P[inside]), bits(X[inside]))
    full, _ = result(case)
    assert np.array_equal(bits(P), bits(full[1:2] if count == 1 else full[:count]))


def test_through_the_polyhedron_class():
    from sofacontrol_amd.utils import Polyhedron
    case = [c for c in CASES if c.key == 'batch/n5_r13'][0]
    full, _ = result(case)
    Y = Polyhedron(case.A, case.b, with_reproject=True)
    got = Y.project_to_polyhedron(case.X[:7])
    assert got.shape == (7, 5) and np.array_equal(bits(got), bits(full[:7]))
    one = Y.project_to_polyhedron(case.X[3])
    assert one.shape == (5,) and np.array_equal(bits(one), bits(full[3]))
    lad = [c for c in CASES if c.key == 'ladder/box3'][0]
    corner = Polyhedron(lad.A, lad.b, with_reproject=True).project_to_polyhedron(lad.X[len(pc.LADDER) - 1])
    assert dist(corner, [1.0, 1.0, 0.0]) <= pr.CONTRACT * 2.0


@pytest.mark.parametrize('name', pc.FAILURES)
def test_failures_name_the_point(name):
    A, b, X, idx, word = pc.failure(name)
    rc, msg, out = spoly(A, b, X)
    print('%s: rc %d, %r' % (name, rc, msg))
    assert rc != 0, 'the call succeeded and returned %r' % (out,)
    assert 'spoly_project' in msg and ('point %d' % idx) in msg and word in msg, msg
    from sofacontrol_amd.utils import Polyhedron
    with pytest.raises(Exception, match='spoly_project'):
        Polyhedron(A, b, with_reproject=True).project_to_polyhedron(X)


def test_a_non_finite_polyhedron_is_refused():
    A, b = pc.box(2)
    for bad in (np.nan, np.inf):
        A2 = A.copy(); A2[1, 0] = bad
        rc, msg, _ = spoly(A2, b, [[3.0, 0.0]])
        assert rc != 0 and 'spoly_project' in msg and 'finite' in msg, (rc, msg)
        b2 = b.copy(); b2[2] = bad
        rc, msg, _ = spoly(A, b2, [[3.0, 0.0]])
        assert rc != 0 and 'spoly_project' in msg and 'finite' in msg, (rc, msg)
