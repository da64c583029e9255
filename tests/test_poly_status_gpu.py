"""GPU: spoly_project_status (csrc/poly.hip), the stand-alone entry of the one-wave projection unit csrc/poly_dev.h -- the form the
closed-loop advance kernels use: a status word per point, never a failed call.

One batch mixes points inside, on a face, one ulp outside, outside with one, two and n active rows, and a NaN and an Inf point; a second
polyhedron is empty.  Asserted: the status words (0 inside, 1 projected, -1 no certified projection, -2 not finite); points with status
0, -1, -2 come back bit for bit; points with status 1 have the bits of spoly_project of the point alone; a member of the batch equals the
point alone; the entry agrees with spoly_project on every family of tests/poly_cases.py; nothing is written outside the outputs."""
import ctypes as C

import numpy as np
import pytest

import poly_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
PAD = 16
ULP1 = float(np.nextafter(1.0, 2.0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def status_call(A, b, X):
    """(rc, message, out, status) of one spoly_project_status call; both outputs between sentinels."""
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    A, b, X = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, X))
    batch, n = X.shape
    buf = np.full(batch * n + 2 * PAD, SENTINEL)
    sbuf = np.full(batch + 2 * PAD, 777, dtype=np.int32)
    out, st = buf[PAD:PAD + batch * n], sbuf[PAD:PAD + batch]
    rc = lib.spoly_project_status(_lib.dptr(A), _lib.dptr(b), C.c_int(A.shape[0]), C.c_int(n), _lib.dptr(X), C.c_int64(batch),
                                  out.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_int32)))
    msg = lib.srh_last_error().decode(errors='replace') if rc != 0 else ''
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + batch * n:] == SENTINEL).all(), 'write outside the points'
    assert (sbuf[:PAD] == 777).all() and (sbuf[PAD + batch:] == 777).all(), 'write outside the status words'
    return rc, msg, out.reshape(batch, n).copy(), st.copy()


def strict_alone(A, b, x):
    from sofacontrol_amd.utils import Polyhedron
    return Polyhedron(A, b, with_reproject=True).project_to_polyhedron(np.asarray(x, dtype=np.float64))


def mixed():
    """The box [-1, 1]^3 and the facet x0 + x1 + x2 <= 2.5: (A, b, X, expected status)."""
    A, b = pc.box(3)
    A, b = np.vstack([A, np.ones((1, 3))]), np.append(b, 2.5)
    X = [([0.2, -0.3, 0.1], 0), ([1.0, 0.3, -0.0], 0), ([1.0, 1.0, 0.5], 0),              # inside, on a face, on an edge and the facet
         ([ULP1, 0.3, 0.0], 1), ([2.0, 0.3, 0.0], 1),                                     # one active row
         ([2.0, -3.0, 0.2], 1), ([3.0, 4.0, 5.0], 1), ([-2.0, -2.0, -2.0], 1),            # two, then n active rows
         ([np.nan, 0.0, 0.0], -2), ([0.5, -np.inf, 0.0], -2), ([0.1, 0.2, np.nan], -2),
         ([0.0, 0.0, 0.0], 0), ([0.9, 0.9, 0.9], 1)]                                      # the oblique facet alone
    return A, b, np.array([x for x, _ in X]), np.array([s for _, s in X], dtype=np.int32)


def test_mixed_batch_status_and_bits():
    A, b, X, want = mixed()
    rc, msg, out, st = status_call(A, b, X)
    assert rc == 0, msg
    print('status words:', st.tolist())
    np.testing.assert_array_equal(st, want)
    for i, s in enumerate(st):
        if s == 1:
            np.testing.assert_array_equal(bits(out[i]), bits(strict_alone(A, b, X[i])), err_msg='point %d' % i)
            assert (A @ out[i] - b).max() <= 1e-12 * max(1.0, np.abs(X[i]).max(), np.abs(b).max())
        else:
            np.testing.assert_array_equal(bits(out[i]), bits(X[i]), err_msg='point %d (status %d)' % (i, s))
        rc1, _, o1, s1 = status_call(A, b, X[i:i + 1])
        assert rc1 == 0 and s1[0] == s
        np.testing.assert_array_equal(bits(o1[0]), bits(out[i]), err_msg='point %d alone' % i)
    # active rows as the case claims them
    act = lambda p: int((np.abs(A @ p - b) <= 1e-12).sum())
    assert [act(out[i]) for i in (4, 5, 6, 7, 12)] == [1, 2, 3, 3, 1]


def test_empty_polyhedron_is_a_status_not_a_failure():
    for name in ('empty', 'empty_in_batch'):
        A, b, X, _, _ = pc.failure(name)
        rc, msg, out, st = status_call(A, b, X)
        assert rc == 0, msg
        assert (st == -1).all(), st
        np.testing.assert_array_equal(bits(out), bits(X))


def test_non_finite_points_of_the_failure_cases():
    for name in ('nan', 'inf', 'nan_in_batch', 'inf_in_batch'):
        A, b, X, bad, _ = pc.failure(name)
        rc, msg, out, st = status_call(A, b, X)
        assert rc == 0, msg
        assert st[bad] == -2 and (np.delete(st, bad) >= 0).all(), (name, st)
        np.testing.assert_array_equal(bits(out[bad]), bits(X[bad]))
        good = [i for i in range(len(X)) if i != bad]
        if good:
            from sofacontrol_amd.utils import Polyhedron
            np.testing.assert_array_equal(bits(out[good]), bits(Polyhedron(A, b, with_reproject=True).project_to_polyhedron(X[good])))


@pytest.mark.parametrize('family', sorted({c.family for c in pc.cases()}))
def test_agrees_with_spoly_project_on_every_family(family):
    from sofacontrol_amd.utils import Polyhedron
    for c in [c for c in pc.cases() if c.family == family]:
        rc, msg, out, st = status_call(c.A, c.b, c.X)
        assert rc == 0, msg
        P = Polyhedron(c.A, c.b, with_reproject=True)
        np.testing.assert_array_equal(bits(out), bits(P.project_to_polyhedron(c.X)), err_msg=c.key)
        inside = ~((c.X @ c.A.T - c.b).max(axis=1) > 0)
        # (numpy's A x and the kernel's fma chain agree on which side every point of these cases lies: the boundary family is exact)
        np.testing.assert_array_equal(st, np.where(inside, 0, 1).astype(np.int32), err_msg=c.key)
        out2, st2 = P.project_with_status(c.X)
        np.testing.assert_array_equal(bits(out2), bits(out)); np.testing.assert_array_equal(st2, st)


def test_limits_and_non_finite_polyhedron_are_refused():
    A, b = pc.box(2)
    X = np.zeros((1, 2))
    bad = A.copy(); bad[1, 0] = np.nan
    rc, msg, _, _ = status_call(bad, b, X)
    assert rc != 0 and 'not finite' in msg and 'row 1' in msg
    rc, msg, _, _ = status_call(np.ones((65, 2)), np.ones(65), X)
    assert rc != 0 and '65' in msg
    rc, msg, _, _ = status_call(np.ones((2, 17)), np.ones(2), np.zeros((1, 17)))
    assert rc != 0 and '17' in msg
