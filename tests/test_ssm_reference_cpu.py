"""No GPU: the long-double statement of the SSM model (tests/ssm_reference.py) against exact rational arithmetic, the float64
oracle (oracle/ssm.py) against the long-double statement on every case of tests/ssm_cases.py -- the measured e_oracle that
sets the tolerance of tests/test_ssm_exact_gpu.py, with its input condition e_oracle <= 1e-11 asserted here -- and the host
side of csrc/ssm.hip: exponent table, the elimination path every shape is listed for, the order and n_u refusals of sssm_create."""
from fractions import Fraction

import numpy as np
import pytest

import ssm_cases as sc
import ssm_reference as sr
from oracle import ssm as ossm


def frac_phi(E, x):
    out = []
    for e in E:
        v = Fraction(1)
        for i, p in enumerate(e):
            v *= x[i] ** int(p)
        out.append(v)
    return out


def frac_dphi(E, x):
    D = []
    for e in E:
        row = []
        for i in range(len(x)):
            if e[i] == 0:
                row.append(Fraction(0))
                continue
            v = Fraction(int(e[i]))
            for k, p in enumerate(e):
                v *= x[k] ** (int(p) - (1 if k == i else 0))
            row.append(v)
        D.append(row)
    return D


def rel_to_fraction(got, exact):
    """max |got - exact| / max(1, max|exact|), the difference formed in rational arithmetic (a long double is a dyadic rational:
    the digits beyond binary64 go through as a second float)."""
    def frac(v):
        hi = float(v)
        return Fraction(hi) + Fraction(float(v - sr.LD(hi)))
    g, e = np.ravel(got), list(exact)
    assert len(g) == len(e)
    scale = max(Fraction(1), max(abs(v) for v in e))
    return float(max(abs(frac(a) - b) for a, b in zip(g, e)) / scale)


@pytest.mark.parametrize('s', [(2, 3, 4, 1), (1, 1, 7, 7)], ids=sc.shape_id)
def test_reference_against_exact_arithmetic(s):
    """phi, dphi, A = R dphi and d = f - A x - B u in fractions.Fraction from the float64 inputs: the long-double statement agrees
    to 1e-18 relative (its own rounding: eps 1.1e-19 times the few dozen operations of these shapes)."""
    n, m = s[0], s[1]
    d = sc.model(s)
    M = sc.reference_model(d)
    X, U, _ = sc.points(s)
    F = lambda a: [[Fraction(float(v)) for v in row] for row in np.atleast_2d(a)]
    R, B = F(d['R']), F(d['B'])
    worst = 0.0
    for x, u in zip(X, U):
        xf, uf = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in u]
        ph, D = frac_phi(M['Er'], xf), frac_dphi(M['Er'], xf)
        A = [[sum(R[i][k] * D[k][j] for k in range(len(ph))) for j in range(n)] for i in range(n)]
        f = [sum(R[i][k] * ph[k] for k in range(len(ph))) + sum(B[i][k] * uf[k] for k in range(m)) for i in range(n)]
        dd = [f[i] - sum(A[i][j] * xf[j] for j in range(n)) - sum(B[i][k] * uf[k] for k in range(m)) for i in range(n)]
        Ar, _, dr = sr.continuous_jacobians(M, x, u)
        es = (rel_to_fraction(sr.phi(M['Er'], x), ph), rel_to_fraction(sr.dphi(M['Er'], x), [v for row in D for v in row]),
              rel_to_fraction(Ar, [v for row in A for v in row]), rel_to_fraction(dr, dd))
        worst = max(worst, *es)
    print('ssm_reference %s against exact arithmetic: worst relative error %.2e over %d points (phi, dphi, A, d)' % (sc.shape_id(s), worst, len(X)))
    assert worst <= 1e-18


def test_reference_inverse_pivots_on_the_first_maximum_and_refuses_a_zero_pivot():
    """Two equal maxima in the first column: row 0 stays (no exchange); the exact case's A_c needs its two exchanges; a zero pivot
    raises like np.linalg.inv."""
    inv, swaps = sr.inverse([[2.0, 1.0], [-2.0, 3.0]])
    assert swaps == 0
    np.testing.assert_array_equal(np.asarray(inv, dtype=float), [[0.375, -0.125], [0.25, 0.25]])
    d, _, _, _ = sc.exact_case()
    inv, swaps = sr.inverse(d['R'])
    assert swaps == 2
    np.testing.assert_array_equal(np.asarray(inv @ sr.ld(d['R']), dtype=float), np.eye(4))
    _, swaps = sr.inverse(np.eye(4) - 0.5 * d['R'])
    assert swaps == 0
    with pytest.raises(np.linalg.LinAlgError):
        sr.inverse([[0.0, 0.0], [0.0, -1.0]])


@pytest.mark.parametrize('dim,order', [(1, 7), (2, 4), (3, 3), (6, 2), (10, 3), (32, 1)])
def test_exponent_tables_agree(dim, order):
    """The reference's table (multisets of variable indices), the oracle's (recursion) and the library's host function."""
    import ctypes as C
    from sofacontrol_amd import _lib
    E = sr.exponents(dim, order)
    np.testing.assert_array_equal(E, ossm.exponents(dim, order))
    nm = _lib.lib().sssm_num_monomials(C.c_int(dim), C.c_int(order))
    assert nm == E.shape[0]
    got = np.empty((nm, dim), dtype=np.int32)
    _lib.check(_lib.lib().sssm_exponents(C.c_int(dim), C.c_int(order), _lib.iptr(got)), 'sssm_exponents')
    np.testing.assert_array_equal(got, E)


@pytest.mark.parametrize('s', sc.SHAPES, ids=sc.shape_id)
def test_oracle_against_reference(s):
    """e_oracle per shape, model kernels and rollouts, printed per path; the input condition of the tolerance rule."""
    _, e_oracle, per_path = sc.reference(s)
    _, e_roll = sc.rollout_reference(s)
    cond = max(np.linalg.cond(sr.continuous_jacobians(sc.reference_model(sc.model(s)), x, u)[0].astype(float)) for x, u, in zip(*sc.points(s)[:2]))
    print('ssm_reference %-14s e_oracle %.2e (tol %.2e) rollout %.2e (tol %.2e) cond(A_c) <= %.1e | %s'
          % (sc.shape_id(s), e_oracle, sc.tolerance(e_oracle), e_roll, sc.tolerance(e_roll), cond,
             ' '.join('%s %.1e' % kv for kv in sorted(per_path.items()))))
    assert e_oracle <= sc.E_ORACLE_MAX and e_roll <= sc.E_ORACLE_MAX


def test_constructed_cases():
    """The exact case is exact (the float64 oracle, whatever route np.linalg.inv takes on these matrices, is not asked to be:
    only the long-double result must be representable in binary64); the rectangular reduce's e_oracle meets the input condition;
    the singular case is singular at its middle point only."""
    d, X, U, (method, _, dt) = sc.exact_case()
    M = sc.reference_model(d)
    for x, u in zip(X, U):
        for out in sr.jacobians(M, x, u, dt, method):
            np.testing.assert_array_equal(sr.ld(out.astype(np.float64)), out)
            assert np.all(out * 8 == np.round(out * 8))               # eighths at most
    _, _, _, e_rect = sc.rectangular_case()
    print('ssm_reference rectangular reduce (4 x 27): e_oracle %.2e (tol %.2e)' % (e_rect, sc.tolerance(e_rect)))
    d, X, U = sc.singular_case()
    M = sc.reference_model(d)
    for b, (x, u) in enumerate(zip(X, U)):
        for method, dt in (('be', 0.01), ('bil', 0.05)):
            if b == 1:
                with pytest.raises(np.linalg.LinAlgError):
                    sr.jacobians(M, x, u, dt, method)
            else:
                assert all(np.isfinite(o.astype(float)).all() for o in sr.jacobians(M, x, u, dt, method))
        assert all(np.isfinite(o.astype(float)).all() for o in sr.jacobians(M, x, u, 0.01, 'fe'))


@pytest.mark.parametrize('s', sc.SHAPES, ids=sc.shape_id)
def test_shapes_reach_their_listed_paths(s):
    """n * n against the thresholds of ssm::inverse_wave (stated once, tests/ssm_cases.py), the leading dimension and the scratch
    limits of csrc/ssm_dev.h that the shape is listed for."""
    n, m, ro, so = s
    assert sc.inverse_path(n) == sc.INVERSE_PATH[s]
    assert 1 <= n <= sc.N_X_MAX and m <= (n | 1) and max(ro, so) <= sc.SSM_MAX_ORDER
    if s in sc.STAGED_SHAPES:
        # the compact derivative values of jacobians_l live in Work::D: max(nr n, ns n_o) + 4 n doubles (ssm::work_doubles)
        Er, Es = sr.exponents(n, ro), sr.exponents(n, so)
        assert 4 * n * sc.jacobian_list_cap(Er) <= max(Er.size, Es.size) + 4 * n
        assert n <= 16 and m <= 16


def test_the_shape_list_covers_every_path_and_edge():
    paths = [sc.INVERSE_PATH[s] for s in sc.SHAPES]
    assert set(paths) == {'EP1', 'EP2', 'EP4', 'loop'}
    ns = [s[0] for s in sc.SHAPES]
    for edge in (1, 8, 9, 11, 12, 16, 17, sc.N_X_MAX):                  # both sides of every threshold, both ends of the range
        assert edge in ns
    assert any(s[1] == s[0] + 1 and s[0] % 2 == 0 for s in sc.SHAPES)   # the B_d scratch limit
    assert any(s[2] == 1 for s in sc.SHAPES) and any(max(s[2:]) == sc.SSM_MAX_ORDER for s in sc.SHAPES)
    assert set(sc.STAGED_SHAPES) <= set(sc.SHAPES)


def _create_rc(n, m, no, ro, so):
    """sssm_create with tiny coefficient arrays of the right sizes; returns (rc, message).  A refusal happens before any device call."""
    import ctypes as C
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    nr, ns = max(lib.sssm_num_monomials(C.c_int(n), C.c_int(ro)), 1), max(lib.sssm_num_monomials(C.c_int(no), C.c_int(so)), 1)
    z = lambda *sh: _lib.dptr(np.zeros(sh))
    h = C.c_void_p()
    rc = lib.sssm_create(C.byref(h), C.c_int(n), C.c_int(m), C.c_int(no), C.c_int(ro), C.c_int(so), z(n, nr), z(n, m), None, None, z(no, ns),
                         z(n, ns), z(no))
    assert rc != 0 and not h.value, 'these calls are refusals: nothing may have been created'
    return rc, lib.srh_last_error().decode()


@pytest.mark.parametrize('ro,so', [(8, 1), (1, 8), (8, 8), (9, 2)])
def test_create_refuses_orders_above_seven(ro, so):
    """SsmLds keeps order + 1 level offsets in eight slots: an order-8 model (n_x = 1: eight monomials, fits everywhere else) is
    refused at creation, with the limit in the message.  Host check: no device is touched."""
    rc, msg = _create_rc(1, 1, 1, ro, so)
    assert rc == -1 and '<= 7' in msg and 'order' in msg, (rc, msg)


@pytest.mark.parametrize('n,m', [(2, 4), (5, 6), (1, 2)])
def test_create_states_the_real_input_limit(n, m):
    """n_u <= n_x | 1: the message names the limit it enforces."""
    rc, msg = _create_rc(n, m, n, 2, 2)
    assert rc == -1 and 'n_u <= n_x | 1' in msg and '(= %d)' % (n | 1) in msg, (rc, msg)
