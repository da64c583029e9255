"""CPU: the reference and the cases of the exact Koopman lift tests stand on their own -- the order of the observables is sympy's, the
case list reaches every tile class, the float64 twin is within its roundings of long double, the derived bound of W psi holds for numpy's
own product, and each decode error the device test is there to find is caught by the comparison that test makes."""
import numpy as np
import pytest

import koopman_lift_cases as kc
import koopman_lift_reference as kr


# --------------------------------------------------------------------------------------------------------------------------- order
@pytest.mark.parametrize('nz,degree', [(1, 4), (3, 2), (4, 4), (5, 3)])
def test_exponents_are_sympys_order(nz, degree):
    """get_lifting_function (koopman_utils.py:156-175): sorted(itermonomials(zeta, d), key=monomial_key('grlex', reversed(zeta))), the
    constant moved to the end (dropped for DMD)."""
    sympy = pytest.importorskip('sympy')
    from sympy.polys.monomials import itermonomials
    from sympy.polys.orderings import monomial_key
    z = sympy.symbols('z1:%d' % (nz + 1))
    poly = sorted(itermonomials(list(z), degree), key=monomial_key('grlex', list(reversed(z))))
    assert poly[0] == 1
    poly = poly[1:] + [poly[0]]
    E = np.array([[sympy.degree(p, v) if p != 1 else 0 for v in z] for p in poly], dtype=np.int64)
    assert np.array_equal(kr.exponents(nz, degree, False), E)
    assert np.array_equal(kr.exponents(nz, degree, True), E[:-1])


def test_psi_multiplies_ascending_left_to_right():
    E = kr.exponents(3, 3, False)
    z = np.array([[1.1, 1.3, 1.7]])
    k = [tuple(e) for e in E].index((2, 0, 1))
    assert kr.factors(E)[k] == [0, 0, 2]
    assert kr.psi(z, E, np.float64)[0, k] == (1.1 * 1.1) * 1.7
    assert kr.psi(z, E, np.float64)[0, -1] == 1.0 and not E[-1].any()
    # the parent of every observable (one removed from its last variable) is the observable of its leading factors
    F = kr.factors(E)
    for f in F[:-1]:
        assert len(f) == 1 or f[:-1] in F


# ------------------------------------------------------------------------------------------------------------------------ coverage
def test_case_table_is_the_restated_rule():
    for name in kc.LIFT_CASES:
        c = kc.case(name)
        assert kr.n_psi(c['nz'], c['degree'], c['dmd']) == c['P'] == len(kc.exps(c['nz'], c['degree'], c['dmd'])), name
        assert kr.tile_model(c['nz'], c['P']) == (c['ld'], c['TR'], c['lds']), name
    for nz, degree in kc.REFUSED:
        assert kr.n_psi(nz, degree, False) > kr.KP_MAX_PSI >= kr.n_psi(nz - 1, degree, False)


def test_case_table_reaches_every_class():
    cs = [kc.case(n) for n in kc.LIFT_CASES]
    assert {c['TR'] for c in cs} == {64, 32, 16}
    assert {c['P'] % 4 for c in cs} == {0, 1, 2, 3}
    assert {c['ld'] - c['P'] for c in cs} == {1, 2, 3, 4}
    lds = sorted(c['lds'] for c in cs)
    assert lds[0] == 2560 and any(v <= 64 * 1024 for v in lds) and any(v > 64 * 1024 for v in lds)
    assert 64000 in lds and 66560 in lds                      # the last request under 64 KiB and the first over it
    # the largest request any admissible handle makes, under the 160 KiB of a CU
    worst = max(kr.tile_model(nz, kr.n_psi(nz, d, dmd))[2] for nz in range(1, kr.KP_MAX_NZ + 1) for d in range(1, kr.KP_MAX_DEG + 1)
                for dmd in (False, True) if kr.n_psi(nz, d, dmd) <= kr.KP_MAX_PSI)
    assert worst == lds[-1] == 133120 < 160 * 1024
    # the neighbours of the class boundaries sit on the other side
    assert kr.tile_model(13, 105)[1] == 64 and kr.tile_model(14, 120)[1] == 32
    assert kr.tile_model(20, 231)[1] == 32 and kr.tile_model(21, 252)[1] == 16 and kr.tile_model(21, 253)[1] == 16
    assert kr.tile_model(19, 210)[2] <= 64 * 1024 < kr.tile_model(20, 231)[2]
    # one case per TR class runs every row count; W runs on each class and on both ~1000-observable tables
    assert {kc.LIFT_CASES[n][5] for n in kc.FULL_ROWS.values()} == {64, 32, 16}
    assert {kc.LIFT_CASES[n][5] for n in kc.W_CASES} == {64, 32, 16}
    for name in kc.LIFT_CASES:
        TR = kc.LIFT_CASES[name][5]
        assert {1, 17, TR + 1} <= set(kc.rows_of(name))
    for TR, name in kc.FULL_ROWS.items():
        assert {1, 15, 16, 17, TR - 1, TR, TR + 1, 2 * TR + 1} == set(kc.rows_of(name))
    assert {kc.record_dims(n)['TR'] for n in kc.RECORD_CASES} == {64, 32, 16}
    assert [kc.record_dims(n)['nz'] for n in kc.RECORD_CASES] == [1, 10, 7, 17, 60]
    assert sorted({kc.ring_dims(n)['delays'] for n in kc.RING_CASES}) == [0, 1, 2, 3]
    assert {kc.ring_dims(n)['TR'] for n in kc.RING_CASES} == {64, 32, 16}
    assert {kc.ring_dims(n)['TR'] for n in kc.RING_CASES if kc.ring_dims(n)['with_w']} == {64, 32, 16}


def test_integer_data_is_what_the_exactness_argument_needs():
    for name in kc.LIFT_CASES:
        c = kc.case(name)
        Z = kc.zeta(name, 'int')
        assert np.array_equal(Z, np.round(Z)) and np.abs(Z).max() <= 3 and np.all(np.abs(Z[:, -1]) == 3)
        room = 2 * 7 ** (c['nz'] - 1)
        distinct = len({tuple(r) for r in Z})
        assert distinct == min(len(Z), room), name
    for name in kc.W_CASES:
        P = kc.LIFT_CASES[name][3]
        for Nw in kc.nw_of(name):
            W = kc.w_of(name, Nw, 'int')
            assert W.shape == (Nw, P) and np.array_equal(W, np.round(W)) and np.abs(W).max() <= 8
            assert np.all(np.abs(W[:, -1]) == 8) and np.all(np.abs(W[-1]) == 8)
            assert not (Nw == P and np.array_equal(W, np.eye(P)))
            # the largest |sum| any order of accumulation can meet
            big = (np.abs(kc.psi_of(name, 'int', False)) @ np.abs(W).T).max()
            assert big <= 1001 * 81 * 8 < 2 ** 20 < 2 ** 53


# ------------------------------------------------------------------------------------------------------------ roundings and the bound
@pytest.mark.parametrize('name', list(kc.LIFT_CASES))
def test_float64_psi_is_within_its_roundings_of_long_double(name):
    c = kc.case(name)
    p64, pld = kc.psi_of(name, 'real', False), kc.psi_of(name, 'real', True)
    rel = np.abs(p64.astype(np.longdouble) - pld) / np.abs(pld)
    # (degree - 1) products, each within 2^-53 relative; the zeta entries themselves are the same doubles in both
    assert rel.max() <= (c['degree'] - 1) * np.longdouble(kr.U), (name, float(rel.max() / kr.U))
    # per observable: as many roundings as it has products
    nprod = np.array([max(len(f) - 1, 0) for f in kr.factors(kc.exps(c['nz'], c['degree'], c['dmd']))])
    assert np.all(rel.max(axis=0) <= nprod * np.longdouble(kr.U))
    # integer data: exact in both
    assert np.array_equal(kc.psi_of(name, 'int', False).astype(np.longdouble), kc.psi_of(name, 'int', True))


@pytest.mark.parametrize('name', kc.W_CASES)
def test_numpy_product_is_inside_the_bound_and_integer_products_are_exact(name):
    c = kc.case(name)
    worst = 0.0
    for Nw in kc.nw_of(name):
        ref, bound = kc.w_reference(name, Nw, 'real')
        got = kr.project(kc.psi_of(name, 'real', False), kc.w_of(name, Nw, 'real'), np.float64)
        frac = kr.bound_fraction(got, ref, bound)
        worst = max(worst, frac)
        assert kr.inside(got, ref, bound), (name, Nw, frac)
        # integer data: float64 equals Python-int arithmetic on sampled entries
        exp, none = kc.w_reference(name, Nw, 'int')
        assert none is None
        Pi, Wi = kc.psi_of(name, 'int', False), kc.w_of(name, Nw, 'int')
        rng = np.random.default_rng(Nw)
        for _ in range(12):
            r, j = int(rng.integers(0, Pi.shape[0])), int(rng.integers(0, Nw))
            assert int(exp[r, j]) == sum(int(a) * int(b) for a, b in zip(Pi[r], Wi[j])) and exp[r, j] == int(exp[r, j])
        assert np.abs(exp).max() < 2 ** 53
    print('%s: numpy float64 psi W^T at most %.3f of w_bound' % (name, worst))
    assert 0 < worst    # the bound is compared with something that does round


# ---------------------------------------------------------------------------------------------------------------------------- zeta
@pytest.mark.parametrize('name', list(kc.RECORD_CASES))
@pytest.mark.parametrize('kind', kc.KINDS)
def test_zeta_record_equals_zeta_ring(name, kind):
    d = kc.record_dims(name)
    sc = kc.scales(d['n_y'], d['m'], kind, name)
    T = d['delays'] + 5
    y, u = kc.samples(T, d['n_y'], d['m'], d['delays'], kind, sc, name)
    for dtype in (np.float64, np.longdouble):
        Zr = kr.zeta_record(y, u, d['delays'], sc, dtype)
        assert Zr.shape == (5, d['nz'])
        for r in range(5):
            t = r + d['delays']
            pushed = [(y[k:k + 1], u[k:k + 1]) for k in range(t + 1)]
            assert np.array_equal(Zr[r:r + 1], kr.zeta_ring(pushed, d['delays'], sc, dtype))
    assert kr.zeta_record(y[:d['delays']], u[:d['delays']], d['delays'], sc, np.float64).shape == (0, d['nz'])
    if kind == 'int':
        Z = kr.zeta_record(y, u, d['delays'], sc, np.float64)
        assert np.array_equal(Z, np.round(Z)) and np.abs(Z).max() <= 3 and np.all(np.abs(Z[:, -1]) == 3)
    # the layout, spelled out once: [y_t | y_{t-1} .. | u_{t-1} ..]
    Z = kr.zeta_record(y, u, d['delays'], sc, np.float64)
    ys, us = kr.scale_down(y, sc[0], sc[1], np.float64), kr.scale_down(u, sc[2], sc[3], np.float64)
    assert np.array_equal(Z[0, :d['n_y']], ys[d['delays']])
    if d['delays']:
        yb = d['n_y'] * (d['delays'] + 1)
        assert np.array_equal(Z[0, d['n_y']:2 * d['n_y']], ys[d['delays'] - 1])
        assert np.array_equal(Z[0, yb:yb + d['m']], us[d['delays'] - 1])
        assert np.array_equal(Z[0, -d['m']:], us[0])


# ----------------------------------------------------------------------------------------------------------------------- mutations
def _compare(got, name, Nw, kind, rows):
    """The device test's comparison of a lift of the first `rows` master rows: bits without W and on integer data, the bound otherwise."""
    if Nw is None:
        return kr.same_bits(got, kc.psi_of(name, kind, False)[:rows])
    ref, bound = kc.w_reference(name, Nw, kind)
    if kind == 'int':
        return kr.same_bits(got, ref[:rows])
    return kr.inside(got, ref[:rows], bound[:rows])


@pytest.mark.parametrize('name', list(kc.LIFT_CASES))
@pytest.mark.parametrize('kind', kc.KINDS)
def test_exchanged_observables_and_rows_are_caught(name, kind):
    c = kc.case(name)
    ps = kc.psi_of(name, kind, False)
    for rows in (17, c['TR'] + 1):
        good = ps[:rows]
        assert _compare(good.copy(), name, None, kind, rows)
        # one exponent row exchanged with its neighbour = two neighbouring columns exchanged: every such pair differs somewhere
        if c['P'] > 1:
            assert np.all((good[:, 1:] != good[:, :-1]).any(axis=0)), name
            for k in {0, c['P'] // 2 - 1, c['P'] - 2} - {-1}:
                bad = good.copy()
                bad[:, [k, k + 1]] = bad[:, [k + 1, k]]
                assert not _compare(bad, name, None, kind, rows)
        # two output rows exchanged (any two whose zeta rows differ: their degree-1 observables differ then; only nz = 1 on integer
        # data, two possible rows, has no room for all to differ)
        Z = kc.zeta(name, kind)
        assert not np.array_equal(Z[0], Z[1])
        for a, b in ((0, 1), (rows - 2, rows - 1), (0, rows - 1)):
            if np.array_equal(Z[a], Z[b]):
                assert c['nz'] == 1 and kind == 'int'
                continue
            bad = good.copy()
            bad[[a, b]] = bad[[b, a]]
            assert not _compare(bad, name, None, kind, rows), (name, a, b)


@pytest.mark.parametrize('name', kc.W_CASES)
def test_w_mutations_are_caught(name):
    c = kc.case(name)
    P, ld = c['P'], c['ld']
    rows = c['TR'] + 1
    for Nw in kc.nw_of(name):
        ps, W = kc.psi_of(name, 'int', False)[:rows], kc.w_of(name, Nw, 'int')
        assert _compare(kr.project(ps, W, np.float64), name, Nw, 'int', rows)
        # the last column of W dropped
        Wd = W.copy()
        Wd[:, P - 1] = 0.0
        assert not _compare(kr.project(ps, Wd, np.float64), name, Nw, 'int', rows)
        # the last k-step (k >= 4 (ld / 4 - 1)) left out: where P % 4 == 0 that step multiplies padding only and nothing is lost;
        # everywhere else it holds the constant column at the least
        k_last = 4 * (ld // 4 - 1)
        short = kr.project(ps[:, :k_last], W[:, :k_last], np.float64)
        assert _compare(short, name, Nw, 'int', rows) == (P % 4 == 0)
        # the last k-step that holds data
        k_data = 4 * ((P - 1) // 4)
        assert not _compare(kr.project(ps[:, :k_data], W[:, :k_data], np.float64), name, Nw, 'int', rows)
        # exchanged output rows, through W
        good = kr.project(ps, W, np.float64)
        swapped = good.copy()
        swapped[[0, rows - 1]] = swapped[[rows - 1, 0]]
        assert not _compare(swapped, name, Nw, 'int', rows)
        # real data: a relative error of 1e-12 in one entry (a thousandth of the old tolerance's reach) is outside the bound
        ref, bound = kc.w_reference(name, Nw, 'real')
        got = kr.project(kc.psi_of(name, 'real', False), kc.w_of(name, Nw, 'real'), np.float64)[:rows]
        assert _compare(got, name, Nw, 'real', rows)
        scale = (np.abs(kc.psi_of(name, 'real', True)[:rows]) @ np.abs(kc.w_of(name, Nw, 'real')).T).astype(np.float64)
        off = got.copy()
        off[rows - 1, Nw - 1] += 1e-12 * scale[rows - 1, Nw - 1]
        assert not _compare(off, name, Nw, 'real', rows)


@pytest.mark.parametrize('name', [n for n in kc.RECORD_CASES if kc.RECORD_CASES[n][2] > 0])
@pytest.mark.parametrize('kind', kc.KINDS)
def test_zeta_mutations_are_caught(name, kind):
    d = kc.record_dims(name)
    dl, ny, m = d['delays'], d['n_y'], d['m']
    sc = kc.scales(ny, m, kind, name)
    T = dl + 17
    y, u = kc.samples(T, ny, m, dl, kind, sc, name)
    E = kc.exps(d['nz'], d['degree'], d['dmd'])
    good = kr.psi(kr.zeta_record(y, u, dl, sc, np.float64), E, np.float64)
    # u_{t-j} read at j - 1: the input columns one sample too new
    ys, us = kr.scale_down(y, sc[0], sc[1], np.float64), kr.scale_down(u, sc[2], sc[3], np.float64)
    Zb = np.array([np.concatenate([ys[t]] + [ys[t - j] for j in range(1, dl + 1)] + [us[t - j + 1] for j in range(1, dl + 1)])
                   for t in range(dl, T)])
    assert not kr.same_bits(kr.psi(Zb, E, np.float64), good)
    # ring slot `head` off by one: the newest slot is taken for the one before it, and the walk back wraps into the newest
    for t in range(dl, T):
        pushed = [(y[k:k + 1], u[k:k + 1]) for k in range(t + 1)]
        right = kr.psi(kr.zeta_ring(pushed, dl, sc, np.float64), E, np.float64)
        assert kr.same_bits(right, good[t - dl:t - dl + 1])
        rotated = pushed[:-(dl + 1)] + [pushed[-1]] + pushed[-(dl + 1):-1]
        assert not kr.same_bits(kr.psi(kr.zeta_ring(rotated, dl, sc, np.float64), E, np.float64), right)
