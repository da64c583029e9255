"""CPU: the cases of tests/eigh_cases.py and the references of tests/eigh_reference.py, without a GPU -- the integer construction is
exact and has the claimed spectrum, the exact eigenpairs, the long-double Jacobi and numpy's double-precision eigh all meet the
bounds that tests/test_eigh_exact_gpu.py asserts of the kernels (so the bounds are conditions on the kernel, not on the case), every
cluster's gap carries the asserted projector tolerance, and the size table covers each solver's padded and unpadded size."""
import numpy as np
import pytest

import eigh_cases as ec
import eigh_reference as er

L = np.longdouble
MARGIN = 100.0                        # the references meet every bound with this factor to spare

KEYS = ec.matrix_keys()
EXACT_KEYS = [(k, n) for k, n in KEYS if k in ec.EXACT_KINDS]
_id = lambda kn: '%s-%d' % kn


def _bounds_of(kind, n):
    """The bound sets of the paths that run (kind, n)."""
    out = [ec.PATHS[path][2] for path, m, k in ec.device_cases() if (k, m) == (kind, n)]
    if (kind, n) == (ec.SWITCH_KIND, ec.SWITCH_N):
        out.append(ec.BLOCK)
    return out


def _exact_pairs(c):
    """(w ascending, W) in long double from the exact spectrum and Qs / s."""
    order = np.argsort(c['lam'], kind='stable')
    return c['lam'][order].astype(L), np.asarray(c['Qs'], dtype=L)[:, order] / L(c['s'])


def _assert_within(G, w, W, w_ref, frac, what):
    """Eigenvalue error, defect and residual inside frac times the TIGHT bounds (the stricter set)."""
    w_max = float(np.abs(w_ref).max())
    defect, resid, asc = er.certificates(G, w, W)
    err = float(np.abs(np.asarray(w, dtype=L) - w_ref).max())
    assert asc, what
    assert err <= frac * ec.TIGHT['eig'] * w_max, (what, err, w_max)
    assert defect <= frac * ec.TIGHT['defect'], (what, defect)
    assert resid <= frac * ec.TIGHT['resid'] * w_max, (what, resid, w_max)


# --------------------------------------------------------------------------------------------------------- construction
@pytest.mark.parametrize('n', sorted({n for _, n in KEYS}))
def test_householder_vector(n):
    v, s = ec.householder_vector(n)
    assert v.shape == (n,) and np.all(v >= 1) and int((v * v).sum()) == s
    if n != 3:
        assert s & (s - 1) == 0 and s < 16 * n, 'every size of the table but 3 has a power of two'
    else:
        assert s == 3


@pytest.mark.parametrize('key', EXACT_KEYS, ids=_id)
def test_integer_construction_is_exact(key):
    kind, n = key
    c = ec.case(kind, n)
    N, Qs, s, den, G = c['N'], c['Qs'], c['s'], c['den'], c['G']
    assert N.dtype == np.int64 and np.abs(N).max() < 2 ** 53 and np.array_equal(N, N.T)
    assert den & (den - 1) == 0                                           # 1 or s^2 with s a power of two: the division is exact
    assert np.array_equal(G * float(den), N.astype(np.float64)) and np.array_equal((G * float(den)).astype(np.int64), N)
    assert np.array_equal(G, G.T)
    # the spectrum: N Qs = Qs diag(den lam) and Qs Qs^T = s^2 I, exactly in int64 (entries below 2^53 * 2^10)
    assert np.array_equal(N @ Qs, Qs * (den * c['lam']))
    assert np.array_equal(Qs @ Qs.T, s * s * np.eye(n, dtype=np.int64))
    assert np.array_equal(np.sort(c['lam']), np.sort(ec.spectrum(kind, n) * (1 if s & (s - 1) == 0 else s * s)))
    if kind != 'scalar' and n >= 63:
        assert np.count_nonzero(G) >= 0.99 * n * n, 'dense (a few entries cancel where v is all ones)'
    elif kind == 'scalar':
        assert np.array_equal(G, np.diag(np.diag(G)))


def test_spectra_have_the_stated_shape():
    for n in (63, 127, 193, 256, 300):
        mult = lambda D: sorted(np.unique(D, return_counts=True)[1].tolist())
        assert mult(ec.spectrum('distinct', n)) == [1] * n
        m = mult(ec.spectrum('clusters', n))
        assert m[-3:] == [2, 3, n // 3] and set(m[:-3]) == {1}
        D = ec.spectrum('indefinite', n)
        assert (D == 0).sum() >= 3 and (D < 0).sum() >= 3 and (D > 0).sum() >= 3
        for kind, r in (('rank3', 3), ('rank10', max(4, n // 10))):
            D = ec.spectrum(kind, n)
            assert (D == 0).sum() == n - r and (D > 0).sum() == r and len(np.unique(D)) == r + 1
    for n in (127, 256):
        d = ec.diagonal_values(n)
        assert len(np.unique(d)) < n and np.any(np.diff(d) < 0) and (d < 0).any() and (d == 0).any() and (d > 0).any()
        S = ec.gramian_snapshots(n)
        G = ec.case('gramian', n)['G']
        assert not S[1].any() and np.array_equal(S[2], S[n - 1]) and S[2].any()
        assert not G[1].any() and not G[:, 1].any() and np.array_equal(G[2], G[n - 1]) and np.abs(G).max() < 2 ** 53
        assert np.linalg.matrix_rank(S.astype(np.float64)) <= max(2, n // 4) < n - 3
        g = ec.case('graded', n)['G']
        assert np.array_equal(g, g.T) and np.array_equal(ec.case('graded_up', n)['G'] / ec.UP, g)
        assert np.array_equal(ec.case('graded_down', n)['G'] / ec.DOWN, g)
        w = np.linalg.eigvalsh(g)
        assert w[0] > 0 and w[-1] / w[0] > 1e5, 'graded over at least five decades'


# ------------------------------------------------------------------------------------------------ the references, bounds
@pytest.mark.parametrize('key', [(k, n) for k, n in KEYS if ec.case(k, n)['Qs'] is not None], ids=_id)
def test_exact_eigenpairs_meet_every_bound(key):
    """The exact pairs (lam, Qs / s) rounded to long double: the reference of the exact-spectrum and diagonal cases."""
    c = ec.case(*key)
    w, W = _exact_pairs(c)
    _assert_within(c['G'], w, W, w, 1.0 / MARGIN, key)
    for f, m, gap, err in er.subspace_errors(W, c['lam'], c['Qs'], c['s']):
        assert err == 0.0


@pytest.mark.parametrize('key', ec.real_keys(), ids=_id)
def test_jacobi_reference_meets_every_bound_and_matches_the_golden_file(key):
    """The real spectra: the row-cyclic long-double Jacobi, recomputed; its eigenvalues are those of tests/golden (to 1e-17 w_max,
    five decades below the tightest bound) and its pairs meet the bounds with the margin, on the case and on its two scalings."""
    kind, n = key
    G = ec.case(kind, n)['G']
    w, W, sweeps = er.jacobi(G)
    w_max = float(np.abs(w).max())
    gold = ec.reference_w(kind, n)
    print('%s n %d: %d sweeps, golden differs by %.1e w_max' % (kind, n, sweeps, float(np.abs(w - gold).max()) / w_max))
    assert float(np.abs(w - gold).max()) <= 1e-17 * w_max
    _assert_within(G, w, W, gold, 1.0 / MARGIN, key)
    if kind == 'graded':
        for scaled in ('graded_up', 'graded_down'):
            cs = ec.case(scaled, n)
            ws = ec.reference_w(scaled, n)
            assert np.array_equal(ws, gold * L(cs['base'][1]))
            _assert_within(cs['G'], w * L(cs['base'][1]), W, ws, 1.0 / MARGIN, (scaled, n))


@pytest.mark.parametrize('kind,n', [(k, n) for n in (3, 64, 65) for k in ec.EXACT_KINDS + ('diagonal', 'zero', 'identity')
                                    if not (n == 3 and k in ('rank3', 'rank10'))])
def test_jacobi_reference_against_exact_spectra(kind, n):
    """The reference method itself on cases whose answer is known: eigenvalues, certificates and every cluster's subspace."""
    c = ec.case(kind, n)
    w, W, sweeps = er.jacobi(c['G'])
    wx, _ = _exact_pairs(c)
    _assert_within(c['G'], w, W, wx, 1.0 / MARGIN, (kind, n))
    w_max = float(np.abs(wx).max())
    defect, resid, _ = er.certificates(c['G'], w, W)
    for f, m, gap, err in er.subspace_errors(W, c['lam'], c['Qs'], c['s']):
        assert err <= er.subspace_bound(n, m, gap, defect, resid, w_max) + n * 2.0 ** -60, (f, m, gap, err)


@pytest.mark.parametrize('key', KEYS, ids=_id)
def test_numpy_double_meets_every_bound(key):
    """numpy.linalg.eigh in double precision passes what the kernels are asked to pass (the tight set, on every case)."""
    kind, n = key
    c = ec.case(kind, n)
    w, W = np.linalg.eigh(c['G'])
    w_ref = np.sort(c['lam']).astype(L) if c['lam'] is not None else ec.reference_w(kind, n)
    _assert_within(c['G'], w, W, w_ref, 1.0, key)


@pytest.mark.parametrize('key', [(k, n) for k, n in KEYS if ec.case(k, n)['Qs'] is not None], ids=_id)
def test_cluster_gaps_carry_the_projector_tolerance(key):
    """At the largest residual and defect the bounds permit, residual over gap stays below the asserted projector tolerance."""
    kind, n = key
    c = ec.case(kind, n)
    w_max = float(np.abs(c['lam']).max())
    for b in _bounds_of(kind, n):
        tol = ec.PROJ_TOL['block' if b is ec.BLOCK else 'tight']
        for f, m, gap, in er.clusters(np.sort(c['lam'])):
            assert er.subspace_bound(n, m, gap, b['defect'], b['resid'] * w_max, w_max) <= tol, (key, m, gap)


# ----------------------------------------------------------------------------------------------------------- size table
def test_size_table_covers_each_solvers_padding():
    sizes = lambda name: set(ec.PATHS[name][3])
    full = lambda name: {n for n, kinds in ec.PATHS[name][3].items() if kinds == ec.FULL}
    # csrc/eigh.hip: ne = (n + 1) & ~1 for the LDS and grid kernels, ne = ceil(n / P) P, nb = ne / (P / 2), nb / 2 pairs for the block form
    assert ec.ne_block(129, 128) == (256, 4, 2) and ec.ne_block(129, 64) == (192, 6, 3)
    assert ec.ne_block(257, 128) == (384, 6, 3) and ec.ne_block(193, 64) == (256, 8, 4) and ec.ne_block(256, 128) == (256, 4, 2)
    for name, P in (('lds', 0), ('grid', 0), ('block64', 64), ('block128', 128)):
        ne = (lambda n: ec.ne_block(n, P)[0]) if P else ec.ne_scalar
        assert any(ne(n) > n for n in full(name)) and any(ne(n) == n for n in full(name)), name
        for n in full(name):
            assert all((name, n, kind) in ec.device_cases() for kind in ec.FULL)
    # the boundaries of the dispatch: the paths without a switch get the solver they are named for
    for name in ('lds', 'grid', 'block64_default'):
        assert ec.PATHS[name][1] == {} and all(ec.default_solver(n) == ec.PATHS[name][0] for n in sizes(name)), name
    assert {128} <= sizes('lds') and {129, 256} <= sizes('grid') and {257} <= sizes('block64_default')
    assert sizes('lds') == {1, 2, 3, 63, 64, 65, 127, 128} and sizes('grid') == {129, 255, 256} and sizes('grid_forced') == {257, 300}
    assert sizes('block64') == {129, 191, 192, 193} and sizes('block128') == {129, 255, 256, 257}
    assert max(n for _, n in KEYS) <= 400
    for path, n, kind in ec.device_cases():
        assert set(ec.EDGE) <= set(ec.PATHS[path][3][n])
    assert ec.KNOWN == ec.FULL[:9] and all(ec.PATHS['grid_forced'][3][n] == ec.KNOWN for n in (257, 300))
    assert ec.ne_scalar(257) == 258 and ec.ne_scalar(300) == 300
    assert {name for name, _ in ec.SWITCHES} == {'order0', 'order1', 'inner2'}
    for path, n, kind in ec.REPEAT:
        assert (path, n, kind) in ec.device_cases()
    assert {ec.PATHS[p][0] for p, _, _ in ec.REPEAT} == {'lds', 'grid', 'block64', 'block128'}


# ------------------------------------------------------------------------------------------------- the checks have teeth
def test_checks_reject_small_errors_and_accept_a_rotation_inside_a_cluster():
    c = ec.case('clusters', 64)
    w, W = _exact_pairs(c)
    n, w_max = 64, float(np.abs(w).max())
    cl = er.clusters(np.sort(c['lam']))
    big = max(cl, key=lambda fmg: fmg[1])                                      # the cluster of multiplicity n / 3
    lone = next(f for f, m, _ in cl if m == 1)
    worst = lambda V: max(e for _, _, _, e in er.subspace_errors(V, c['lam'], c['Qs'], c['s']))

    def rotated(i, j, angle):
        V, angle = W.copy(), L(angle)
        V[:, i], V[:, j] = np.cos(angle) * W[:, i] - np.sin(angle) * W[:, j], np.sin(angle) * W[:, i] + np.cos(angle) * W[:, j]
        return V
    # any orthonormal basis of a cluster is an answer: certificates and projectors do not move
    V = rotated(big[0], big[0] + 1, 0.5)
    defect, resid, _ = er.certificates(c['G'], w, V)
    assert defect <= 1e-17 and resid <= 1e-17 * w_max and worst(V) <= 1e-17
    # a rotation by 1e-5 between a cluster and a simple eigenvector: orthonormal still, but residual and subspace both show it
    V = rotated(big[0], lone, 1e-5)
    defect, resid, _ = er.certificates(c['G'], w, V)
    assert defect <= 1e-17 and resid > ec.BLOCK['resid'] * w_max and worst(V) > ec.PROJ_TOL['block'] / 10
    # an eigenvalue off by 2e-11 w_max: the eigenvalue bounds of both sets and the residual bound of the tight set
    w2 = w.copy()
    w2[lone] += L(2e-11) * w_max
    assert float(np.abs(w2 - w).max()) > ec.BLOCK['eig'] * w_max and er.certificates(c['G'], w2, W)[1] > ec.TIGHT['resid'] * w_max
    # a column scaled by 1 + 1e-10: the defect
    V = W.copy()
    V[:, 3] *= 1 + L(1e-10)
    assert er.certificates(c['G'], w, V)[0] > ec.BLOCK['defect']
    # two eigenpairs exchanged: w is no longer ascending
    order = np.arange(n)
    order[[lone, big[0]]] = order[[big[0], lone]]
    assert not er.certificates(c['G'], w[order], W[:, order])[2]
