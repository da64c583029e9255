"""GPU: srom_eigh_dev (csrc/eigh.hip) on every Jacobi path -- the one-workgroup LDS kernel, the scalar grid form (default and forced
above 256), the block form with pairs of 64 and of 128, and the block form's switches -- on the cases of tests/eigh_cases.py, checked
by tests/eigh_reference.py in long double.

Per case: return code 0; w ascending; eigenvalues against the exact integers (exact-spectrum and structured cases) or the
long-double Jacobi's (real spectra, tests/golden/eigh_reference_w.npz); defect = max |W^T W - I| and resid = max |G W - W diag(w)|;
for the exact cases every cluster's projector (a simple eigenvalue: the vector up to sign) against the exact one inside the
Davis-Kahan bound of the measured certificates and inside the fixed tolerance; diagonal inputs bit for bit (w the sorted diagonal,
W a permutation matrix).  The bounds are those of tests/test_edge_cases_gpu.py, relative to w_max = max |w_ref| (the zero matrix:
equality).  G and w sit between sentinel guards on the device."""
import ctypes as C

import numpy as np
import pytest

import eigh_cases as ec
import eigh_reference as er

pytestmark = pytest.mark.gpu

L = np.longdouble
GUARD = 64
SENTINEL = -7.25e300


class Guarded:
    """A device buffer of `count` doubles with GUARD sentinels on either side (tests/test_pod_build_exact_gpu.py), optionally
    filled with `data`."""

    def __init__(self, count, data=None):
        from sofacontrol_amd import _lib
        self.count = int(count)
        a = np.full(self.count + 2 * GUARD, SENTINEL)
        if data is not None:
            a[GUARD:-GUARD] = np.asarray(data, dtype=np.float64).ravel()
        self.buf = _lib.DeviceBuffer.from_array(a)
        self.ptr = C.c_void_p(self.buf.ptr.value + 8 * GUARD)

    def get(self, shape):
        """The payload, after checking that both guards are untouched."""
        a = self.buf.to_array((self.count + 2 * GUARD,))
        assert np.array_equal(a[:GUARD], np.full(GUARD, SENTINEL)) and np.array_equal(a[-GUARD:], np.full(GUARD, SENTINEL)), 'guard overwritten'
        return a[GUARD:-GUARD].reshape(shape).copy()


def _eigh(G, env, monkeypatch):
    """(w, W with the eigenvectors as columns) of srom_eigh_dev under exactly the switches of `env`."""
    from sofacontrol_amd import _lib
    for name in ec.ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    n = G.shape[0]
    dG, dw = Guarded(n * n, G), Guarded(n)
    rc = _lib.lib().srom_eigh_dev(dG.ptr, C.c_int64(n), dw.ptr, None)
    _lib.sync()
    assert rc == 0, (rc, _lib.lib().srh_last_error())
    w, V = dw.get((n,)), dG.get((n, n))
    assert np.isfinite(w).all() and np.isfinite(V).all()
    return w, V.T


def _reference_w(c):
    return np.sort(c['lam']).astype(L) if c['lam'] is not None else ec.reference_w(c['kind'], c['n'])


def _check(tag, c, w, W, bounds):
    """Print the measured figures, then assert every property of the module docstring."""
    G, n, kind = c['G'], c['n'], c['kind']
    w_ref = _reference_w(c)
    w_max = float(np.abs(w_ref).max())
    defect, resid, asc = er.certificates(G, w, W)
    err = float(np.abs(w.astype(L) - w_ref).max())
    rel = lambda x: x / w_max if w_max > 0 else x
    sub, worst = [], (0.0, 0.0)
    if c['Qs'] is not None and kind not in ec.DIAGONAL_KINDS:
        tol = ec.PROJ_TOL['block' if bounds is ec.BLOCK else 'tight']
        for f, m, gap, e in er.subspace_errors(W, c['lam'], c['Qs'], c['s']):
            bound = min(tol, er.subspace_bound(n, m, gap, defect, resid, w_max) + n * 2.0 ** -60)
            sub.append((f, m, gap, e, bound))
            if e / bound >= worst[0]:
                worst = (e / bound, e)
    zeros = int((w == 0.0).sum())
    print('%-34s eig %.2e (%.1e of bound)  defect %.2e (%.1e)  resid %.2e (%.1e)  subspace %.2e (%.1e of its bound)  exact zeros %d' %
          (tag, rel(err), rel(err) / bounds['eig'], defect, defect / bounds['defect'], rel(resid), rel(resid) / bounds['resid'],
           worst[1], worst[0], zeros))
    assert asc, 'w is not ascending'
    assert err <= bounds['eig'] * w_max
    assert defect <= bounds['defect']
    assert resid <= bounds['resid'] * w_max
    for f, m, gap, e, bound in sub:
        assert e <= bound, ('cluster at %d of multiplicity %d, gap %g' % (f, m, gap), e, bound)
    if kind in ec.DIAGONAL_KINDS:
        # a diagonal input is never rotated: the sorted diagonal, a permutation matrix, G W = W diag(w) -- all bit for bit
        assert np.array_equal(w, np.sort(c['lam']).astype(np.float64))
        assert er.is_permutation(W)
        assert np.array_equal(G @ W, W * w)
    if c['zero_rows'] and kind not in ec.DIAGONAL_KINDS:
        # an exactly zero row of G is never rotated either: its unit vector comes back exactly, with an exactly zero eigenvalue.
        # The rest of the null space comes out at rounding noise -- except that the pair of identical snapshots, rotated by exactly
        # 45 degrees should the ordering take it first, can leave one more exact zero.
        rows = np.flatnonzero(~G.any(axis=1))
        units = [j for j in range(n) if np.count_nonzero(W[:, j]) == 1 and abs(W[:, j]).max() == 1.0 and np.flatnonzero(W[:, j])[0] in rows]
        assert len(units) == len(rows) == c['zero_rows'] and all(w[j] == 0.0 for j in units)
        assert c['zero_rows'] <= zeros <= c['zero_rows'] + 1


def _tag(path, n, kind):
    return '%s n=%d %s' % (path, n, kind)


@pytest.mark.parametrize('path,n,kind', ec.device_cases(), ids=lambda v: str(v))
def test_eigh_path_case(path, n, kind, monkeypatch):
    solver, env, bounds, _ = ec.PATHS[path]
    c = ec.case(kind, n)
    w, W = _eigh(c['G'], env, monkeypatch)
    _check(_tag(path, n, kind), c, w, W, bounds)
    if c['base'] is not None:
        # an exact scaling: reported, not asserted (the thresholds 1e-300 and the squares of the norm test are not scale-free)
        wb, Wb = _eigh(ec.case(c['base'][0], n)['G'], env, monkeypatch)
        print('%-34s w / 2^(+-100) bit-identical to the unscaled run: %s, W: %s' %
              ('', np.array_equal(w / c['base'][1], wb), np.array_equal(W, Wb)))


@pytest.mark.parametrize('name,env', ec.SWITCHES, ids=[s[0] for s in ec.SWITCHES])
def test_eigh_block_switches(name, env, monkeypatch):
    """SRH_EIGH_BLOCK_ORDER 0 and 1 (1 has its own permutation loop) and SRH_EIGH_BLOCK_INNER 2, pairs of 64, on the indefinite
    spectrum at n = 193: 63 padding positions with eigenvalue 0 beside a zero eigenvalue of multiplicity 15."""
    c = ec.case(ec.SWITCH_KIND, ec.SWITCH_N)
    w, W = _eigh(c['G'], env, monkeypatch)
    _check(_tag('block64 ' + name, ec.SWITCH_N, ec.SWITCH_KIND), c, w, W, ec.BLOCK)


@pytest.mark.parametrize('path,n,kind', ec.REPEAT, ids=lambda v: str(v))
def test_eigh_repeat_calls_are_bit_identical(path, n, kind, monkeypatch):
    """The method is deterministic (fixed pairing, fixed-order reductions): two calls on the same input agree bit for bit."""
    env = ec.PATHS[path][1]
    G = ec.case(kind, n)['G']
    w1, W1 = _eigh(G, env, monkeypatch)
    w2, W2 = _eigh(G, env, monkeypatch)
    print('%-34s repeat call: w identical %s, W identical %s' % (_tag(path, n, kind), np.array_equal(w1, w2), np.array_equal(W1, W2)))
    assert np.array_equal(w1, w2) and np.array_equal(W1, W2)
