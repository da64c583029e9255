"""GPU: the TPWL table kernels (csrc/tpwl.hip, csrc/tpwl_dev.h) against the long-double statement of tests/tpwl_table_reference.py on the
cases of tests/tpwl_table_cases.py: exact ties that no rounding can break, minima on lane / round / thread-stride boundaries, non-finite
states, every search path (tpwl::nearest_wave, the register table of tpwl::nearest_many, the HELD search of the staged rollout,
weights_kernel).  tests/test_tpwl_table_reference_cpu.py shows without a GPU that every finite query is decided (float64 rounding
cannot move its minimum), so the indices are compared for equality.

The handles are made through the C ABI from the cases' own tables.  Non-finite states go ONLY through the entry points that just write an
index (stpwl_nearest, stpwl_nearest_many); every other consumer calls the same function."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import tpwl as otpwl
import tpwl_table_cases as tc
import tpwl_table_reference as tr

pytestmark = pytest.mark.gpu


class Handle:
    """stpwl handle over a model dict (with 'A_d', 'B_d', 'd_d'); plain=True: created under SRH_TPWL_ROLLOUT_PLAIN=1."""

    def __init__(self, model, H=None, z_ref=None, plain=False):
        from sofacontrol_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.P, self.r = model['q'].shape
        self.n, self.m, self.nz = 2 * self.r, model['u'].shape[1], 0
        self.h = C.c_void_p()
        tabs = [_lib.f64(model[k]) for k in ('q', 'v', 'u', 'A_c', 'B_c', 'd_c', 'A_d', 'B_d', 'd_d')]
        old = os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
        try:
            if plain:
                os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = '1'
            _lib.check(self.L.stpwl_create(C.byref(self.h), C.c_int(self.P), C.c_int(self.r), C.c_int(self.m), *[_lib.dptr(t) for t in tabs],
                                           C.c_double(model['w_q']), C.c_double(model['w_v'])), 'stpwl_create')
        finally:
            os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
            if old is not None:
                os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = old
        if H is not None:
            self.nz = H.shape[0]
            _lib.check(self.L.stpwl_set_output(self.h, _lib.dptr(_lib.f64(H)), _lib.dptr(_lib.f64(z_ref)), C.c_int(self.nz)), 'stpwl_set_output')

    def nearest(self, X):
        X = self._lib.f64(X)
        idx = np.full(len(X), -7, dtype=np.int32)
        self._lib.check(self.L.stpwl_nearest(self.h, self._lib.dptr(X), C.c_int64(len(X)), self._lib.iptr(idx)), 'stpwl_nearest')
        return idx

    def nearest_many(self, X, threads):
        X = self._lib.f64(X)
        idx = np.full(len(X), -7, dtype=np.int32)
        self._lib.check(self.L.stpwl_nearest_many(self.h, self._lib.dptr(X), C.c_int(len(X)), C.c_int(threads), self._lib.iptr(idx)),
                        'stpwl_nearest_many')
        return idx

    def linearize(self, X, discrete):
        X = self._lib.f64(X)
        B, n, m = len(X), self.n, self.m
        A, Bm, d = np.full((B, n, n), np.nan), np.full((B, n, m), np.nan), np.full((B, n), np.nan)
        idx = np.full(B, -7, dtype=np.int32)
        self._lib.check(self.L.stpwl_linearize(self.h, self._lib.dptr(X), C.c_int64(B), C.c_int(discrete), self._lib.dptr(A),
                                               self._lib.dptr(Bm), self._lib.dptr(d), self._lib.iptr(idx)), 'stpwl_linearize')
        return A, Bm, d, idx

    def weights(self, X, beta):
        X = self._lib.f64(X)
        W = np.full((len(X), self.P), -7.0)
        self._lib.check(self.L.stpwl_weights(self.h, self._lib.dptr(X), C.c_int64(len(X)), C.c_double(beta), self._lib.dptr(W)), 'stpwl_weights')
        return W

    def linearize_weighted(self, X, beta):
        X = self._lib.f64(X)
        B, n, m = len(X), self.n, self.m
        A, Bm, d, W = np.full((B, n, n), np.nan), np.full((B, n, m), np.nan), np.full((B, n), np.nan), np.full((B, self.P), np.nan)
        self._lib.check(self.L.stpwl_linearize_weighted(self.h, self._lib.dptr(X), C.c_int64(B), C.c_double(beta), self._lib.dptr(A),
                                                        self._lib.dptr(Bm), self._lib.dptr(d), self._lib.dptr(W)), 'stpwl_linearize_weighted')
        return A, Bm, d, W

    def plan(self, N, batch):
        return self._lib.tpwl_rollout_plan(self.h, N, batch)

    def rollout(self, x0, u):
        _lib = self._lib
        x0, u = _lib.f64(x0), _lib.f64(u)
        Bn, N = u.shape[0], u.shape[1]
        X = np.full((Bn, N + 1, self.n), np.nan)
        Z = np.full((Bn, N + 1, self.nz), np.nan) if self.nz else None
        _lib.check(self.L.stpwl_rollout(self.h, _lib.dptr(x0), _lib.dptr(u), C.c_int(N), C.c_int64(Bn), _lib.dptr(X),
                                        _lib.dptr(Z) if self.nz else None), 'stpwl_rollout')
        return X, Z

    def characteristic(self):
        xc, fc = np.full(self.n, np.nan), np.full(self.n, np.nan)
        self._lib.check(self.L.stpwl_characteristic(self.h, self._lib.dptr(xc), self._lib.dptr(fc)), 'stpwl_characteristic')
        return xc, fc

    def __del__(self):
        try:
            self.L.stpwl_destroy(self.h)
        except Exception:
            pass


def handle(s, kind):
    return Handle(tc.table(s, kind))


def windows(Q, B):
    """Index windows of length B that together cover range(Q) (the last one wraps; B > Q: one window, tiled)."""
    if B >= Q:
        return [np.resize(np.arange(Q), B)]
    return [np.arange(a, a + B) % Q for a in range(0, Q, B)]


def mismatch(got, ref, fam, sel=None):
    bad = np.flatnonzero(got != ref)
    return [(int(k if sel is None else sel[k]), str(fam[k if sel is None else sel[k]]), int(got[k]), int(ref[k])) for k in bad[:8]]


# ---------------------------------------------------------------------------------------- stpwl_nearest (tpwl::nearest_wave)
@pytest.mark.parametrize('s', tc.SPECS, ids=tc.spec_id)
def test_nearest_equals_the_reference_at_every_batch_size(s):
    """Every family at B in {1, 3, 4, 5, 257} (nearest_kernel: four states per workgroup, whole waves retire at B % 4 != 0).  A state that
    is not a number gives 0 and leaves the states beside it in the batch alone: every index of every batch equals the reference."""
    for kind in tc.kinds(s):
        X, want, fam = tc.queries(s, kind)
        ref = tc.reference(s, kind)[0]
        h = handle(s, kind)
        for B in (1, 3, 4, 5, 257):
            for sel in windows(len(X), B):
                got = h.nearest(X[sel])
                assert np.array_equal(got, ref[sel]), (kind, B, mismatch(got, ref[sel], fam, sel))
        bad = ~tc.finite(X)
        if bad.any():
            assert (h.nearest(X)[bad] == want[bad]).all() and (want[bad & (fam != 'nan-v')] == 0).all()


# ---------------------------------------------------------------------------------------- stpwl_linearize (nearest_wave + gather)
LIN_SPECS = [s for s in tc.SPECS if s[:2] in ((2, 2), (64, 32), (65, 17), (129, 5), (300, 5), (7, 48))]


@pytest.mark.parametrize('discrete', [0, 1], ids=['continuous', 'discrete'])
@pytest.mark.parametrize('s', LIN_SPECS, ids=tc.spec_id)
def test_linearize_gathers_the_tables_of_the_first_minimum(s, discrete):
    """The tie and boundary families (finite states only): idx equals the reference and A/B/d are the tables of that index -- the two
    points of a tie have different tables."""
    names = ('A_d', 'B_d', 'd_d') if discrete else ('A_c', 'B_c', 'd_c')
    for kind in tc.kinds(s):
        X, want, fam = tc.queries(s, kind)
        keep = tc.finite(X) & (fam != 'random')
        if not keep.any():
            continue
        m = tc.table(s, kind)
        ref = tc.reference(s, kind)[0][keep]
        A, B, d, idx = handle(s, kind).linearize(X[keep], discrete)
        assert np.array_equal(idx, ref), (kind, mismatch(idx, ref, fam[keep]))
        for got, name in zip((A, B, d), names):
            assert np.array_equal(got, m[name][ref]), (kind, name)


# ---------------------------------------------------------------------------------------- tpwl::nearest_many
MANY_SPECS = [s for s in tc.SPECS if s[:2] in ((64, 32), (63, 15), (65, 17), (64, 33))]          # w_v = 0: inside / outside the register branch


@pytest.mark.parametrize('threads', [256, 512])
@pytest.mark.parametrize('s', MANY_SPECS, ids=tc.spec_id)
def test_nearest_many_equals_the_reference_across_the_switch(s, threads):
    """One workgroup over count states, as the GuSTO kernels call it.  The register table takes over at count = 2 waves (w_v = 0,
    P <= 64, r <= 32); below, and for every other model, the wave search: same indices on both sides of the switch, equal to the
    reference and to stpwl_nearest.  51 states: 6 or 3 full rounds and a last one that the prefetch clamps."""
    waves = threads // 64
    for kind in tc.kinds(s):
        X, want, fam = tc.queries(s, kind)
        ref = tc.reference(s, kind)[0]
        sel = np.resize(np.arange(len(X)), 51)
        if len(X) > 51:                                                  # keep every family: the non-random ones first
            order = np.argsort(fam == 'random', kind='stable')
            sel = order[:51]
        h = handle(s, kind)
        wave_idx = h.nearest(X[sel])
        assert np.array_equal(wave_idx, ref[sel]), (kind, mismatch(wave_idx, ref[sel], fam, sel))
        got = {}
        for count in (1, 2 * waves - 1, 2 * waves, 2 * waves + 1, 51):
            got[count] = h.nearest_many(X[sel[:count]], threads)
            assert np.array_equal(got[count], ref[sel[:count]]), (kind, count, mismatch(got[count], ref[sel[:count]], fam, sel))
            assert np.array_equal(got[count], wave_idx[:count])
        assert np.array_equal(got[2 * waves][:2 * waves - 1], got[2 * waves - 1])
        assert np.array_equal(got[2 * waves + 1][:2 * waves], got[2 * waves]) and np.array_equal(got[51][:2 * waves], got[2 * waves])


# ---------------------------------------------------------------------------------------- rollouts that land on ties
@pytest.mark.parametrize('r,P,w_v,path', [(5, 9, 0.0, (True, True)), (33, 9, 0.0, (True, False)), (5, 70, 0.0, (True, False)),
                                          (5, 9, 0.5, (True, False))], ids=['held', 'wave-r33', 'wave-P70', 'wave-w_v'])
def test_rollouts_on_ties_take_the_first_point(r, P, w_v, path):
    """x_{k+1} = d_d[i_k] exactly (A_d = B_d = 0), on a duplicated point or on the midpoint of a mirror pair at every stage, and the two
    candidates send the state to different places: the staged kernel of the shape (HELD search or nearest_wave) and the plain kernel give
    the reference's trajectory and outputs, bit for bit."""
    model, Ad, Bd, dd, H, z_ref, x0, u, want = tc.tie_rollout(r, P, w_v)
    model = dict(model, A_d=Ad, B_d=Bd, d_d=dd)
    refs = [tr.rollout(model, Ad, Bd, dd, x0[b], u[b]) for b in range(2)]
    assert refs[0][1].tolist() == want.tolist()
    Xr = np.stack([x.astype(float) for x, _ in refs])
    Zr = np.stack([(tr.ld(H) @ x.T).T + tr.ld(z_ref) for x, _ in refs]).astype(float)
    staged, plain = Handle(model, H, z_ref), Handle(model, H, z_ref, plain=True)
    N = u.shape[1]
    ps = staged.plan(N, 2)
    assert (ps['staged'], ps['held']) == path and not plain.plan(N, 2)['staged']
    Xs, Zs = staged.rollout(x0, u)
    Xp, Zp = plain.rollout(x0, u)
    assert np.array_equal(Xs, Xr), [np.flatnonzero((Xs[b] != Xr[b]).any(axis=1)).tolist() for b in range(2)]
    assert np.array_equal(Xp, Xr), [np.flatnonzero((Xp[b] != Xr[b]).any(axis=1)).tolist() for b in range(2)]
    assert np.array_equal(Zs, Zr) and np.array_equal(Zp, Zr)
    # and the index-only entry on the states of the trajectory
    for b in range(2):
        assert np.array_equal(staged.nearest(Xr[b][:N]), refs[b][1])


def test_plain_rollout_computes_every_column_above_256():
    """n_x = 258 (r = 129, P = 3, m = 2, N = 3, batch 2): the layout is far above 64 KB, the plain kernel runs, and its products have more
    columns than the workgroup has threads.  Every column of every state within 1e-10 of the largest value (the tolerance of
    tests/test_tpwl_gpu.py) of oracle.tpwl.rollout."""
    r, m, P, N, batch = 129, 2, 3, 3, 2
    model = otpwl.synthetic_model(r, m, P, seed=r + m)
    model['q'] *= 0.1
    Ad, Bd, dd = otpwl.pre_discretize(model, 0.05, 'zoh')
    rng = np.random.default_rng(3)
    x0 = 0.01 * rng.standard_normal((batch, 2 * r))
    u = rng.uniform(1.0, 800.0, (batch, N, m))
    Xo = np.stack([otpwl.rollout(model, Ad, Bd, dd, x0[b], u[b]) for b in range(batch)])
    assert np.isfinite(Xo).all()
    H = otpwl.synthetic_output_matrix(r, seed=4)
    z_ref = rng.uniform(-100.0, 100.0, 6)
    h = Handle(dict(model, A_d=Ad, B_d=Bd, d_d=dd), H, z_ref)
    assert not h.plan(N, batch)['staged']
    X, Z = h.rollout(x0, u)
    tol = 1e-10 * max(1.0, float(np.abs(Xo).max()))
    err = np.abs(X - Xo).max(axis=(0, 1))                                # per column; NaN where a column was never written
    print('largest error in the columns < 256: %.3e, >= 256: %.3e (tolerance %.3e)' % (err[:256].max(), err[256:].max(), tol))
    assert np.isfinite(X).all() and (err <= tol).all(), np.flatnonzero(~(err <= tol)).tolist()
    Zo = np.einsum('aj,bkj->bka', H, Xo) + z_ref
    np.testing.assert_allclose(Z, Zo, rtol=0, atol=1e-10 * max(1.0, float(np.abs(Zo).max())))


# ---------------------------------------------------------------------------------------- stpwl_characteristic
@pytest.mark.parametrize('s', [(65, 17, 1.0, 0.0), (129, 5, 1.0, 0.5), (300, 5, 1.0, 0.0)], ids=tc.spec_id)
def test_characteristic_values_with_duplicated_points(s):
    """char_kernel evaluates f at every stored point with the tables of ITS nearest point: for both points of a duplicated pair that is
    the first one's (1e-12 of the largest value, as tests/test_tpwl_gpu.py::test_golden_g3).  The SECOND point's d_c carries 1e6 in
    columns of its own, far above every other |f| (~5e3): f_char shows it if either point of the pair is evaluated with the second one's tables."""
    for kind in [k for k in tc.kinds(s) if k.startswith('dup')]:
        pairs = tc.pair_groups(s[0])[int(kind[3:])]
        m = dict(tc.table(s, kind))
        m['d_c'] = m['d_c'].copy()
        for k, (a, b) in enumerate(pairs):
            m['d_c'][b, k::len(pairs)] += 1e6
        S = tc.points(m)
        j = tr.nearest(m, S)
        for a, b in pairs:
            assert j[a] == a and j[b] == a

        def f_char(pick):
            f = np.stack([tr.ld(m['A_c'][pick[i]]) @ tr.ld(S[i]) + tr.ld(m['B_c'][pick[i]]) @ tr.ld(m['u'][i]) + tr.ld(m['d_c'][pick[i]])
                          for i in range(len(S))])
            return np.abs(f).max(axis=0).astype(float)
        f_ref, x_ref = f_char(j), np.abs(S).max(axis=0)
        assert f_ref.max() < 1e5 and (f_char(np.arange(len(S))) > 5e5).any()          # each point with its own tables: visibly different
        xc, fc = Handle(m).characteristic()
        assert np.array_equal(xc, x_ref)
        np.testing.assert_allclose(fc, f_ref, rtol=0, atol=1e-12 * max(1.0, float(f_ref.max())))


# ---------------------------------------------------------------------------------------- stpwl_weights
@pytest.mark.parametrize('s', tc.SPECS, ids=tc.spec_id)
def test_weights_within_the_bound_of_the_reference(s):
    """Per component |w_i - ref_i| <= tc.weight_bound (16 eps (1 + beta d_i / d_min) ref_i + P eps ref_i over the float64 floor), for
    beta in {0, 3, 50}; P = 257, 300: the thread stride wraps.  On a duplicated point: one-hot at the first duplicate, exactly.  1e-9
    next to a point: most weights underflow to 0, the sum stays 1, nothing is NaN.  Every row equals its single-query result."""
    P, r, w_q, w_v = s
    worst = 0.0
    for kind, (X, fam) in tc.weight_queries(s).items():
        m, h = tc.table(s, kind), handle(s, kind)
        for beta in tc.BETAS:
            W = h.weights(X, beta)
            assert np.isfinite(W).all()
            for k, (x, f) in enumerate(zip(X, fam)):
                D = tr.distances(m, x)
                Wr = tr.weights(m, x, beta)
                err, bound = np.abs(W[k] - Wr), tc.weight_bound(Wr, D, beta, P)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (kind, beta, f, k, float((err / bound).max()))
                assert abs(W[k].sum() - 1.0) <= (P + 16) * tr.EPS
                if f == 'dup-on':
                    assert np.array_equal(W[k], Wr.astype(float)) and W[k][tr.first_min(D)] == 1.0 and W[k].sum() == 1.0
                if beta == 0 and D.min() > 0:
                    assert np.array_equal(W[k], np.full(P, 1.0 / P))
                if f == 'near' and beta > 0 and P > 1 and (w_q or w_v):
                    assert (W[k] == 0).sum() >= P // 2 and W[k].max() > 0.99
            for k in (0, len(X) - 1):
                assert np.array_equal(h.weights(X[k:k + 1], beta)[0], W[k])
    print('%s: the kernel uses %.3f of the bound at most' % (tc.spec_id(s), worst))


@pytest.mark.parametrize('s', [(65, 17, 1.0, 0.5), (300, 5, 1.0, 0.0)], ids=tc.spec_id)
def test_weights_of_a_nan_state_are_nan_and_stay_in_their_row(s):
    X = tc.weight_queries(s)['rand'][0][:5].copy()
    h = handle(s, 'rand')
    single = [h.weights(X[k:k + 1], 3.0)[0] for k in range(5)]
    X[2, s[1]] = np.nan                                                  # a position coordinate
    W = h.weights(X, 3.0)
    assert np.isnan(W[2]).all()
    for k in (0, 1, 3, 4):
        assert np.array_equal(W[k], single[k])


# ---------------------------------------------------------------------------------------- stpwl_linearize_weighted (the blend)
@pytest.mark.parametrize('shape', tc.BLEND_SHAPES, ids=lambda t: '-'.join(map(str, t)))
def test_blend_within_the_bound_with_the_kernels_own_weights(shape):
    """blend_kernel in isolation: with the W the call returns, every element of A/B/d within (P + 2) eps sum_i |w_i T_i| of the
    long-double sum.  n_x^2 + n_x m + n_x just below, at and just above multiples of 256 (the grid.y tiling)."""
    r, m, P = shape
    model, X = tc.blend_case(*shape)
    h = Handle(dict(model, A_d=model['A_c'], B_d=model['B_c'], d_d=model['d_c']))
    A, B, d, W = h.linearize_weighted(X, 3.0)
    assert np.array_equal(W, h.weights(X, 3.0))
    for k in range(len(X)):
        assert abs(W[k].sum() - 1.0) <= (P + 16) * tr.EPS and (W[k] > 0).sum() >= 2
        for got, T, name in ((A[k], model['A_c'], 'A'), (B[k], model['B_c'], 'B'), (d[k], model['d_c'], 'd')):
            err, bound = np.abs(got - tr.blend(W[k], T)), (P + 2) * tr.EPS * tr.blend_abs(W[k], T)
            assert (err <= bound).all(), (name, k, int(np.argmax(err - bound)))
