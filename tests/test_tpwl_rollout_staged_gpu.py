"""GPU: the TPWL rollout with the region panel staged in LDS (csrc/tpwl.hip: rollout_staged_kernel) against the plain kernel of a handle
created under SRH_TPWL_ROLLOUT_PLAIN=1 -- X and Z bit for bit -- and against oracle.tpwl.rollout at the tolerance of
tests/test_tpwl_gpu.py (1e-10 of the largest value).  The handles are made through the C ABI with discrete tables of the test's own, so
that the sequence of nearest points is under the test's control; inputs are random and non-zero (zero inputs never show the order of the
B u sums); no state is non-finite (every search gives index 0 for one -- the rule of csrc/tpwl_dev.h, tested through the index-only
entry points in tests/test_tpwl_table_exact_gpu.py; a rollout from such a state only carries the NaN on)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import tpwl as otpwl

pytestmark = pytest.mark.gpu


def close(a, b, rtol=1e-10):
    np.testing.assert_allclose(a, b, rtol=0, atol=rtol * max(1.0, float(np.abs(b).max())))


class Handle:
    """stpwl handle over a model dict and its discrete tables; plain=True: created under SRH_TPWL_ROLLOUT_PLAIN=1."""

    def __init__(self, model, Ad, Bd, dd, H, z_ref, plain=False):
        from sofacontrol_amd import _lib
        self._lib = _lib
        P, r = model['q'].shape
        self.n, self.m, self.nz = 2 * r, model['u'].shape[1], H.shape[0]
        self.h = C.c_void_p()
        f = _lib.f64
        tabs = [f(model[k]) for k in ('q', 'v', 'u', 'A_c', 'B_c', 'd_c')] + [f(Ad), f(Bd), f(dd)]
        old = os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
        try:
            if plain:
                os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = '1'
            _lib.check(_lib.lib().stpwl_create(C.byref(self.h), C.c_int(P), C.c_int(r), C.c_int(self.m), *[_lib.dptr(t) for t in tabs],
                                               C.c_double(model['w_q']), C.c_double(model['w_v'])), 'stpwl_create')
        finally:
            os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
            if old is not None:
                os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = old
        _lib.check(_lib.lib().stpwl_set_output(self.h, _lib.dptr(f(H)), _lib.dptr(f(z_ref)), C.c_int(self.nz)), 'stpwl_set_output')

    def plan(self, N, batch):
        return self._lib.tpwl_rollout_plan(self.h, N, batch)

    def rollout(self, x0, u):
        _lib = self._lib
        x0, u = _lib.f64(x0), _lib.f64(u)
        Bn, N = u.shape[0], u.shape[1]
        X = np.full((Bn, N + 1, self.n), np.nan)
        Z = np.full((Bn, N + 1, self.nz), np.nan)
        _lib.check(_lib.lib().stpwl_rollout(self.h, _lib.dptr(x0), _lib.dptr(u), C.c_int(N), C.c_int64(Bn), _lib.dptr(X), _lib.dptr(Z)),
                   'stpwl_rollout')
        return X, Z

    def __del__(self):
        try:
            self._lib.lib().stpwl_destroy(self.h)
        except Exception:
            pass


def output_model(r, seed):
    rng = np.random.default_rng(seed)
    return otpwl.synthetic_output_matrix(r, seed=seed), rng.uniform(-100.0, 100.0, 6)


_cases = {}


def shape_case(r, m, P, N, batch, w_v=0.0):
    """The model of tests/test_tpwl_gpu.py (points a tenth apart, zero-order-hold tables at dt = 0.05: the rollouts cross regions), its
    oracle trajectories and both handles; built once per shape."""
    key = (r, m, P, N, batch, w_v)
    if key not in _cases:
        model = otpwl.synthetic_model(r, m, P, seed=r + m, w_v=w_v)
        model['q'] *= 0.1
        Ad, Bd, dd = otpwl.pre_discretize(model, 0.05, 'zoh')
        H, z_ref = output_model(r, 7 * r + m)
        rng = np.random.default_rng(1000 * r + 10 * m + N)
        x0 = 0.01 * rng.standard_normal((batch, 2 * r))
        u = rng.uniform(1.0, 800.0, (batch, N, m))
        Xo = np.stack([otpwl.rollout(model, Ad, Bd, dd, x0[b], u[b]) for b in range(batch)])
        assert np.isfinite(Xo).all()
        staged = Handle(model, Ad, Bd, dd, H, z_ref)
        plain = Handle(model, Ad, Bd, dd, H, z_ref, plain=True)
        _cases[key] = dict(model=model, tabs=(Ad, Bd, dd), H=H, z_ref=z_ref, x0=x0, u=u, Xo=Xo, staged=staged, plain=plain)
    return _cases[key]


def check_against_plain_and_oracle(c, want_staged, want_held):
    x0, u = c['x0'], c['u']
    batch, N = u.shape[0], u.shape[1]
    plan = c['staged'].plan(N, batch)
    assert (plan['staged'], plan['held']) == (want_staged, want_held), plan
    assert plan['lds_bytes'] <= 64 * 1024
    pp = c['plain'].plan(N, batch)
    assert (pp['staged'], pp['held']) == (False, False), pp
    Xs, Zs = c['staged'].rollout(x0, u)
    Xp, Zp = c['plain'].rollout(x0, u)
    assert np.array_equal(Xs, Xp) and np.array_equal(Zs, Zp)
    close(Xs, c['Xo'])
    close(Zs, np.einsum('aj,bkj->bka', c['H'], c['Xo']) + c['z_ref'])


# (r, m, P, N, batch) -> (staged, held)
SHAPES = [((30, 4, 64, 50, 6), (True, True)),          # the bench shape
          ((5, 3, 9, 10, 1), (True, True)),            # small, batch 1
          ((30, 8, 64, 12, 3), (True, True)),          # n_u = 8: two input rows per slice
          ((32, 4, 64, 8, 2), (True, True)),           # last held-table size (n_x = 64: the whole of wave 0)
          ((33, 4, 64, 8, 2), (True, False)),          # first size on nearest_wave (n_x = 66: the sums span two waves)
          ((36, 4, 20, 12, 3), (True, False)),         # shipped basis
          ((30, 4, 65, 8, 2), (True, False)),          # P > 64
          ((2, 1, 1, 5, 2), (True, True)),             # one point
          ((46, 4, 8, 6, 2), (False, False))]          # layout above 64 KB: plain


@pytest.mark.parametrize('shape,path', SHAPES, ids=['-'.join(map(str, s)) for s, _ in SHAPES])
def test_staged_equals_plain_and_oracle(shape, path):
    check_against_plain_and_oracle(shape_case(*shape), *path)


def test_velocity_weighted_model_takes_the_wave_search():
    """w_v != 0: both distances, tpwl::nearest_wave on the staged path."""
    c = shape_case(6, 3, 12, 12, 3, w_v=0.5)
    idx = [otpwl.nearest_points(c['model'], x[:-1]) for x in c['Xo']]
    assert any(len(set(i.tolist())) > 1 for i in idx)
    check_against_plain_and_oracle(c, True, False)


@pytest.mark.parametrize('N', [0, 1])
def test_empty_and_one_stage_horizons(N):
    check_against_plain_and_oracle(shape_case(5, 3, 9, N, 3), True, True)
    check_against_plain_and_oracle(shape_case(33, 4, 64, N, 2), True, False)


# ---------------------------------------------------------------------------------------- region changes
def jump_model(kind, r=5, m=3, P=9, N=10, seed=11):
    """Tables of the test's own: d_d[i] = [0 ; q_next(i)] with small A_d, B_d, so that the state of the next stage lies next to the point
    next(i) (the points are ~9 apart, A x + B u stays under ~1).
    'every': next(i) = i + 1 mod P -- a change at every stage;
    'first': next(i) = c for every i, x0 next to a != c -- i_0 = a, then c for good;
    'last':  next(i) = i, and B_d[a][:, 0] = [0 ; q_c - q_a] with u_0 = 1 at stage N - 2 only -- a for the stages 0 .. N - 2, c at N - 1."""
    rng = np.random.default_rng(seed)
    n = 2 * r
    model = otpwl.synthetic_model(r, m, P, seed=seed)
    q = model['q']
    Ad = 0.02 * rng.standard_normal((P, n, n))
    Bd = 0.05 * rng.standard_normal((P, n, m))
    dd = 0.01 * rng.standard_normal((P, n))
    a, c = 2, 6
    nxt = {'every': lambda i: (i + 1) % P, 'first': lambda i: c, 'last': lambda i: i}[kind]
    for i in range(P):
        dd[i, r:] += q[nxt(i)]
    x0 = np.concatenate((0.1 * rng.standard_normal(r), q[a] + 0.1 * rng.standard_normal(r)))
    u = rng.uniform(0.05, 0.3, (N, m))
    if kind == 'last':
        Bd[a, :, 0] = 0.0
        Bd[a, r:, 0] = q[c] - q[a]
        u[:, 0] = rng.uniform(0.01, 0.03, N)
        u[N - 2, 0] = 1.0
    H, z_ref = output_model(r, seed + 1)
    return model, Ad, Bd, dd, H, z_ref, x0, u


@pytest.mark.parametrize('kind', ['every', 'first', 'last'])
def test_region_changes_reload_the_panel(kind):
    model, Ad, Bd, dd, H, z_ref, x0, u = jump_model(kind)
    N = u.shape[0]
    Xo = otpwl.rollout(model, Ad, Bd, dd, x0, u)
    idx = otpwl.nearest_points(model, Xo[:N])                     # i_0 .. i_{N-1}: the regions the N stages run in
    changes = np.flatnonzero(idx[1:] != idx[:-1]) + 1             # the stages whose region differs from the stage before
    if kind == 'every':
        assert len(changes) >= N - 1, idx
    elif kind == 'first':
        assert changes.tolist() == [1], idx
    else:
        assert changes.tolist() == [N - 1], idx
    assert np.isfinite(Xo).all()
    staged, plain = Handle(model, Ad, Bd, dd, H, z_ref), Handle(model, Ad, Bd, dd, H, z_ref, plain=True)
    assert staged.plan(N, 2)['staged'] and staged.plan(N, 2)['held']
    assert not plain.plan(N, 2)['staged']
    # a second rollout beside it that starts in another region: the panels of the two workgroups differ
    x0b = np.stack((x0, np.concatenate((x0[:5], model['q'][4] + 0.1))))
    ub = np.stack((u, u[::-1].copy()))
    Xs, Zs = staged.rollout(x0b, ub)
    Xp, Zp = plain.rollout(x0b, ub)
    assert np.array_equal(Xs, Xp) and np.array_equal(Zs, Zp)
    close(Xs[0], Xo)
    close(Xs[1], otpwl.rollout(model, Ad, Bd, dd, x0b[1], ub[1]))
    close(Zs[0], (H @ Xo.T).T + z_ref)


# ---------------------------------------------------------------------------------------- more rollouts than resident workgroups
def test_batch_above_the_resident_workgroups():
    """1100 rollouts (256 CUs x 4 staged workgroups = 1024 slots) at (5, 3, 9, 4): three calls give the same bits, four sampled rows equal
    their one-rollout calls, and the plain kernel agrees."""
    r, m, P, N, batch = 5, 3, 9, 4, 1100
    c = shape_case(r, m, P, N, 4)
    rng = np.random.default_rng(5)
    x0 = 0.01 * rng.standard_normal((batch, 2 * r))
    u = rng.uniform(1.0, 800.0, (batch, N, m))
    assert c['staged'].plan(N, batch)['staged']
    X1, Z1 = c['staged'].rollout(x0, u)
    assert np.isfinite(X1).all() and np.isfinite(Z1).all()
    for _ in range(2):
        X2, Z2 = c['staged'].rollout(x0, u)
        assert np.array_equal(X1, X2) and np.array_equal(Z1, Z2)
    Xp, Zp = c['plain'].rollout(x0, u)
    assert np.array_equal(X1, Xp) and np.array_equal(Z1, Zp)
    for b in (0, 511, 1024, 1099):
        Xb, Zb = c['staged'].rollout(x0[b:b + 1], u[b:b + 1])
        assert np.array_equal(Xb[0], X1[b]) and np.array_equal(Zb[0], Z1[b])
        close(X1[b], otpwl.rollout(c['model'], *c['tabs'], x0[b], u[b]))
