"""Seeded SSM model problems shared by tests/test_ssm_reference_cpu.py (which checks the input conditions without a GPU) and
tests/test_ssm_exact_gpu.py (which runs the kernels of csrc/ssm.hip / csrc/ssm_dev.h on them).

Models: workloads.ssm_model(n, m, rom_order, ssm_order, seed=500 + n).  Its oscillator pairs [[-zt, -w], [w, -zt]] (w > zt) make
inv(A_c) exchange rows at every pair while I - h A_c needs none: both pivot outcomes occur at every shape with n >= 2.
Points per shape: x = amp N(0, 1), amp in AMPS, DRAWS draws each, u = N(0, 1), from default_rng(n).  Every input is generated
here, once, so that the long-double reference, the float64 oracle and the device are driven by the same numbers; whatever the
functions below return is cached: treat it as read-only."""
import numpy as np

import ssm_reference as sr
from oracle import ssm as ossm

E_ORACLE_MAX = 1e-11

# (n_x, n_u, rom order, ssm order): the smallest shape that reaches what its comment names
SHAPES = [
    (1, 1, 7, 7),        # ld = 1, the highest admitted order
    (2, 3, 4, 1),        # n_u = n_x + 1 = ld: the limit of the B_d scratch panel; linear observer
    (5, 5, 3, 3),        # odd n: ld = n, no padding column; EP = 1
    (8, 1, 3, 2),        # n * n = 64: the last of EP = 1; one input
    (9, 4, 2, 2),        # the first of EP = 2
    (11, 4, 2, 2),       # the last of EP = 2
    (12, 8, 2, 2),       # the first of EP = 4
    (16, 4, 2, 1),       # n * n = 256: the last of EP = 4
    (17, 4, 2, 1),       # the first of the un-gathered loop
    (24, 8, 2, 1),       # un-gathered loop, several trips of every strided loop
    (32, 8, 1, 1),       # the n_x limit; order 1: every derivative is the constant (table value -2)
    (10, 8, 3, 2),       # C3, the benchmark's shape
]
# ssm::inverse_wave (csrc/ssm_dev.h) chooses its elimination by n * n: EP entries per lane gathered in one read phase up to
# 64 / 128 / 256, the un-gathered loop above
EP1_MAX, EP2_MAX, EP4_MAX = 64, 128, 256
INVERSE_PATH = {(1, 1, 7, 7): 'EP1', (2, 3, 4, 1): 'EP1', (5, 5, 3, 3): 'EP1', (8, 1, 3, 2): 'EP1', (9, 4, 2, 2): 'EP2',
                (11, 4, 2, 2): 'EP2', (12, 8, 2, 2): 'EP4', (16, 4, 2, 1): 'EP4', (17, 4, 2, 1): 'loop', (24, 8, 2, 1): 'loop',
                (32, 8, 1, 1): 'loop', (10, 8, 3, 2): 'EP2'}
SSM_MAX_ORDER = 7        # csrc/ssm_dev.h; sssm_create refuses more
N_X_MAX = 32

AMPS = (0.05, 0.3, 1.0)
DRAWS = 3
# (label, `mode` of sssm_linearize, method of the reference / oracle, dt)
CONT = ('cont', 0, None, 0.0)
DISCRETE = [('fe@0.01', 1, 'fe', 0.01), ('be@0.01', 2, 'be', 0.01), ('be@0.05', 2, 'be', 0.05), ('bil@0.05', 3, 'bil', 0.05),
            ('map', 4, 'map', 0.01)]
MODES = [CONT] + DISCRETE
ROLL_N, ROLL_BATCH = 6, 3
# the iLQR kernel takes n_z = n_o <= 16 outputs
STAGED_SHAPES = [(1, 1, 7, 7), (2, 3, 4, 1), (5, 5, 3, 3), (9, 4, 2, 2), (12, 8, 2, 2), (16, 4, 2, 1), (10, 8, 3, 2)]


def shape_id(s):
    return 'n%d-m%d-r%d-s%d' % tuple(s)


def inverse_path(n):
    nn = n * n
    return 'EP1' if nn <= EP1_MAX else 'EP2' if nn <= EP2_MAX else 'EP4' if nn <= EP4_MAX else 'loop'


def tolerance(e_oracle):
    """The rule of tests/test_ekf_exact_gpu.py: the float64 oracle measures what float64 can do on these inputs; the factor
    100 covers the kernels' different route (Gauss-Jordan inverses, sep = inv(A_c) (A_d - I), fused multiply-adds, split sums)."""
    assert e_oracle <= E_ORACLE_MAX, e_oracle
    return max(100.0 * e_oracle, 1e-13)


def worst(got, ref):
    """Worst error over the leading (point / problem) axis."""
    assert len(got) == len(ref)
    return max(sr.err(g, r) for g, r in zip(got, ref))


_CACHE = {}


def cached(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            _CACHE[k] = fn(*key)
        return _CACHE[k]
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


@cached
def model(s):
    """The float64 coefficient arrays of a shape (n_o = n_x)."""
    import workloads
    n, m, ro, so = s
    d = workloads.ssm_model(n, m, ro, so, seed=500 + n)
    d['n_o'] = n
    return d


def reference_model(d):
    return sr.make_model(d['n'], d['m'], d['n_o'], d['rom_order'], d['ssm_order'], d['R'], d['B'], d['W'] if d['n_o'] == d['n'] else None,
                         d['V'], d['z_ref'], d.get('Rd'), d.get('Bd'))


def oracle_model(d):
    assert d['n_o'] == d['n']
    return ossm.make_model(d['n'], d['m'], d['rom_order'], d['ssm_order'], d['R'], d['B'], d['W'], d['V'], d['z_ref'], d.get('Rd'), d.get('Bd'))


@cached
def points(s):
    """X (9, n), U (9, m), Z (9, n) = z_ref + X (the arguments of sssm_reduce)."""
    n, m = s[0], s[1]
    rng = np.random.default_rng(n)
    X = np.concatenate([amp * rng.standard_normal((DRAWS, n)) for amp in AMPS])
    U = rng.standard_normal((len(AMPS) * DRAWS, m))
    return X, U, model(s)['z_ref'] + X


def evaluate(M, lib_, X, U, Z, modes=MODES, observer=True, dtype=np.float64):
    """Every output of the model kernels at the points, from the statements of module `lib_` (ssm_reference or oracle.ssm) on its
    model M: {label: array with the points on the first axis}.  Labels: lin/<mode>/A|B|d, dyn/cont|map, obs/z|H|c, reduce."""
    out = {}
    for label, _, method, dt in modes:
        if lib_ is sr:
            res = [sr.jacobians(M, x, u, dt, method) for x, u in zip(X, U)]
        else:
            res = [ossm.continuous_jacobians(M, x, u) if method is None else ossm.jacobians(M, x, u, dt, 'fe' if method == 'map' else method,
                                                                                           discrete=method == 'map') for x, u in zip(X, U)]
        for i, name in enumerate('ABd'):
            out['lin/%s/%s' % (label, name)] = np.array([r[i] for r in res], dtype=dtype)
    out['dyn/cont'] = np.array([lib_.dynamics(M, x, u) for x, u in zip(X, U)], dtype=dtype)
    if M['Rd'] is not None:
        out['dyn/map'] = np.array([lib_.dynamics(M, x, u, True) for x, u in zip(X, U)], dtype=dtype)
    if observer:
        out['obs/z'] = np.array([lib_.observe(M, x) for x in X], dtype=dtype)
        hc = [lib_.observer_jacobians(M, x) for x in X]
        out['obs/H'] = np.array([h for h, _ in hc], dtype=dtype)
        out['obs/c'] = np.array([c for _, c in hc], dtype=dtype)
    out['reduce'] = np.array([lib_.reduce(M, z) for z in Z], dtype=dtype)
    return out


def errors(got, ref):
    """{label: worst error over the points}; both dictionaries must carry the same labels."""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    return {k: worst(got[k], ref[k]) for k in ref}


def by_path(errs):
    """{lin/<mode> | dyn | obs | reduce: worst error}: the per-path figures that the tests print."""
    out = {}
    for k, e in errs.items():
        p = k.rsplit('/', 1)[0] if k.startswith('lin/') else k.split('/')[0]
        out[p] = max(out.get(p, 0.0), e)
    return out


@cached
def reference(s):
    """(long-double outputs at the points, e_oracle of the shape = worst error of oracle/ssm.py over the same points, modes and
    outputs, the same per path)."""
    X, U, Z = points(s)
    ref = evaluate(reference_model(model(s)), sr, X, U, Z, dtype=sr.LD)
    eo = errors(evaluate(oracle_model(model(s)), ossm, X, U, Z), ref)
    return ref, max(eo.values()), by_path(eo)


@cached
def rollout_inputs(s):
    """x0 (3, n), U (3, 6, m)."""
    n, m = s[0], s[1]
    rng = np.random.default_rng(1000 + n)
    return 0.3 * rng.standard_normal((ROLL_BATCH, n)), rng.standard_normal((ROLL_BATCH, ROLL_N, m))


@cached
def rollout_reference(s):
    """({mode label: (X (3, 7, n), Z (3, 7, n) with z_ref)} in long double, e_oracle measured on the rollouts)."""
    x0, U = rollout_inputs(s)
    Mr, Mo = reference_model(model(s)), oracle_model(model(s))
    ref, e_oracle = {}, 0.0
    for label, _, method, dt in DISCRETE:
        rr = [sr.rollout(Mr, a, u, dt, method) for a, u in zip(x0, U)]
        oo = [ossm.rollout(Mo, a, u, dt, 'fe' if method == 'map' else method, discrete=method == 'map') for a, u in zip(x0, U)]
        ref[label] = (np.array([r[0] for r in rr]), np.array([r[1] for r in rr]))
        e_oracle = max(e_oracle, worst([o[0] for o in oo], ref[label][0]), worst([o[1] for o in oo], ref[label][1]))
    return ref, e_oracle


def jacobian_list_cap(E):
    """Slots per compact derivative list of the staged evaluator (ssm::jacobian_list_cap): the longest list (variable j, k mod 4)
    of monomials k that contain x_j."""
    return max(int((E[g::4, j] > 0).sum()) for j in range(E.shape[1]) for g in range(4))


# ---- constructed cases ----------------------------------------------------------------------------------------------------

@cached
def exact_case():
    """Order-1 model, n = 4, m = 2, A_c anti-diagonal (+2, -2, +2, -2), small integer B, be at dt = 0.5, points and inputs in
    quarters.  inv(A_c) exchanges rows at its first two pivots (rows 0 <-> 3, 1 <-> 2: after them every row is in place), I - h A_c
    = [[1, -1], [1, 1]] / [[1, 1], [-1, 1]] per pair (0, 3) / (1, 2) has determinant 2 and needs no exchange.  Every operation
    (products of small dyadic numbers, divisions by 1 and 2) is exact in binary64: device = long double bit for bit."""
    R = np.zeros((4, 4))
    R[0, 3], R[1, 2], R[2, 1], R[3, 0] = 2.0, -2.0, 2.0, -2.0
    B = np.array([[1.0, -2.0], [3.0, 0.0], [0.0, 1.0], [-1.0, 2.0]])
    d = dict(n=4, m=2, n_o=4, rom_order=1, ssm_order=1, R=R, B=B, W=np.eye(4), V=np.eye(4), z_ref=np.zeros(4), Rd=None, Bd=None)
    X = np.array([[0.5, -0.25, 1.0, 0.75], [-1.5, 2.0, 0.25, -0.5], [0.0, 1.0, -1.0, 3.0]])
    U = np.array([[1.0, -0.5], [0.25, 2.0], [-3.0, 0.75]])
    return d, X, U, ('be', 2, 0.5)


@cached
def rectangular_case():
    """n_x = 4, n_o = 6, ssm order 2: V is 4 x 27, phi_s has six arguments.  Returns the model, Z (9, 6), the long-double
    sssm_reduce result and e_oracle of oracle.ssm.reduce on the same points."""
    rng = np.random.default_rng(46)
    n, m, no, ro, so = 4, 2, 6, 2, 2
    nr, ns = sr.exponents(n, ro).shape[0], sr.exponents(no, so).shape[0]
    assert (nr, ns) == (14, 27)
    R = np.hstack([-np.eye(n), 0.2 * rng.standard_normal((n, nr - n))])
    d = dict(n=n, m=m, n_o=no, rom_order=ro, ssm_order=so, R=R, B=rng.standard_normal((n, m)), W=0.1 * rng.standard_normal((no, ns)),
             V=0.3 * rng.standard_normal((n, ns)), z_ref=rng.standard_normal(no), Rd=None, Bd=None)
    Z = d['z_ref'] + np.concatenate([amp * rng.standard_normal((DRAWS, no)) for amp in AMPS])
    Mr = reference_model(d)
    ref = np.array([sr.reduce(Mr, z) for z in Z])
    Mo = dict(V=d['V'], Es=ossm.exponents(no, so), z_ref=d['z_ref'])
    return d, Z, ref, worst([ossm.reduce(Mo, z) for z in Z], ref)


@cached
def singular_case():
    """n = 2, m = 1, order 2: f_1 = a x_1^2 + u, f_2 = -x_2 + u / 2, so A_c = diag(2 a x_1, -1); three points, the middle one
    with x_1 = 0 exactly: inv(A_c) meets a zero pivot there (the reference raises) and nowhere else."""
    a = 1.5
    R = np.zeros((2, 5))                                          # x1, x2, x1^2, x1 x2, x2^2
    R[0, 2], R[1, 1] = a, -1.0
    WV = np.hstack([np.eye(2), np.zeros((2, 3))])
    d = dict(n=2, m=1, n_o=2, rom_order=2, ssm_order=2, R=R, B=np.array([[1.0], [0.5]]), W=WV, V=WV.copy(), z_ref=np.zeros(2),
             Rd=None, Bd=None)
    X = np.array([[0.4, -0.3], [0.0, 0.6], [-0.7, 0.2]])
    U = np.array([[0.5], [-1.0], [0.25]])
    return d, X, U


# ---- the device ------------------------------------------------------------------------------------------------------------

class DeviceModel:
    """An sssm handle made through the C ABI (needs the built library; every call but the constructor's refusals needs a GPU)."""

    def __init__(self, d):
        import ctypes as C
        from sofacontrol_amd import _lib
        self.C, self.L, self.lib, self.d = C, _lib, _lib.lib(), d
        self.n, self.m, self.no = d['n'], d['m'], d['n_o']
        f = lambda k: _lib.dptr(_lib.f64(d.get(k)))
        self.h = C.c_void_p()
        _lib.check(self.lib.sssm_create(C.byref(self.h), C.c_int(self.n), C.c_int(self.m), C.c_int(self.no), C.c_int(d['rom_order']),
                                        C.c_int(d['ssm_order']), f('R'), f('B'), f('Rd'), f('Bd'), f('W'), f('V'), f('z_ref')), 'sssm_create')

    def __del__(self):
        if getattr(self, 'h', None):
            self.lib.sssm_destroy(self.h)
            self.h = None

    def linearize(self, X, U, mode, dt):
        X, U, p = self.L.f64(X), self.L.f64(U), self.L.dptr
        Bn = X.shape[0]
        A, B, d = np.empty((Bn, self.n, self.n)), np.empty((Bn, self.n, self.m)), np.empty((Bn, self.n))
        self.L.check(self.lib.sssm_linearize(self.h, p(X), p(U), self.C.c_int64(Bn), self.C.c_int(mode), self.C.c_double(dt), p(A), p(B), p(d)),
                     'sssm_linearize')
        return A, B, d

    def dynamics(self, X, U, discrete):
        X, U, p = self.L.f64(X), self.L.f64(U), self.L.dptr
        F = np.empty((X.shape[0], self.n))
        self.L.check(self.lib.sssm_dynamics(self.h, p(X), p(U), self.C.c_int64(X.shape[0]), self.C.c_int(discrete), p(F)), 'sssm_dynamics')
        return F

    def observe(self, X, want_z=True, want_h=True, want_c=True):
        X, p = self.L.f64(X), self.L.dptr
        Bn = X.shape[0]
        Z = np.empty((Bn, self.no)) if want_z else None
        H = np.empty((Bn, self.no, self.n)) if want_h else None
        c = np.empty((Bn, self.no)) if want_c else None
        self.L.check(self.lib.sssm_observe(self.h, p(X), self.C.c_int64(Bn), p(Z), p(H), p(c)), 'sssm_observe')
        return Z, H, c

    def reduce(self, Z):
        Z, p = self.L.f64(Z), self.L.dptr
        X = np.empty((Z.shape[0], self.n))
        self.L.check(self.lib.sssm_reduce(self.h, p(Z), self.C.c_int64(Z.shape[0]), p(X)), 'sssm_reduce')
        return X

    def rollout(self, x0, U, mode, dt, with_z=True):
        x0, U, p = self.L.f64(x0), self.L.f64(U), self.L.dptr
        Bn, N = U.shape[0], U.shape[1]
        X = np.empty((Bn, N + 1, self.n))
        Z = np.empty((Bn, N + 1, self.no)) if with_z else None
        self.L.check(self.lib.sssm_rollout(self.h, p(x0), p(U), self.C.c_int(N), self.C.c_int64(Bn), self.C.c_int(mode), self.C.c_double(dt),
                                           p(X), p(Z)), 'sssm_rollout')
        return X, Z

    def ilqr_first_forward_pass(self, x0, U, mode, dt):
        """silqr_solve_ssm with max_iter = -1: the loop of ilqr_kernel runs `while (!converged && it <= max_iter)`, so only the
        initial forward pass of u_warm runs -- the staged evaluator at every stage -- and x is its rollout.  Identity weights,
        zero targets.  Returns x (batch, N + 1, n), iters (batch)."""
        C, L, p = self.C, self.L, self.L.dptr
        x0, U = L.f64(x0), L.f64(U)
        Bn, N = U.shape[0], U.shape[1]
        par = L.SIlqrParams()
        self.lib.silqr_default_params.restype = None
        self.lib.silqr_default_params(C.byref(par))
        par.max_iter = -1
        zt, Q, R = np.zeros((Bn, N + 1, self.no)), np.eye(self.no), np.eye(self.m)
        x, u, K = np.empty((Bn, N + 1, self.n)), np.empty((Bn, N, self.m)), np.empty((Bn, N, self.m, self.n))
        cost, iters = np.empty(Bn), np.full(Bn, -7, dtype=np.int32)
        L.check(self.lib.silqr_solve_ssm(self.h, C.c_int(mode), C.c_double(dt), C.c_int(N), C.c_int64(Bn), p(x0), p(zt), p(U), None, p(Q), p(R),
                                         p(Q), C.byref(par), p(x), p(u), p(K), p(cost), L.iptr(iters)), 'silqr_solve_ssm')
        np.testing.assert_array_equal(u, U)                       # the first pass applies u_warm as it is
        return x, iters
