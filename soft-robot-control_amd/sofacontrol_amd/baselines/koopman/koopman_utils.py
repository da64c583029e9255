"""Koopman model, data and scaling -- surface of sofacontrol/baselines/koopman/koopman_utils.py.

KoopmanScaling (86-107), KoopmanData (16-47) and the constructor checks of KoopmanModel (110-154) are host bookkeeping and
restated as they are.  The lift (get_lifting_function, 156-175: a sympy-lambdified list of monomials) runs on the device
(csrc/koopman.hip): the observable table is built in the reference's order when the handle is created, so no sympy is needed
at run time.  `KoopmanOfflineData.add_zeta_offline` and `KoopmanModel.lift_record` run the bulk embed + lift kernel."""
import ctypes as C

import numpy as np

from ... import _lib
from ...utils import load_data

_BOUND = False


def _bind():
    global _BOUND
    if _BOUND:
        return _lib.lib()
    L = _lib.lib()
    vp, dp, i64 = C.c_void_p, _lib.c_double_p, C.c_int64
    L.skoop_num_observables.argtypes = [C.c_int, C.c_int, C.c_int]
    L.skoop_exponents.argtypes = [C.c_int, C.c_int, C.c_int, _lib.c_int32_p]
    L.skoop_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, C.c_int, i64]
    L.skoop_destroy.argtypes = [vp]
    L.skoop_info.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    L.skoop_lift.argtypes = [vp, dp, i64, dp]
    L.skoop_lift_dev.argtypes = [vp, vp, i64, vp, vp]
    L.skoop_embed_lift.argtypes = [vp, dp, dp, i64, dp]
    L.skoop_embed_lift_dev.argtypes = [vp, vp, vp, i64, vp, vp]
    L.skoop_push.argtypes = [vp, dp, dp]
    L.skoop_reset.argtypes = [vp]
    L.skoop_state_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(vp)]
    L.skoop_ring_lift_dev.argtypes = [vp, vp]
    L.skoop_mpc_create.argtypes = [C.POINTER(vp), vp, vp, dp, dp]
    L.skoop_mpc_destroy.argtypes = [vp]
    L.skoop_mpc_step.argtypes = [vp, dp, dp, dp, dp, dp, dp, dp, dp, dp, _lib.c_int32_p]
    L.skoop_mpc_set_timing.argtypes = [vp, C.c_int]
    L.skoop_mpc_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), dp]
    _BOUND = True
    return L


def num_observables(nzeta, degree, DMD=False):
    return int(_bind().skoop_num_observables(int(nzeta), int(degree), 1 if DMD else 0))


def observable_exponents(nzeta, degree, DMD=False):
    """(n_psi x nzeta) exponents of the lift's observables in the reference's order (constant row last unless DMD)."""
    L = _bind()
    n = num_observables(nzeta, degree, DMD)
    out = np.zeros((n, nzeta), dtype=np.int32)
    _lib.check(L.skoop_exponents(int(nzeta), int(degree), 1 if DMD else 0, _lib.iptr(out)), 'skoop_exponents')
    return out


class KoopmanLift:
    """A device lift handle (skoop_t): scaling, delay embedding, observable table, optional W, and the online ring of
    `batch` problems.  `n_out` columns come out of every lift: rows of W, or n_psi without W (W = identity is not applied)."""

    def __init__(self, n_y, m, delays, degree, DMD=False, y_offset=None, y_factor=None, u_offset=None, u_factor=None, W=None,
                 batch=1):
        L = _bind()
        self.n_y, self.m, self.delays, self.degree, self.DMD, self.batch = int(n_y), int(m), int(delays), int(degree), bool(DMD), int(batch)
        one = lambda v, n, d: _lib.f64(np.full(n, d) if v is None else np.ravel(v))
        self._scale = [one(y_offset, n_y, 0.0), one(y_factor, n_y, 1.0), one(u_offset, m, 0.0), one(u_factor, m, 1.0)]
        self._W = None if W is None else _lib.f64(W)
        n_w = 0 if W is None else self._W.shape[0]
        self._h = C.c_void_p()
        _lib.check(L.skoop_create(C.byref(self._h), self.n_y, self.m, self.delays, self.degree, 1 if DMD else 0,
                                  *[_lib.dptr(s) for s in self._scale], _lib.dptr(self._W), n_w, C.c_int64(self.batch)),
                   'skoop_create')
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(L.skoop_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), 'skoop_info')
        self.nzeta, self.n_psi, self.n_out, self.has_w = a.value, b.value, c.value, bool(d.value)

    @classmethod
    def for_zeta(cls, nzeta, degree, DMD=False, W=None, batch=1):
        """A handle that lifts ready-made zeta rows only (no embedding: n_y = nzeta, no delays)."""
        return cls(nzeta, 1, 0, degree, DMD=DMD, W=W, batch=batch)

    def lift(self, Z):
        Z = _lib.f64(np.atleast_2d(Z))
        if Z.shape[1] != self.nzeta:
            raise RuntimeError('KoopmanLift.lift: zeta rows have %d entries, the model has nzeta = %d' % (Z.shape[1], self.nzeta))
        out = np.empty((Z.shape[0], self.n_out))
        _lib.check(_bind().skoop_lift(self._h, _lib.dptr(Z), C.c_int64(Z.shape[0]), _lib.dptr(out)), 'skoop_lift')
        return out

    def lift_dev(self, zeta_ptr, rows, out_ptr, stream=None):
        _lib.check(_bind().skoop_lift_dev(self._h, zeta_ptr, C.c_int64(rows), out_ptr, stream), 'skoop_lift_dev')

    def embed_lift(self, y, u):
        """add_zeta_offline (koopman_utils.py:75-83) + lift of a raw record: y (T x n_y), u (T x m) -> (T - delays) x n_out."""
        y = _lib.f64(np.atleast_2d(y)); u = _lib.f64(np.atleast_2d(u))
        T = y.shape[0]
        if y.shape[1] != self.n_y or u.shape != (T, self.m):
            raise RuntimeError('KoopmanLift.embed_lift: need y (T x %d), u (T x %d)' % (self.n_y, self.m))
        out = np.empty((max(0, T - self.delays), self.n_out))
        _lib.check(_bind().skoop_embed_lift(self._h, _lib.dptr(y), _lib.dptr(u), C.c_int64(T), _lib.dptr(out)), 'skoop_embed_lift')
        return out

    def embed_lift_dev(self, y_ptr, u_ptr, T, out_ptr, stream=None):
        _lib.check(_bind().skoop_embed_lift_dev(self._h, y_ptr, u_ptr, C.c_int64(T), out_ptr, stream), 'skoop_embed_lift_dev')

    def push(self, y, u):
        """One raw sample per problem into the device ring (asynchronous)."""
        y = _lib.f64(np.reshape(y, (self.batch, self.n_y))); u = _lib.f64(np.reshape(u, (self.batch, self.m)))
        _lib.check(_bind().skoop_push(self._h, _lib.dptr(y), _lib.dptr(u)), 'skoop_push')

    def reset(self):
        _lib.check(_bind().skoop_reset(self._h), 'skoop_reset')

    def state(self):
        """(ring device pointer, slots, newest slot, samples pushed, stream)."""
        p, s, h, c, st = C.c_void_p(), C.c_int(), C.c_int(), C.c_int64(), C.c_void_p()
        _lib.check(_bind().skoop_state_dev(self._h, C.byref(p), C.byref(s), C.byref(h), C.byref(c), C.byref(st)), 'skoop_state_dev')
        return p.value, s.value, h.value, c.value, st.value

    def ring_lift_dev(self, out_ptr):
        _lib.check(_bind().skoop_ring_lift_dev(self._h, out_ptr), 'skoop_ring_lift_dev')

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                _lib.lib().skoop_destroy(self._h)
                self._h = None
        except Exception:
            pass


class KoopmanData:
    """koopman_utils.py:8-47: scaled measurement history of the online controller."""

    def __init__(self, scale, delay):
        self.delay = delay
        self.scaling = KoopmanScaling(scale)
        self.y_norm = None  # Down-scaled
        self.u_norm = None  # Down-scaled

    def add_measurement(self, y, u):
        if self.y_norm is None:
            self.y_norm = self.scaling.scale_down(y=y)
            self.u_norm = self.scaling.scale_down(u=u)
        else:
            self.y_norm = np.append(self.y_norm, self.scaling.scale_down(y=y), axis=0)
            self.u_norm = np.append(self.u_norm, self.scaling.scale_down(u=u), axis=0)

    def get_zeta(self, step=-1):
        """[y[step], y[step-1 .. step-delay], u[step-1 .. step-delay]]; None before delay + 1 samples."""
        if len(self.y_norm) < self.delay + 1:
            return None
        ny, nu = self.y_norm.shape[1], self.u_norm.shape[1]
        ydel = np.zeros(self.delay * ny)
        udel = np.zeros(self.delay * nu)
        for j in range(self.delay):
            ydel[ny * j:ny * (j + 1)] = self.y_norm[step - (j + 1), :]
            udel[nu * j:nu * (j + 1)] = self.u_norm[step - (j + 1), :]
        return np.hstack([self.y_norm[step], ydel, udel])


class KoopmanOfflineData(KoopmanData):
    """koopman_utils.py:50-83."""

    def __init__(self, scale, delay):
        super().__init__(scale, delay)
        self.y = None
        self.u = None
        self.t = None
        self.zeta = None

    def load_offline_data(self, file):
        data = load_data(file)
        self.y = data['z']
        self.t = data['t']
        self.u = data['u']
        self.y_norm = self.scaling.scale_down(y=self.y)
        self.u_norm = self.scaling.scale_down(u=self.u)

    def add_zeta_offline(self):
        """zeta rows for i = delay .. T-1, through the bulk embed kernel (a degree-1 DMD lift is zeta itself: every observable
        is 1 * zeta_j, exact) on the already scaled record."""
        T, ny = self.y_norm.shape
        nu = self.u_norm.shape[1]
        emb = KoopmanLift(ny, nu, self.delay, 1, DMD=True)
        self.zeta = emb.embed_lift(self.y_norm, self.u_norm)


def _unwrap(v):
    """loadmat stores every struct field as a (1, 1) object array around the value."""
    while isinstance(v, np.ndarray) and v.dtype == object and v.size == 1:
        v = v.flat[0]
    return v


class KoopmanScaling:
    """koopman_utils.py:86-107.  `scale` is the loadmat struct (fields `[0, 0]` are (1, n) arrays) or a dict of arrays
    (kept (1, n), as the reference's results keep a leading axis of 1)."""

    def __init__(self, scale):
        def get(k):
            v = scale[k]
            if isinstance(v, np.ndarray) and v.dtype == object:
                return np.atleast_2d(np.asarray(_unwrap(v), dtype=np.float64))
            return np.atleast_2d(np.asarray(v, dtype=np.float64))
        self.y_offset = get('y_offset')
        self.y_factor = get('y_factor')
        self.u_offset = get('u_offset')
        self.u_factor = get('u_factor')

    def scale_up(self, u=None, y=None):
        if y is not None:
            return y * self.y_factor + self.y_offset
        elif u is not None:
            return u * self.u_factor + self.u_offset

    def scale_down(self, u=None, y=None):
        if y is not None:
            return (y - self.y_offset) / self.y_factor
        elif u is not None:
            return (u - self.u_offset) / self.u_factor


def _field(src, k):
    if isinstance(src, dict):
        return src[k]
    return src[k][0, 0]


def _has(src, k):
    if isinstance(src, dict):
        return k in src and src[k] is not None
    return k in src.dtype.names


class KoopmanModel:
    """koopman_utils.py:110-175.  model_in / params_in: the loadmat structs of the reference's model file
    (`loadmat(f)['py_data'][0, 0]['model']`, `['params']`) or plain dicts of arrays (params: n, m, N, nzeta, delays,
    obs_degree, obs_type, Ts, scale = dict of y_offset / y_factor / u_offset / u_factor)."""

    def __init__(self, model_in, params_in, DMD=False):
        self.A_d = np.asarray(_field(model_in, 'A'), dtype=np.float64)
        self.B_d = np.asarray(_field(model_in, 'B'), dtype=np.float64)
        self.C = np.asarray(_field(model_in, 'C'), dtype=np.float64)
        self.H = self.C.copy()
        self.M = _field(model_in, 'M') if _has(model_in, 'M') else None
        self.K = _field(model_in, 'K') if _has(model_in, 'K') else None
        # V is right matrix, W is inverse of V
        self.V = np.asarray(_field(model_in, 'V')) if _has(model_in, 'V') else np.eye(self.A_d.shape[0])
        self.W = np.asarray(_field(model_in, 'W')) if _has(model_in, 'W') else np.eye(self.A_d.shape[0])
        p = params_in if isinstance(params_in, dict) else None
        get = (lambda k: p[k]) if p is not None else (lambda k: params_in[k])
        self.n = int(np.ravel(_unwrap(get('n')))[0])
        self.m = int(np.ravel(_unwrap(get('m')))[0])
        self.N = int(np.ravel(_unwrap(get('N')))[0])
        self.state_dim = int(np.ravel(_unwrap(get('nzeta')))[0])
        self.delays = int(np.ravel(_unwrap(get('delays')))[0])
        self.obs_degree = int(np.ravel(_unwrap(get('obs_degree')))[0])
        ot = _unwrap(get('obs_type'))
        self.obs_type = str(np.ravel(ot)[0]) if isinstance(ot, np.ndarray) else str(ot)
        self.Ts = float(np.ravel(_unwrap(get('Ts')))[0])
        self.scale = get('scale') if p is not None else params_in['scale'][0, 0]
        self.DMD = DMD

        self.assert_dimensions()
        if self.obs_type != 'poly':
            raise RuntimeError('{} is not implemented / not a valid selection. Please select a different obs type'
                               .format(self.obs_type))
        self.scaling = KoopmanScaling(self.scale)
        self._lifts = {}

    def assert_dimensions(self):
        """koopman_utils.py:146-152."""
        assert self.A_d.shape == (self.N, self.N)
        assert self.B_d.shape == (self.N, self.m)
        assert self.C.shape == (self.n, self.N)

    @property
    def n_psi(self):
        return num_observables(self.state_dim, self.obs_degree, self.DMD)

    def new_lift(self, project=False, batch=1):
        """A NEW device handle of this model: psi (project=False) or W psi (project=True), with its own measurement ring of
        `batch` problems.  Every controller / solver node that pushes samples needs a handle of its own: the ring is state."""
        nz = self.n * (self.delays + 1) + self.m * self.delays
        if nz != self.state_dim:
            raise RuntimeError('KoopmanModel: nzeta = %d, but n (delays + 1) + m delays = %d' % (self.state_dim, nz))
        s = self.scaling
        return KoopmanLift(self.n, self.m, self.delays, self.obs_degree, DMD=self.DMD, y_offset=s.y_offset, y_factor=s.y_factor,
                           u_offset=s.u_offset, u_factor=s.u_factor, W=self.W if project else None, batch=batch)

    def lift_handle(self, project=False):
        """The model's cached handle for the STATELESS lifts (lift_data, lift_batch, lift_record): never pushed to."""
        key = bool(project)
        if key not in self._lifts:
            self._lifts[key] = self.new_lift(project)
        return self._lifts[key]

    def lift_data(self, *zeta):
        """The lambdified lift (koopman_utils.py:174): the n_psi observables of one zeta, computed on the device."""
        return self.lift_handle().lift(np.asarray(zeta, dtype=np.float64).reshape(1, -1))[0]

    def lift_batch(self, Z):
        """lift_data over the rows of Z (rows x nzeta) -> (rows x n_psi)."""
        return self.lift_handle().lift(Z)

    def lift_record(self, y, u, project=True):
        """Raw record y (T x n), u (T x m) -> W lift(zeta_i) (or lift(zeta_i)), i = delays .. T-1, in one kernel."""
        return self.lift_handle(project).embed_lift(y, u)
