"""Koopman model identification (EDMD) on the device: records (y, u) -> a KoopmanModel that KoopmanMPC, KoopmanSolverNode and
KoopmanClosedLoopBatch accept unchanged (csrc/koopman_fit.hip; C ABI: skoop_fit_* in include/sofacontrol_hip.h).

THE FIT.  The reference's model was trained by an external MATLAB package that is not part of it; this text defines the fit.
  Records: E episodes, each y (T x n_y), u (T x m), raw (unscaled).  `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode: a
  record at dt_sim becomes one at Ts = s dt_sim (the input is held over a controller step, so row i s carries it).  T' = rows kept.
  zeta_i = [y_i, y_{i-1} .. y_{i-d}, u_{i-1} .. u_{i-d}] of scaled samples for kept row i >= d (d = delays) -- what
  KoopmanLift.embed_lift builds, a scaled sample (v - offset) / factor being rounded once here (within one ulp of the lift's, which
  rounds the subtraction and the division separately) -- and psi_i = psi(zeta_i), the observables of `observable_exponents` (the constant last unless DMD).
  Input of a pair: v_i = scale_down(u[i + u_lag]), u_lag in {0, 1}.  u_lag = 0: row i holds the input applied AFTER y_i (the layout
  of the closed loops' own res.y / res.u, and of the trainer's data).  u_lag = 1: row i holds the input applied BEFORE y_i (the rows
  KoopmanData.add_measurement(y, u_prev) and the device ring keep).  A model meant for the online controller must be fitted on the
  zeta the controller builds; that is why u_lag is a parameter.
  Pairs (i, i + 1) for d <= i <= T' - 2; never across an episode; an episode with T' <= d + 1 contributes nothing.
  Sums, with Phi_i = [psi_i; v_i] (n = P + m): G = sum Phi_i Phi_i^T, R = sum psi_{i+1} Phi_i^T, Q = sum |psi_{i+1}|^2, S = pairs.
  Model: [A B] = R (G + ridge I)^-1, ridge >= 0 -- the minimiser of sum |psi_{i+1} - A psi_i - B v_i|^2 + ridge |[A B]|_F^2.
  C (n_y x P) has one 1 per row, at the observable whose exponent vector is e_j (read from observable_exponents); M and K are None;
  W = V = I; params: n, m, N = P, nzeta, delays, obs_degree, obs_type 'poly', Ts, scale.
  Scaling: given (a dict of y_offset / y_factor / u_offset / u_factor), or computed on the device from the kept rows of the first
  records added: offset = (max + min) / 2, factor = (max - min) / 2, which maps the data to [-1, 1].  A channel with max == min is
  refused by name.
  Failure: a pivot of G + ridge I that is not positive, not finite, or not above n eps of its diagonal entry (its sign would be
  rounding noise) raises (the pivot is named: increase ridge); S == 0 is refused.
  Limits: n = P + m <= 128, and the lift's own (nzeta <= 64, degree <= 4).

NOT OFFERED: the trainer's L1 (lasso) constraint; sample weights; non-polynomial observables; truncation (W): a lift with W is
refused."""
import ctypes as C

import numpy as np

from ... import _lib
from . import koopman_utils as ku

_BOUND = False
MAX_N = 128


def _bind():
    global _BOUND
    L = ku._bind()
    if _BOUND:
        return L
    vp, dp, i64, ip = C.c_void_p, _lib.c_double_p, C.c_int64, C.POINTER(C.c_int)
    L.skoop_fit_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, ip, C.POINTER(i64)]
    L.skoop_fit_create.argtypes = [C.POINTER(vp), vp]
    L.skoop_fit_destroy.argtypes = [vp]
    L.skoop_fit_reset.argtypes = [vp]
    L.skoop_fit_minmax.argtypes = [dp, dp, i64, i64, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp]
    L.skoop_fit_minmax_dev.argtypes = [vp, vp, i64, i64, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, vp]
    L.skoop_fit_add.argtypes = [vp, dp, dp, i64, i64, C.c_int, C.c_int]
    L.skoop_fit_add_dev.argtypes = [vp, vp, vp, i64, i64, C.c_int, C.c_int, vp]
    L.skoop_fit_sums.argtypes = [vp, dp, dp, dp, C.POINTER(i64)]
    L.skoop_fit_solve.argtypes = [vp, C.c_double, dp, dp, _lib.c_int32_p]
    _BOUND = True
    return L


def fit_plan(nzeta, degree, DMD, m):
    """skoop_fit_plan, on the host (no GPU): {'n_psi', 'n', 'rows_per_chunk', 'lds_bytes'}; raises when the shape is refused."""
    a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    _lib.check(_bind().skoop_fit_plan(int(nzeta), int(degree), 1 if DMD else 0, int(m), C.byref(a), C.byref(b), C.byref(c), C.byref(d)),
               'skoop_fit_plan')
    return {'n_psi': a.value, 'n': b.value, 'rows_per_chunk': c.value, 'lds_bytes': int(d.value)}


def _check_scale(scale, n_y, m):
    s = ku.KoopmanScaling(scale)
    out = {}
    for key, w, name in (('y_offset', n_y, 'y'), ('y_factor', n_y, 'y'), ('u_offset', m, 'u'), ('u_factor', m, 'u')):
        v = np.ravel(getattr(s, key)).astype(np.float64)
        if v.shape != (w,):
            raise RuntimeError('KoopmanSysID: scale[%r] must have %d entries, got %d' % (key, w, v.size))
        if not np.all(np.isfinite(v)):
            raise RuntimeError('KoopmanSysID: scale[%r] holds a non-finite entry' % key)
        if key.endswith('factor') and np.any(v == 0.0):
            raise RuntimeError('KoopmanSysID: channel %s[%d] is constant (factor 0): it cannot be scaled' % (name, int(np.argmax(v == 0.0))))
        out[key] = v.reshape(1, w)
    return out


def _records(Y, U, n_y, m, shape, who):
    """(Y, U, E, T, on_device) of records given as arrays ((E, T, n_y) / (T, n_y)) or DeviceBuffers with shape = (E, T)."""
    dev = isinstance(Y, _lib.DeviceBuffer)
    if dev != isinstance(U, _lib.DeviceBuffer):
        raise RuntimeError('%s: Y and U must both be arrays or both be DeviceBuffers' % who)
    if dev:
        if shape is None or len(tuple(shape)) != 2:
            raise RuntimeError('%s: DeviceBuffer records need shape = (E, T)' % who)
        E, T = int(shape[0]), int(shape[1])
        if E < 1 or T < 1 or Y.nbytes < 8 * E * T * n_y or U.nbytes < 8 * E * T * m:
            raise RuntimeError('%s: the DeviceBuffers are smaller than (E, T, n_y) = (%d, %d, %d) and (E, T, m) = (%d, %d, %d) doubles'
                               % (who, E, T, n_y, E, T, m))
        return Y, U, E, T, True
    Y, U = np.asarray(Y, dtype=np.float64), np.asarray(U, dtype=np.float64)
    if Y.ndim == 2:
        Y = Y[None]
    if U.ndim == 2:
        U = U[None]
    if Y.ndim != 3 or Y.shape[2] != n_y or Y.shape[0] < 1 or Y.shape[1] < 1:
        raise RuntimeError('%s: Y must have shape (E, T, n_y) or (T, n_y) with n_y = %d, got %r' % (who, n_y, tuple(np.shape(Y))))
    if U.shape != (Y.shape[0], Y.shape[1], m):
        raise RuntimeError('%s: U (E, T, m) must have shape %r, got %r' % (who, (Y.shape[0], Y.shape[1], m), tuple(U.shape)))
    return _lib.f64(Y), _lib.f64(U), Y.shape[0], Y.shape[1], False


def _check_layout(stride, u_lag, who):
    if int(stride) != stride or stride < 1:
        raise RuntimeError('%s: stride = %r, need an integer stride >= 1' % (who, stride))
    if u_lag not in (0, 1):
        raise RuntimeError('%s: u_lag = %r, need 0 (row i holds the input applied after y_i) or 1 (before y_i)' % (who, u_lag))


class KoopmanFitResult:
    """pairs (S), ridge, and residual_rms = sqrt((Q - 2 tr(X R^T) + tr(X G X^T)) / (S P)), X = [A B]: the one-step residual of the fit per
    observable, from the sums (the three terms cancel: of an exact fit about sqrt(eps) of the observables' rms survives)."""

    def __init__(self, pairs, ridge, residual_rms):
        self.pairs, self.ridge, self.residual_rms = pairs, ridge, residual_rms

    def __repr__(self):
        return 'KoopmanFitResult(pairs=%d, ridge=%g, residual_rms=%g)' % (self.pairs, self.ridge, self.residual_rms)


class KoopmanSysID:
    """Accumulates the sums of the fit over any number of `add` calls and solves for the model (the module's docstring states the fit).
    With scale=None the first `add` fixes the scale from its own records."""

    def __init__(self, n_y, m, Ts, obs_degree=2, delays=1, DMD=False, scale=None):
        self.n_y, self.m, self.Ts = int(n_y), int(m), float(Ts)
        self.obs_degree, self.delays, self.DMD = int(obs_degree), int(delays), bool(DMD)
        if self.n_y < 1 or self.m < 1 or self.obs_degree < 1 or self.delays < 0 or not self.Ts > 0:
            raise RuntimeError('KoopmanSysID: need n_y, m, obs_degree >= 1, delays >= 0 and Ts > 0')
        self.nzeta = self.n_y * (self.delays + 1) + self.m * self.delays
        plan = fit_plan(self.nzeta, self.obs_degree, self.DMD, self.m)      # refuses n > 128 and the lift's limits, on the host
        self.n_psi, self.n, self.rows_per_chunk = plan['n_psi'], plan['n'], plan['rows_per_chunk']
        self.scale = None if scale is None else _check_scale(scale, self.n_y, self.m)
        self._lift, self._h, self._pairs = None, C.c_void_p(), 0

    @classmethod
    def for_lift(cls, lift, Ts):
        """A fit on the shape and scaling of an existing KoopmanLift; a lift that projects with W is refused (no truncated models)."""
        if getattr(lift, 'has_w', False):
            raise RuntimeError('KoopmanSysID: the lift projects with W; truncated models are not fitted')
        sc = dict(zip(('y_offset', 'y_factor', 'u_offset', 'u_factor'), lift._scale))
        return cls(lift.n_y, lift.m, Ts, obs_degree=lift.degree, delays=lift.delays, DMD=lift.DMD, scale=sc)

    @property
    def pairs(self):
        return self._pairs

    def _ensure(self):
        if self._lift is None:
            s = self.scale
            self._lift = ku.KoopmanLift(self.n_y, self.m, self.delays, self.obs_degree, DMD=self.DMD, y_offset=s['y_offset'],
                                        y_factor=s['y_factor'], u_offset=s['u_offset'], u_factor=s['u_factor'])
            _lib.check(_bind().skoop_fit_create(C.byref(self._h), self._lift._h), 'skoop_fit_create')

    def add(self, Y, U, stride=1, u_lag=0, shape=None, stream=None):
        """Adds records to the sums: Y (E, T, n_y) or (T, n_y) and U alike, numpy arrays or _lib.DeviceBuffers with shape = (E, T)
        (device records are read in place, asynchronously on `stream`).  Returns the pairs added."""
        _check_layout(stride, u_lag, 'KoopmanSysID.add')
        Y, U, E, T, dev = _records(Y, U, self.n_y, self.m, shape, 'KoopmanSysID.add')
        L = _bind()
        if self.scale is None:
            sc = [np.zeros(self.n_y), np.zeros(self.n_y), np.zeros(self.m), np.zeros(self.m)]
            if dev:
                _lib.check(L.skoop_fit_minmax_dev(Y.ptr, U.ptr, E, T, self.n_y, self.m, int(stride), *[_lib.dptr(v) for v in sc], stream),
                           'skoop_fit_minmax_dev')
            else:
                _lib.check(L.skoop_fit_minmax(_lib.dptr(Y), _lib.dptr(U), E, T, self.n_y, self.m, int(stride), *[_lib.dptr(v) for v in sc]),
                           'skoop_fit_minmax')
            self.scale = _check_scale(dict(zip(('y_offset', 'y_factor', 'u_offset', 'u_factor'), sc)), self.n_y, self.m)
        self._ensure()
        if dev:
            _lib.check(L.skoop_fit_add_dev(self._h, Y.ptr, U.ptr, E, T, int(stride), int(u_lag), stream), 'skoop_fit_add_dev')
        else:
            _lib.check(L.skoop_fit_add(self._h, _lib.dptr(Y), _lib.dptr(U), E, T, int(stride), int(u_lag)), 'skoop_fit_add')
        added = E * max(0, (T - 1) // int(stride) + 1 - 1 - self.delays)
        self._pairs += added
        return added

    def sums(self):
        """{'G' (n x n), 'R' (n_psi x n), 'Q', 'pairs'} as accumulated so far (synchronises the device)."""
        if self._lift is None:
            return {'G': np.zeros((self.n, self.n)), 'R': np.zeros((self.n_psi, self.n)), 'Q': 0.0, 'pairs': 0}
        G, R, Q, S = np.zeros((self.n, self.n)), np.zeros((self.n_psi, self.n)), C.c_double(0.0), C.c_int64(0)
        _lib.check(_bind().skoop_fit_sums(self._h, _lib.dptr(G), _lib.dptr(R), C.cast(C.byref(Q), _lib.c_double_p), C.byref(S)), 'skoop_fit_sums')
        assert S.value == self._pairs
        return {'G': G, 'R': R, 'Q': Q.value, 'pairs': S.value}

    def solve_AB(self, ridge=0.0):
        """(A, B) of [A B] = R (G + ridge I)^-1 by the device's Cholesky; raises (code SRH_ENUMERIC) on a failing pivot."""
        if not (ridge >= 0.0 and np.isfinite(ridge)):
            raise RuntimeError('KoopmanSysID.solve: need a finite ridge >= 0, got %r' % (ridge,))
        if self._pairs == 0:
            raise RuntimeError('KoopmanSysID.solve: no pairs have been added (S = 0)')
        A, B, info = np.zeros((self.n_psi, self.n_psi)), np.zeros((self.n_psi, self.m)), np.full(1, -1, dtype=np.int32)
        rc = _bind().skoop_fit_solve(self._h, float(ridge), _lib.dptr(A), _lib.dptr(B), _lib.iptr(info))
        self.last_info = int(info[0])
        _lib.check(rc, 'skoop_fit_solve')
        return A, B

    def solve(self, ridge=0.0):
        """The fitted KoopmanModel."""
        A, B = self.solve_AB(ridge)
        return self._model(A, B)

    def _model(self, A, B):
        exps = ku.observable_exponents(self.nzeta, self.obs_degree, self.DMD)
        Cm = np.zeros((self.n_y, self.n_psi))
        for j in range(self.n_y):
            e = np.zeros(self.nzeta, dtype=exps.dtype)
            e[j] = 1
            at = np.flatnonzero((exps == e).all(axis=1))
            assert at.size == 1
            Cm[j, at[0]] = 1.0
        params = dict(n=self.n_y, m=self.m, N=self.n_psi, nzeta=self.nzeta, delays=self.delays, obs_degree=self.obs_degree, obs_type='poly',
                      Ts=self.Ts, scale={k: v.copy() for k, v in self.scale.items()})
        return ku.KoopmanModel(dict(A=A, B=B, C=Cm), params, DMD=self.DMD)

    def reset(self):
        """Sums and pairs back to zero; the scale stays."""
        if self._lift is not None:
            _lib.check(_bind().skoop_fit_reset(self._h), 'skoop_fit_reset')
        self._pairs = 0

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                _lib.lib().skoop_fit_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def residual_rms(sums, A, B):
    """sqrt((Q - 2 tr(X R^T) + tr(X G X^T)) / (S P)) with X = [A B], clipped at 0."""
    X = np.hstack([A, B])
    r2 = sums['Q'] - 2.0 * np.sum(X * sums['R']) + np.sum((X @ sums['G']) * X)
    return float(np.sqrt(max(r2, 0.0) / (max(1, sums['pairs']) * A.shape[0])))


def fit_koopman(Y, U, Ts, obs_degree=2, delays=1, DMD=False, scale=None, stride=1, u_lag=0, ridge=0.0, shape=None, n_y=None, m=None):
    """The one-call form: records -> (KoopmanModel, KoopmanFitResult).  Arrays give n_y and m by their last axis; DeviceBuffers need
    shape = (E, T), n_y and m."""
    if not isinstance(Y, _lib.DeviceBuffer):
        n_y, m = np.shape(Y)[-1], np.shape(U)[-1]
    elif n_y is None or m is None:
        raise RuntimeError('fit_koopman: DeviceBuffer records need n_y and m')
    sid = KoopmanSysID(n_y, m, Ts, obs_degree=obs_degree, delays=delays, DMD=DMD, scale=scale)
    sid.add(Y, U, stride=stride, u_lag=u_lag, shape=shape)
    A, B = sid.solve_AB(ridge)
    res = KoopmanFitResult(sid.pairs, float(ridge), residual_rms(sid.sums(), A, B))
    return sid._model(A, B), res


def one_step_error(model, Y, U, stride=1, u_lag=0):
    """rms over pairs and observables of psi_{i+1} - A psi_i - B v_i on held-out records (arrays (E, T, n_y) / (T, n_y)), the pairs
    and v_i as the fit defines them; psi from the model's own lift_record."""
    _check_layout(stride, u_lag, 'one_step_error')
    Y, U, E, T, _ = _records(Y, U, model.n, model.m, None, 'one_step_error')
    d, tot, cnt = model.delays, 0.0, 0
    for e in range(E):
        y, u = Y[e, ::stride], U[e, ::stride]
        if y.shape[0] <= d + 1:
            continue
        psi = model.lift_record(y, u, project=False)                     # rows i = d .. T' - 1
        v = model.scaling.scale_down(u=u)[d + u_lag:y.shape[0] - 1 + u_lag]
        err = psi[1:] - psi[:-1] @ model.A_d.T - v @ model.B_d.T
        tot += float(np.sum(err * err))
        cnt += err.size
    if cnt == 0:
        raise RuntimeError('one_step_error: the records hold no pair')
    return float(np.sqrt(tot / cnt))
