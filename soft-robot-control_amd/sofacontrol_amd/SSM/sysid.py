"""SSM model identification on the device: records (y, u) -> the nested `model` / `params` dictionaries that SSM.__init__ reads, so that
SSMDynamics, SSMGuSTO, the SSM scp controller and SSMClosedLoopBatch take a fitted model as they take the shipped one
(csrc/ssm_fit.hip; C ABI: sssm_fit_* in include/sofacontrol_hip.h).

THE FIT.  The reference ships one model trained by an external MATLAB package and no trainer; INTEGRATION.md ("SSM model
identification") defines the fit, and this is its summary.
  Records: E episodes, each y (T x n_y), u (T x m), raw.  `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode (a record at dt_sim
  read at Ts = s dt_sim); T' = rows kept.  Row i holds the input applied after y_i.
  Chart: x_i = V^T (y_i - y_ref), V (n_y x n_x) given, or chart='pca': the n_x leading eigenvectors of C = sum (y - y_ref)(y - y_ref)^T
  over the kept rows of the FIRST records added (C on the device, the n_y x n_y eigenproblem on the host), each with the sign that
  makes its entry of largest magnitude positive.
  Samples: interior rows 1 <= i <= T' - 2, never across an episode; an episode with T' < 3 contributes nothing.
  Regressor: Phi_i = [phi(x_i); u_i], phi the monomials of the model's basis (graded, no constant) up to P = max(ROM_order, SSM_order).
  Sums (one pass): G = sum Phi Phi^T, R_d = sum x_{i+1} Phi_i^T, R_c = sum ((x_{i+1} - x_{i-1}) / (2 Ts)) Phi_i^T,
  R_w = sum (y_i - y_ref) phi(x_i)^T, the sample count and the three targets' squared norms.
  Solves: [rd_coeff Bd] and [r_coeff B] on {monomials up to ROM_order} + {inputs}, w_coeff on the monomials up to SSM_order, each block
  equilibrated by its diagonal: (D^-1/2 G_S D^-1/2 + ridge I) z = D^-1/2 r, coeff = D^-1/2 z.  v_coeff = [V^T | 0] over the basis of
  n_y variables that sssm_create expects.  A pivot that is not positive (above n eps of its unit diagonal) raises and names the pivot
  and its monomial or input; S == 0 is refused.
  Limits: n = nmon(n_x, P) + m <= 128, n_x <= 32, n_x <= n_y <= 64, orders <= 7.  The dictionaries exist for n_y = n_x only: SSM
  applies w_coeff to the basis of output_dim variables, so `solve` refuses a fit with n_y != n_x by name; `solve_coeffs` and
  `result` return its coefficients and figures.
  Records split over several `add` calls at episode boundaries give the bits of one call: a workgroup sums a fixed run of chunks of
  one episode, and the runs join the sums in order.

THE SSM HORIZON ERROR.  horizon_error judges a model the way the planners use it: rolled out open loop over H steps from every window
start of held-out records, started from the observer map as the planner starts, read in place on the device (csrc/ssm_horizon.hip;
C ABI: sssm_horizon_error; the reference's model check, examples/hardware/diamond_SSM.py module_test, for every window at once).
INTEGRATION.md ("SSM horizon error") defines it, and this is its summary.
  Records: y (E, T, n_y) raw measurements as SSMSysID.add takes them, u (E, T, m), row i holds the input applied after y_i; `stride`
  keeps rows 0, s, 2s, .. (T' kept rows); arrays, or DeviceBuffers with shape = (E, T), read in place.
  Model: an SSMDynamics: its handle, its mode (model._mode(): discrete map, fe, be or bil), dt (default float(model.Ts)) and its
  z_ref.  Required: n_x == n_o == n_y.
  Observed states: xo_j = W_map(y_j - z_ref) for every kept row (the reference's SSMObserver).
  Windows: starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, numbered episode by
  episode in row order; an episode with T' <= H has none; W = 0 raises.
  Prediction: xh_0 = xo_{j0}, or x_start (n_x,) for every window (p0 = zeros of module_test); xh_{k+1} = A_d xh_k + B_d u_{j0+k} + d_d,
  linearised at (xh_k, u_{j0+k}) and discretised by the mode at dt; zh_k = C_map(xh_k) + z_ref.  The arithmetic is the SSM closed
  loop's plant step: the X and Z + z_ref records of sgusto_ssm_loop_advance bit for bit (not the bits of SSM.rollout).
  Errors: ez_k = zh_k - y_{j0+k} (NOT zero at k = 0: C_map(W_map(.)) is not the identity); ex_k = xh_k - xo_{j0+k} (exactly 0 at k = 0
  without x_start).
  Window status: 0 ok; 1 some xh_k or zh_k is not finite; 2 some record row the window reads (y at j0 .. j0 + H, u at j0 .. j0 + H - 1) is
  not finite; 2 wins over 1.  Only status-0 windows enter the sums and the maxima.
  Results for k = 0 .. H: sse_x, sse_z; rms_x = sqrt(sse_x / (ok n_x)), rms_z = sqrt(sse_z / (ok n_o)) (NaN when no window is ok);
  worst_x, worst_z with worst_*_at = (episode, unstrided row) of that window's start, ties to the lowest window number; the counts
  windows, diverged (status 1) and bad_rows (status 2).
  On request: per_window=True gives final_x, final_z (W,) (NaN where status != 0) and status (W,); predictions=True gives x_pred
  (W, H + 1, n_x), z_pred (W, H + 1, n_o) and x_obs (E, T', n_x), together refused above the byte cap that horizon_plan states.  A window
  that left its loop at step k keeps rows 0 .. k, the rows behind are NaN; a status-2 window is not rolled out: all its rows are NaN.
  Limits, each refused on the host with the offending number: n_x <= 32, m <= 16, 1 <= H <= 1024, stride, every >= 1, the continuous
  mode, the discrete map without rd_coeff, m > (n_x | 1) in be / bil, n_x != n_o or n_y != n_o, a launch above 160 KiB of LDS.
  Not offered: the Koopman analogue, models with n_x != n_o, closed-loop (feedback) prediction, error weights.  one_step_error is
  unchanged.

NOT OFFERED: delay-embedded observations, a polynomial chart, separate autonomous and forced record sets, sample weights, fitting
inside a running loop."""
import ctypes as C

import numpy as np

from .. import _lib

_BOUND = False
MAX_N = 128


def _bind():
    global _BOUND
    L = _lib.lib()
    if _BOUND:
        return L
    vp, dp, i64, ip = C.c_void_p, _lib.c_double_p, C.c_int64, C.POINTER(C.c_int)
    L.sssm_fit_plan.argtypes = [C.c_int] * 5 + [ip, ip, ip, C.POINTER(i64)]
    L.sssm_fit_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 5 + [C.c_double, dp, dp]
    L.sssm_fit_destroy.argtypes = [vp]
    L.sssm_fit_reset.argtypes = [vp]
    L.sssm_fit_cov.argtypes = [dp, i64, i64, C.c_int, C.c_int, dp, dp, C.POINTER(i64)]
    L.sssm_fit_cov_dev.argtypes = [vp, i64, i64, C.c_int, C.c_int, dp, dp, C.POINTER(i64), vp]
    L.sssm_fit_add.argtypes = [vp, dp, dp, i64, i64, C.c_int]
    L.sssm_fit_add_dev.argtypes = [vp, vp, vp, i64, i64, C.c_int, vp]
    L.sssm_fit_sums.argtypes = [vp, dp, dp, dp, dp, dp, C.POINTER(i64)]
    L.sssm_fit_solve.argtypes = [vp, C.c_double, dp, dp, dp, dp, dp, _lib.c_int32_p]
    L.sssm_num_monomials.argtypes = [C.c_int, C.c_int]
    L.sssm_exponents.argtypes = [C.c_int, C.c_int, _lib.c_int32_p]
    i64p, i32p, dbl = C.POINTER(i64), _lib.c_int32_p, C.c_double
    hor = [C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, dp, dp, dp, i64p, i64p, dp, i32p, dp, dp, dp]
    L.sssm_horizon_plan.argtypes = [C.c_int] * 8 + [i64, i64, C.c_int, C.c_int, C.c_int, i64p, ip, i64p, i64p, i64p, i64p]
    L.sssm_horizon_error.argtypes = [vp, C.c_int, dbl, dp, dp] + hor
    L.sssm_horizon_error_dev.argtypes = [vp, C.c_int, dbl, vp, vp] + hor + [vp]
    _BOUND = True
    return L


def fit_plan(n_x, n_y, m, ROM_order, SSM_order):
    """sssm_fit_plan, on the host (no GPU): {'n_mon', 'n', 'rows_per_chunk', 'lds_bytes'}; raises when the shape is refused."""
    a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    _lib.check(_bind().sssm_fit_plan(int(n_x), int(n_y), int(m), int(ROM_order), int(SSM_order), C.byref(a), C.byref(b), C.byref(c),
                                     C.byref(d)), 'sssm_fit_plan')
    return {'n_mon': a.value, 'n': b.value, 'rows_per_chunk': c.value, 'lds_bytes': int(d.value)}


def exponents(dim, order):
    """(n_mon, dim) exponent table of the model's basis (sssm_exponents)."""
    L = _bind()
    E = np.empty((L.sssm_num_monomials(int(dim), int(order)), int(dim)), dtype=np.int32)
    _lib.check(L.sssm_exponents(int(dim), int(order), _lib.iptr(E)), 'sssm_exponents')
    return E


def pca_chart(Cov, n_x):
    """(V (n_y x n_x), eigenvalues descending) of a covariance: the n_x leading eigenvectors, each with the sign that makes its entry of
    largest magnitude positive."""
    w, Q = np.linalg.eigh(np.asarray(Cov, dtype=np.float64))
    order = np.argsort(w)[::-1]
    w, V = w[order], Q[:, order[:n_x]].copy()
    for j in range(n_x):
        if V[np.argmax(np.abs(V[:, j])), j] < 0:
            V[:, j] = -V[:, j]
    return np.ascontiguousarray(V), w


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


def _check_stride(stride, who):
    if int(stride) != stride or stride < 1:
        raise RuntimeError('%s: stride = %r, need an integer stride >= 1' % (who, stride))


def _mat(v):
    a = np.empty((1, 1), dtype=object)
    a[0, 0] = np.asarray(v)
    return a


class SSMFitResult:
    """samples (S), ridge and the one-step residuals of the three fits from the sums, each sqrt((Q - 2 tr(X R^T) + tr(X G_S X^T)) / (S rows)):
    residual_rms_d of x_{i+1} - rd_coeff phi - Bd u, residual_rms_c of the central difference - r_coeff phi - B u, residual_rms_w of
    (y - y_ref) - w_coeff phi.  The three terms cancel: of an exact fit about sqrt(eps) of the target's rms survives, and a figure
    clipped to 0 says no more than that.  residual_floor (d, c, w) = sqrt(eps Q / (S rows)) is that resolution: read a figure below its
    floor as "at most the floor" (one_step_error measures the discrete map's residual directly)."""

    def __init__(self, samples, ridge, residual_rms_d, residual_rms_c, residual_rms_w, residual_floor=(0.0, 0.0, 0.0)):
        self.samples, self.ridge = samples, ridge
        self.residual_rms_d, self.residual_rms_c, self.residual_rms_w = residual_rms_d, residual_rms_c, residual_rms_w
        self.residual_floor = tuple(residual_floor)

    def __repr__(self):
        return 'SSMFitResult(samples=%d, ridge=%g, residual_rms_d=%g, residual_rms_c=%g, residual_rms_w=%g, residual_floor=(%g, %g, %g))' % (
            (self.samples, self.ridge, self.residual_rms_d, self.residual_rms_c, self.residual_rms_w) + self.residual_floor)


class SSMSysID:
    """Accumulates the sums of the fit over any number of `add` calls and solves for the model (the module's docstring states the fit).
    Give V (n_y x n_x), or chart='pca': the first `add` then fixes V from its own records.  y_ref defaults to zeros."""

    def __init__(self, n_y, m, Ts, state_dim, ROM_order, SSM_order, V=None, y_ref=None, chart=None):
        self.n_y, self.m, self.Ts, self.n_x = int(n_y), int(m), float(Ts), int(state_dim)
        self.ROM_order, self.SSM_order = int(ROM_order), int(SSM_order)
        if not self.Ts > 0 or not np.isfinite(self.Ts):
            raise RuntimeError('SSMSysID: need a finite Ts > 0, got %r' % (Ts,))
        plan = fit_plan(self.n_x, self.n_y, self.m, self.ROM_order, self.SSM_order)      # refuses n > 128 and the other limits, on the host
        self.n_mon, self.n, self.rows_per_chunk = plan['n_mon'], plan['n'], plan['rows_per_chunk']
        L = _bind()
        self.n_rom = L.sssm_num_monomials(self.n_x, self.ROM_order)
        self.n_ssm = L.sssm_num_monomials(self.n_x, self.SSM_order)
        if (V is None) == (chart is None):
            raise RuntimeError("SSMSysID: give either the chart V (n_y x n_x) or chart='pca'")
        if chart is not None and chart != 'pca':
            raise RuntimeError("SSMSysID: chart = %r, the only computed chart is 'pca' (a polynomial chart is not offered)" % (chart,))
        self.chart = chart
        self.V = None if V is None else self._check_V(V)
        self.y_ref = np.zeros(self.n_y) if y_ref is None else np.ravel(np.asarray(y_ref, dtype=np.float64)).copy()
        if self.y_ref.shape != (self.n_y,) or not np.all(np.isfinite(self.y_ref)):
            raise RuntimeError('SSMSysID: y_ref must hold n_y = %d finite entries, got shape %r' % (self.n_y, tuple(np.shape(y_ref))))
        self.cov, self.cov_eigenvalues = None, None
        self._h, self._samples = C.c_void_p(), 0

    def _check_V(self, V):
        V = np.asarray(V, dtype=np.float64)
        if V.shape != (self.n_y, self.n_x):
            raise RuntimeError('SSMSysID: V must have shape (n_y, n_x) = (%d, %d), got %r' % (self.n_y, self.n_x, tuple(V.shape)))
        if not np.all(np.isfinite(V)):
            raise RuntimeError('SSMSysID: V holds a non-finite entry')
        return np.ascontiguousarray(V)

    @property
    def samples(self):
        return self._samples

    def _ensure(self):
        if not self._h:
            _lib.check(_bind().sssm_fit_create(C.byref(self._h), self.n_x, self.n_y, self.m, self.ROM_order, self.SSM_order, self.Ts,
                                               _lib.dptr(self.V), _lib.dptr(self.y_ref)), 'sssm_fit_create')

    def covariance(self, Y, stride=1, shape=None, stream=None):
        """(C (n_y x n_y), rows) of sum (y - y_ref)(y - y_ref)^T over the kept rows of the records, on the device."""
        _check_stride(stride, 'SSMSysID.covariance')
        if isinstance(Y, _lib.DeviceBuffer):
            if shape is None or len(tuple(shape)) != 2 or Y.nbytes < 8 * int(shape[0]) * int(shape[1]) * self.n_y:
                raise RuntimeError('SSMSysID.covariance: DeviceBuffer records need shape = (E, T) within the buffer')
            E, T, dev = int(shape[0]), int(shape[1]), True
        else:
            Y = _lib.f64(np.asarray(Y, dtype=np.float64).reshape((-1,) + np.shape(Y)[-2:]))
            if Y.shape[2] != self.n_y:
                raise RuntimeError('SSMSysID.covariance: Y must have n_y = %d columns, got %d' % (self.n_y, Y.shape[2]))
            E, T, dev = Y.shape[0], Y.shape[1], False
        Cm, cnt, L = np.zeros((self.n_y, self.n_y)), C.c_int64(0), _bind()
        if dev:
            _lib.check(L.sssm_fit_cov_dev(Y.ptr, E, T, self.n_y, int(stride), _lib.dptr(self.y_ref), _lib.dptr(Cm), C.byref(cnt), stream),
                       'sssm_fit_cov_dev')
        else:
            _lib.check(L.sssm_fit_cov(_lib.dptr(Y), E, T, self.n_y, int(stride), _lib.dptr(self.y_ref), _lib.dptr(Cm), C.byref(cnt)),
                       'sssm_fit_cov')
        return Cm, cnt.value

    def add(self, Y, U, stride=1, shape=None, stream=None):
        """Adds records to the sums: Y (E, T, n_y) or (T, n_y) and U alike, numpy arrays or _lib.DeviceBuffers with shape = (E, T)
        (device records are read in place, asynchronously on `stream`).  Returns the samples added."""
        _check_stride(stride, 'SSMSysID.add')
        Y, U, E, T, dev = _records(Y, U, self.n_y, self.m, shape, 'SSMSysID.add')
        if self.V is None:
            self.cov, _ = self.covariance(Y, stride=stride, shape=(E, T), stream=stream)
            if not np.all(np.isfinite(self.cov)):
                raise RuntimeError("SSMSysID.add: chart='pca': the covariance of the records holds a non-finite entry")
            self.V, self.cov_eigenvalues = pca_chart(self.cov, self.n_x)
        self._ensure()
        L = _bind()
        if dev:
            _lib.check(L.sssm_fit_add_dev(self._h, Y.ptr, U.ptr, E, T, int(stride), stream), 'sssm_fit_add_dev')
        else:
            _lib.check(L.sssm_fit_add(self._h, _lib.dptr(Y), _lib.dptr(U), E, T, int(stride)), 'sssm_fit_add')
        added = E * max(0, (T - 1) // int(stride) + 1 - 2)
        self._samples += added
        return added

    def sums(self):
        """{'G' (n x n), 'Rd' (n_x x n), 'Rc' (n_x x n), 'Rw' (n_y x n_mon), 'Q' (3), 'samples'} as accumulated so far (synchronises)."""
        G, Rd, Rc = np.zeros((self.n, self.n)), np.zeros((self.n_x, self.n)), np.zeros((self.n_x, self.n))
        Rw, Q, S = np.zeros((self.n_y, self.n_mon)), np.zeros(3), C.c_int64(0)
        if self._h:
            _lib.check(_bind().sssm_fit_sums(self._h, _lib.dptr(G), _lib.dptr(Rd), _lib.dptr(Rc), _lib.dptr(Rw), _lib.dptr(Q), C.byref(S)),
                       'sssm_fit_sums')
            assert S.value == self._samples
        return {'G': G, 'Rd': Rd, 'Rc': Rc, 'Rw': Rw, 'Q': Q, 'samples': S.value}

    def solve_coeffs(self, ridge=0.0):
        """{'rd_coeff', 'Bd', 'r_coeff', 'B', 'w_coeff'} by the device's equilibrated Cholesky; raises (code SRH_ENUMERIC) on a failing pivot."""
        if not (ridge >= 0.0 and np.isfinite(ridge)):
            raise RuntimeError('SSMSysID.solve: need a finite ridge >= 0, got %r' % (ridge,))
        if self._samples == 0:
            raise RuntimeError('SSMSysID.solve: no samples have been added (S = 0)')
        out = dict(rd_coeff=np.zeros((self.n_x, self.n_rom)), Bd=np.zeros((self.n_x, self.m)), r_coeff=np.zeros((self.n_x, self.n_rom)),
                   B=np.zeros((self.n_x, self.m)), w_coeff=np.zeros((self.n_y, self.n_ssm)))
        info = np.full(2, -1, dtype=np.int32)
        rc = _bind().sssm_fit_solve(self._h, float(ridge), *[_lib.dptr(out[k]) for k in ('rd_coeff', 'Bd', 'r_coeff', 'B', 'w_coeff')],
                                    _lib.iptr(info))
        self.last_info = (int(info[0]), int(info[1]))
        _lib.check(rc, 'sssm_fit_solve')
        return out

    def dictionaries(self, coeffs):
        """(model, params) in the loadmat layout SSM.__init__ reads; v_coeff = [V^T | 0] over the basis of n_y variables.  Refused when
        n_y != n_x: SSM reads w_coeff over the basis of output_dim variables, which the fitted n_y x nmon(n_x, SSM_order) array is not
        (solve_coeffs returns the coefficients of such a fit)."""
        if self.n_y != self.n_x:
            raise RuntimeError('SSMSysID.solve: n_y = %d != n_x = %d: SSM.__init__ reads w_coeff as n_y x nmon(n_y, SSM_order), the fit has '
                               'n_y x nmon(n_x, SSM_order) = %d x %d; the dictionaries are made for n_y = n_x only (solve_coeffs returns the '
                               'coefficients)' % (self.n_y, self.n_x, self.n_y, self.n_ssm))
        n_v = _bind().sssm_num_monomials(self.n_y, self.SSM_order)
        v_coeff = np.zeros((self.n_x, n_v))
        v_coeff[:, :self.n_y] = self.V.T
        sc = lambda v: _mat(np.array([[v]]))
        model = dict(Ts=sc(self.Ts), v_coeff=_mat(v_coeff), **{k: _mat(v) for k, v in coeffs.items()})
        params = dict(state_dim=sc(self.n_x), input_dim=sc(self.m), output_dim=sc(self.n_y), SSM_order=sc(self.SSM_order),
                      ROM_order=sc(self.ROM_order))
        return model, params

    def result(self, coeffs, ridge):
        s = self.sums()
        cols = list(range(self.n_rom)) + list(range(self.n_mon, self.n))
        Gd, Gw = s['G'][np.ix_(cols, cols)], s['G'][:self.n_ssm, :self.n_ssm]
        rms = [residual_rms(s['Q'][0], np.hstack([coeffs['rd_coeff'], coeffs['Bd']]), s['Rd'][:, cols], Gd, s['samples']),
               residual_rms(s['Q'][1], np.hstack([coeffs['r_coeff'], coeffs['B']]), s['Rc'][:, cols], Gd, s['samples']),
               residual_rms(s['Q'][2], coeffs['w_coeff'], s['Rw'][:, :self.n_ssm], Gw, s['samples'])]
        floors = [float(np.sqrt(2.0 ** -53 * max(q, 0.0) / (max(1, s['samples']) * rows))) for q, rows in zip(s['Q'], (self.n_x, self.n_x, self.n_y))]
        return SSMFitResult(s['samples'], float(ridge), *rms, residual_floor=tuple(floors))

    def solve(self, ridge=0.0):
        """(model, params, SSMFitResult): the dictionaries SSMDynamics(y_ref, model=model, params=params) takes, and the fit's figures.
        For n_y = n_x; a fit with n_y != n_x is refused before the device solves (solve_coeffs and result serve it)."""
        if self.n_y != self.n_x:
            self.dictionaries(None)
        coeffs = self.solve_coeffs(ridge)
        model, params = self.dictionaries(coeffs)
        return model, params, self.result(coeffs, ridge)

    def reset(self):
        """Sums and samples back to zero; the chart stays."""
        if self._h:
            _lib.check(_bind().sssm_fit_reset(self._h), 'sssm_fit_reset')
        self._samples = 0

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                _lib.lib().sssm_fit_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def residual_rms(Q, X, R, G, samples):
    """sqrt((Q - 2 tr(X R^T) + tr(X G X^T)) / (S rows)), clipped at 0."""
    r2 = Q - 2.0 * np.sum(X * R) + np.sum((X @ G) * X)
    return float(np.sqrt(max(r2, 0.0) / (max(1, samples) * X.shape[0])))


def fit_ssm(Y, U, Ts, state_dim, ROM_order, SSM_order, V=None, y_ref=None, chart=None, stride=1, ridge=0.0, shape=None, n_y=None, m=None):
    """The one-call form: records -> (model, params, SSMFitResult).  Arrays give n_y and m by their last axis; DeviceBuffers need
    shape = (E, T), n_y and m."""
    if not isinstance(Y, _lib.DeviceBuffer):
        n_y, m = np.shape(Y)[-1], np.shape(U)[-1]
    elif n_y is None or m is None:
        raise RuntimeError('fit_ssm: DeviceBuffer records need n_y and m')
    sid = SSMSysID(n_y, m, Ts, state_dim, ROM_order, SSM_order, V=V, y_ref=y_ref, chart=chart)
    sid.add(Y, U, stride=stride, shape=shape)
    return sid.solve(ridge)


def one_step_error(model, Y, U, y_ref=None, stride=1, worst=False):
    """rms over samples and states of x_{i+1} - rd_coeff phi(x_i) - Bd u_i on held-out records (arrays (E, T, n_y) / (T, n_y)), the
    samples as the fit defines them (interior rows), x_i = V^T (y_i - y_ref) with V read from the model's v_coeff; on the host.
    worst=True: the largest 2-norm of a sample's error instead of the rms."""
    _check_stride(stride, 'one_step_error')
    get = lambda k: np.asarray(model[k][0, 0], dtype=np.float64)
    rd, Bd, vc = get('rd_coeff'), get('Bd'), get('v_coeff')
    n_x, m = rd.shape[0], Bd.shape[1]
    Y, U, E, T, _ = _records(Y, U, np.shape(Y)[-1], m, None, 'one_step_error')
    n_y = Y.shape[2]
    order = next((o for o in range(1, 8) if _bind().sssm_num_monomials(n_x, o) == rd.shape[1]), None)
    if order is None or vc.shape[1] < n_y:
        raise RuntimeError('one_step_error: rd_coeff (%r) / v_coeff (%r) do not match a basis of n_x = %d variables and n_y = %d' %
                           (rd.shape, vc.shape, n_x, n_y))
    Ex = exponents(n_x, order)
    ref = np.zeros(n_y) if y_ref is None else np.ravel(y_ref)
    tot, cnt, big = 0.0, 0, 0.0
    for e in range(E):
        x = (Y[e, ::stride] - ref) @ vc[:, :n_y].T
        if x.shape[0] < 3:
            continue
        xi = x[1:-1]
        phi = np.prod(xi[:, None, :] ** Ex[None], axis=2)
        err = x[2:] - phi @ rd.T - U[e, ::stride][1:-1] @ Bd.T
        tot += float(np.sum(err * err))
        cnt += err.size
        big = max(big, float(np.sqrt((err * err).sum(axis=1)).max()))
    if cnt == 0:
        raise RuntimeError('one_step_error: the records hold no sample')
    return big if worst else float(np.sqrt(tot / cnt))


def _horizon_model(model, who):
    """(n_x, m, n_o, ROM_order, SSM_order, mode, has_discrete) of an SSM model; the mode is model._mode() (the continuous mode does not
    occur there: an unknown discr_method raises by name)."""
    for name in ('state_dim', 'input_dim', 'output_dim', 'ROM_order', 'SSM_order', '_mode'):
        if not hasattr(model, name):
            raise RuntimeError('%s: the model must be an SSMDynamics (it has no %s)' % (who, name))
    has_d = getattr(model, 'rd_coeff', None) is not None and getattr(model, 'Bd_r', None) is not None
    return (int(model.state_dim), int(model.input_dim), int(model.output_dim), int(model.ROM_order), int(model.SSM_order), int(model._mode()),
            bool(has_d))


def _horizon_ints(horizon, stride, every, who):
    _check_stride(stride, who)
    for name, val in (('horizon', horizon), ('every', every)):
        if int(val) != val or val < 1:
            raise RuntimeError('%s: %s = %r, need an integer %s >= 1' % (who, name, val, name))
    return int(horizon), int(stride), int(every)


def horizon_plan(model, E, T, horizon, stride=1, every=1, n_y=None):
    """sssm_horizon_plan, on the host (no GPU), for horizon_error(model, records of E episodes of T rows of n_y columns (default: the
    model's n_o), horizon, stride=, every=): {'windows', 'block' (windows of a workgroup), 'blocks', 'lds_bytes', 'launches',
    'pred_cap_bytes' (the most that x_pred + z_pred + x_obs of predictions=True may need)}; raises when the call would be refused."""
    who = 'horizon_plan'
    n_x, m, n_o, ro, so, mode, has_d = _horizon_model(model, who)
    H, stride, every = _horizon_ints(horizon, stride, every, who)
    w, bl, nb, lds, ln, cap = C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_bind().sssm_horizon_plan(n_x, m, n_o, n_o if n_y is None else int(n_y), ro, so, mode, int(has_d), int(E), int(T), H, stride, every,
                                         C.byref(w), C.byref(bl), C.byref(nb), C.byref(lds), C.byref(ln), C.byref(cap)), 'sssm_horizon_plan')
    return {'windows': int(w.value), 'block': bl.value, 'blocks': int(nb.value), 'lds_bytes': int(lds.value), 'launches': int(ln.value),
            'pred_cap_bytes': int(cap.value)}


class SSMHorizonError:
    """The result of horizon_error (the module's docstring defines every field): horizon, dt, windows, diverged, bad_rows; for
    k = 0 .. H: sse_x, rms_x, worst_x (H + 1,), worst_x_at (H + 1, 2) = (episode, unstrided row) of the worst window's start, and the same
    with z; on request final_x, final_z, status (W,), x_pred (W, H + 1, n_x), z_pred (W, H + 1, n_o) and x_obs (E, T', n_x)."""

    def __init__(self, horizon, dt, windows, diverged, bad_rows, sse_x, rms_x, worst_x, worst_x_at, sse_z, rms_z, worst_z, worst_z_at,
                 final_x=None, final_z=None, status=None, x_pred=None, z_pred=None, x_obs=None):
        self.horizon, self.dt, self.windows, self.diverged, self.bad_rows = horizon, dt, windows, diverged, bad_rows
        self.sse_x, self.rms_x, self.worst_x, self.worst_x_at = sse_x, rms_x, worst_x, worst_x_at
        self.sse_z, self.rms_z, self.worst_z, self.worst_z_at = sse_z, rms_z, worst_z, worst_z_at
        self.final_x, self.final_z, self.status = final_x, final_z, status
        self.x_pred, self.z_pred, self.x_obs = x_pred, z_pred, x_obs

    @property
    def windows_ok(self):
        return self.windows - self.diverged - self.bad_rows

    def __repr__(self):
        return 'SSMHorizonError(H=%d, %d windows (%d diverged, %d with bad rows), rms_x[H]=%g, rms_z[0]=%g, rms_z[H]=%g)' % (
            self.horizon, self.windows, self.diverged, self.bad_rows, self.rms_x[-1], self.rms_z[0], self.rms_z[-1])


def horizon_error(model, Y, U, horizon, dt=None, stride=1, every=1, shape=None, x_start=None, per_window=False, predictions=False):
    """The k-step open-loop prediction error of an SSM model over records, k = 0 .. horizon, from every window start (the module's
    docstring states the definition): an SSMHorizonError.  Y (E, T, n_y) or (T, n_y) and U alike, numpy arrays or _lib.DeviceBuffers
    with shape = (E, T) (read in place); dt defaults to float(model.Ts); x_start (n_x,) starts every window there instead of at the
    observed state."""
    who = 'horizon_error'
    n_x, m, n_o, ro, so, mode, has_d = _horizon_model(model, who)
    H, stride, every = _horizon_ints(horizon, stride, every, who)
    n_y = n_o if isinstance(Y, _lib.DeviceBuffer) else int(np.shape(Y)[-1])
    if n_x != n_o or n_y != n_o:                                # (before the records are shaped by n_y)
        horizon_plan(model, 1, H + 1, H, n_y=n_y)
    Y, U, E, T, dev = _records(Y, U, n_y, m, shape, who)
    plan = horizon_plan(model, E, T, H, stride, every, n_y=n_y)  # every refusal of the shapes, on the host
    W, Tk = plan['windows'], (T - 1) // stride + 1
    need = 8 * (W * (H + 1) * (n_x + n_o) + E * Tk * n_x)
    if predictions and need > plan['pred_cap_bytes']:
        raise RuntimeError('%s: x_pred, z_pred and x_obs of %d windows x %d rows and %d kept rows need %d bytes, above the cap of %d bytes'
                           % (who, W, H + 1, E * Tk, need, plan['pred_cap_bytes']))
    dt = float(model.Ts) if dt is None else float(dt)
    if not (dt > 0.0 and np.isfinite(dt)):
        raise RuntimeError('%s: dt = %r, need a finite dt > 0' % (who, dt))
    if x_start is not None:
        x_start = _lib.f64(np.ravel(np.asarray(x_start, dtype=np.float64)))
        if x_start.shape != (n_x,):
            raise RuntimeError('%s: x_start must hold n_x = %d entries, got %d' % (who, n_x, x_start.size))
    sse, worst = np.zeros((2, H + 1)), np.zeros((2, H + 1))
    at, counts = np.zeros((2, H + 1, 2), dtype=np.int64), np.zeros(3, dtype=np.int64)
    fin = np.zeros((2, W)) if per_window else None
    status = np.zeros(W, dtype=np.int32) if per_window else None
    xp = np.zeros((W, H + 1, n_x)) if predictions else None
    zp = np.zeros((W, H + 1, n_o)) if predictions else None
    xo = np.zeros((E, Tk, n_x)) if predictions else None
    i64p = C.POINTER(C.c_int64)
    opt = lambda a: None if a is None else _lib.dptr(a)
    args = [n_y, E, T, H, stride, every, opt(x_start), _lib.dptr(sse), _lib.dptr(worst), at.ctypes.data_as(i64p), counts.ctypes.data_as(i64p),
            opt(fin), _lib.iptr(status) if per_window else None, opt(xp), opt(zp), opt(xo)]
    L = _bind()
    if dev:
        _lib.check(L.sssm_horizon_error_dev(model.handle, mode, dt, Y.ptr, U.ptr, *args, None), 'sssm_horizon_error_dev')
    else:
        _lib.check(L.sssm_horizon_error(model.handle, mode, dt, _lib.dptr(Y), _lib.dptr(U), *args), 'sssm_horizon_error')
    ok = int(counts[0] - counts[1] - counts[2])

    def rms(s, dim):
        return np.sqrt(s / (ok * dim)) if ok > 0 else np.full(H + 1, np.nan)

    def none(a):                                                # no status-0 window: no maximum
        return np.where(a < 0, np.nan, a)

    out = SSMHorizonError(H, dt, int(counts[0]), int(counts[1]), int(counts[2]), sse[0].copy(), rms(sse[0], n_x), none(worst[0]), at[0].copy(),
                          sse[1].copy(), rms(sse[1], n_o), none(worst[1]), at[1].copy())
    if per_window:
        out.final_x, out.final_z, out.status = fin[0].copy(), fin[1].copy(), status
    out.x_pred, out.z_pred, out.x_obs = xp, zp, xo
    return out
