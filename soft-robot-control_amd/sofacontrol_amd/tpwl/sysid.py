"""TPWL model identification on the device: records (x, u) of the reduced state and P linearisation points -> a TPWLATV that the
planners, observers and closed loops accept unchanged (csrc/tpwl_fit.hip; C ABI: stpwl_fit_* in include/sofacontrol_hip.h).

THE FIT.  The reference builds its tables from the simulator's Jacobians (tpwl_utils.TPWLSnapshotData.add_point); this text defines
the fit from records.
  Records: E episodes, each X (T x n_x) of reduced states x = [v; q], n_x = 2 r, and U (T x m).  Row i holds the input applied after
  x_i.  `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode: a record at dt_sim becomes one at Ts = s dt_sim.  T' = rows kept.
  Samples: the kept rows i <= T' - 2, those with a kept successor in the same episode; an episode with one kept row contributes
  nothing; no sample pairs across episodes.
  Points: P points (q_p, v_p) and dist_weights = {q, v}; x_p = [v_p; q_p].
  Assignment: p(i) = the nearest point to x_i by the point-search rule every TPWL kernel uses (calc_nearest_point: the first
  minimum of w_q |q_p - q| + w_v |v_p - v|).
  Regressor phi_i = [x_i - x_p; u_i; 1], n = n_x + m + 1.  Target g_i = (x_{i+1} - x_i) / Ts over kept rows: the forward difference, so
  the fitted model is the one whose 'fe' discretisation at Ts reproduces the one-step map.
  Sums per point over its samples: G_p = sum phi phi^T, R_p = sum g phi^T, Q_p = sum |g|^2, S_p = the samples.
  Solve per point: [A_c | B_c | c] = R_p (G_p + ridge diag)^-1 after equilibration: with D = diag(G_p),
  (D^-1/2 G_p D^-1/2 + ridge I) z = D^-1/2 r, coefficients = D^-1/2 z; the scaled block's diagonal is 1 + ridge exactly; a pivot must
  exceed n eps (1 + ridge).  d_c[p] = c - A_c[p] x_p, so that xdot = A_c[p] x + B_c[p] u + d_c[p]; u[p] = the mean input of the point's
  samples.
  Status per point: 0 solved; 1 S_p < min_samples (default n + 1; a duplicated point falls here: the first-minimum rule gives the later
  duplicate no samples); 2 a failing pivot, with its column named ('state x7', 'input u2', 'constant').
  A kept row that is not finite is refused at `add` with its episode and row; the sums stay untouched.
  Bits: the same sequence of `add` calls gives the same bits, and device-resident records give the bits of host arrays.  Two `add`
  calls do NOT give the bits of one: the samples are ordered by region per call, so the chains of additions differ (both meet the
  same error bound).
  Limits: n = n_x + m + 1 <= 128 (the accumulate kernel then keeps 36 + 64 tiles, 25 per wave, in registers), m <= 16, P <= 1024.

THE POINTS.  The fit takes the caller's points.  Two functions choose them from the records.
  points_by_distance: the reference's distance rule (tpwl_utils.TPWLSnapshotData.evaluate_point, eval_type = 'distance') as a greedy scan
  on the device (csrc/tpwl_select.hip; C ABI: stpwl_select_points).  The candidates are ALL kept rows of every episode (the last kept row
  too), scanned episode by episode in row order; the table starts as the optional seed (q0, v0); with an empty table the first candidate
  is taken unconditionally.  For a candidate c and a point p, dq = w_q |q_p - q_c| and dv = w_v |v_p - v_c| in the arithmetic of the
  point-search rule (with w_v == 0 the velocity is not read, dv = 0).  separate=False: c is taken iff dq + dv >= threshold for EVERY point
  of the table; separate=True: iff dq >= threshold for every point, or dv >= threshold for every point.  A taken candidate joins the table
  before the next one is examined.  max_points counts the seed plus the taken points (max(P0, 1) <= max_points <= 1024); when a candidate
  would become point max_points + 1 the scan stops there (complete = False, stopped_at = its episode and row).  The number of points
  follows the spread of the data, every point is a visited state, and every kept row lies within the threshold of some point.  Scanning
  X1 and then X2 with the first result as the seed gives exactly the result of scanning their concatenation.
  points_from_records: the k-means centroids of the kept states (k is the caller's; a centroid is an average, not a visited state).

THE HORIZON ERROR.  horizon_error judges a model the way the planners use it: rolled out open loop over H steps from every window start
of held-out records, read in place on the device (csrc/tpwl_horizon.hip; C ABI: stpwl_horizon_error; the reference's model check,
examples/hardware/diamond.py TPWL_rollout, for every window at once).
  Records as the fit defines them (X (E, T, n_x), U (E, T, m), row i holds the input applied after x_i; `stride` keeps rows 0, s, 2s, ..,
  T' kept rows; arrays, or DeviceBuffers with shape = (E, T)).
  Model: a nearest-point TPWLATV and a step dt, defaulting to model.fit_Ts; the tables are those of model.handle_for(dt) in the model's
  own discretisation method.  A weighting-mode model is refused by name.
  Windows: starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, numbered episode by
  episode in row order; an episode with T' <= H has none; W = 0 raises.
  Prediction of a window: xh_0 = x_{j0}; xh_{k+1} = the step rule of csrc/tpwl_dev.h applied to (xh_k, u_{j0+k}) with the point search of
  the same file, k = 0 .. H - 1: exactly model.rollout(x_{j0}, U[j0:j0+H], dt), bit for bit.
  Errors: e_k = xh_k - x_{j0+k}; with an output model ez_k = H e_k (z_ref cancels).
  Window status: 0 ok; 1 some xh_k is not finite; 2 some record row the window reads (a state j0 .. j0 + H or an input j0 .. j0 + H - 1)
  is not finite; status 2 wins over 1.  Only status-0 windows enter the sums.
  Results for k = 0 .. H: sse_x[k] = sum_w |e_k|^2 and sse_z[k]; rms_x[k] = sqrt(sse_x[k] / (W_ok n_x)), rms_z with n_z; worst_x[k] =
  max_w |e_k|_2 with worst_x_at[k] = (episode, unstrided row) of that window's start, ties to the lowest window number, the same for z;
  the counts windows, diverged (status 1) and bad_rows (status 2).  Row 0 of every curve is exactly 0.
  On request: per_window=True gives final_x (W,), final_z (W,) (the norms at k = H, NaN where status != 0) and status (W,);
  predictions=True gives x_pred (W, H + 1, n_x), refused above the byte cap that horizon_plan states (tests and small studies; the rows
  behind the one at which a window left its loop are NaN).
  Bits: no floating-point atomics; the windows are dealt to workgroups in fixed blocks by window number and the blocks' partial sums are
  joined in block order, so the result is a function of the records and parameters alone: not of the CU count, a rerun gives the same
  bits, and device records give the bits of host arrays.  max is exact; its tie rule is the lowest window number.
  Limits: n_x <= 128, m <= 16, H <= 1024, each refused on the host with the offending number.
  Not offered here: the Koopman and SSM analogues, weighting-mode models, closed-loop (feedback) prediction, error weights other than the
  model's H.  one_step_error is unchanged.

NOT OFFERED: weighting-mode fits; sample weights; the reference's 'dynamics' rule of selection (it needs the simulator's Jacobians at the
candidate); full-order records (project them first: POD.compute_RO_state)."""
import ctypes as C

import numpy as np

from .. import _lib
from .. import utils as scutils
from .tpwl import TPWLATV

_BOUND = False
MAX_N = 128


def _bind():
    global _BOUND
    L = _lib.lib()
    if _BOUND:
        return L
    vp, dp, i64, ip, i32p = C.c_void_p, _lib.c_double_p, C.c_int64, C.POINTER(C.c_int), _lib.c_int32_p
    L.stpwl_fit_plan.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.POINTER(i64)]
    L.stpwl_fit_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_double]
    L.stpwl_fit_destroy.argtypes = [vp]
    L.stpwl_fit_reset.argtypes = [vp]
    L.stpwl_fit_add.argtypes = [vp, dp, dp, i64, i64, C.c_int]
    L.stpwl_fit_add_dev.argtypes = [vp, vp, vp, i64, i64, C.c_int, vp]
    L.stpwl_fit_counts.argtypes = [vp, C.POINTER(i64)]
    L.stpwl_fit_sums.argtypes = [vp, C.c_int, dp, dp, dp, C.POINTER(i64)]
    L.stpwl_fit_solve.argtypes = [vp, C.c_double, i64, dp, dp, dp, dp, i32p, i32p]
    i64p, dbl = C.POINTER(i64), C.c_double
    sel = [i64, i64, C.c_int, C.c_int, dbl, dbl, dbl, C.c_int, C.c_int, dp, dp, C.c_int, ip, i64p, dp, dp, dp, ip, i64p]
    L.stpwl_select_plan.argtypes = [C.c_int, i64, ip, i64p, i64p]
    L.stpwl_select_points.argtypes = [dp] + sel
    L.stpwl_select_points_dev.argtypes = [vp] + sel + [vp]
    hor = [i64, i64, C.c_int, C.c_int, C.c_int, dp, dp, i64p, i64p, dp, i32p, dp]
    L.stpwl_horizon_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dbl, i64, i64, C.c_int, C.c_int, C.c_int, i64p, ip, i64p, ip, i64p, i64p,
                                     i64p]
    L.stpwl_horizon_error.argtypes = [vp, dp, dp] + hor
    L.stpwl_horizon_error_dev.argtypes = [vp, vp, vp] + hor + [vp]
    _BOUND = True
    return L


def fit_plan(P, r, m):
    """stpwl_fit_plan, on the host (no GPU): {'n', 'rows_per_chunk', 'tiles_per_wave', 'lds_bytes'}; raises when the shape is refused."""
    a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    _lib.check(_bind().stpwl_fit_plan(int(P), int(r), int(m), C.byref(a), C.byref(b), C.byref(c), C.byref(d)), 'stpwl_fit_plan')
    return {'n': a.value, 'rows_per_chunk': b.value, 'tiles_per_wave': c.value, 'lds_bytes': int(d.value)}


def column_name(c, n_x, m):
    """'state x7', 'input u2' or 'constant': column c of phi (1-based within its group)."""
    if c < 0:
        return 'none'
    if c < n_x:
        return 'state x%d' % (c + 1)
    if c < n_x + m:
        return 'input u%d' % (c - n_x + 1)
    if c == n_x + m:
        return 'constant'
    return 'a non-finite solution'


def _records(X, U, n_x, m, shape, who):
    """(X, U, E, T, on_device) of records given as arrays ((E, T, n_x) / (T, n_x)) or DeviceBuffers with shape = (E, T)."""
    dev = isinstance(X, _lib.DeviceBuffer)
    if dev != isinstance(U, _lib.DeviceBuffer):
        raise RuntimeError('%s: X and U must both be arrays or both be DeviceBuffers' % who)
    if dev:
        if shape is None or len(tuple(shape)) != 2:
            raise RuntimeError('%s: DeviceBuffer records need shape = (E, T)' % who)
        E, T = int(shape[0]), int(shape[1])
        if E < 1 or T < 1 or X.nbytes < 8 * E * T * n_x or U.nbytes < 8 * E * T * m:
            raise RuntimeError('%s: the DeviceBuffers are smaller than (E, T, n_x) = (%d, %d, %d) and (E, T, m) = (%d, %d, %d) doubles'
                               % (who, E, T, n_x, E, T, m))
        return X, U, E, T, True
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    if X.ndim == 2:
        X = X[None]
    if U.ndim == 2:
        U = U[None]
    if X.ndim != 3 or X.shape[2] != n_x or X.shape[0] < 1 or X.shape[1] < 1:
        raise RuntimeError('%s: X must have shape (E, T, n_x) or (T, n_x) with n_x = %d, got %r' % (who, n_x, tuple(np.shape(X))))
    if U.shape != (X.shape[0], X.shape[1], m):
        raise RuntimeError('%s: U (E, T, m) must have shape %r, got %r' % (who, (X.shape[0], X.shape[1], m), tuple(U.shape)))
    return _lib.f64(X), _lib.f64(U), X.shape[0], X.shape[1], False


def _check_stride(stride, who):
    if int(stride) != stride or stride < 1:
        raise RuntimeError('%s: stride = %r, need an integer stride >= 1' % (who, stride))


class TPWLFitResult:
    """samples (the total), counts (P), status (P), column (P: the failing column of a status-2 point, else -1), ridge, and per point
    residual_rms = sqrt((Q - 2 tr(X R^T) + tr(X G X^T)) / (S n_x)), X = [A_c | B_c | c], from the sums (NaN of a point that did not
    solve).  The three terms cancel: of an exact fit about sqrt(eps) of the target's rms survives, and a figure clipped to 0 says no
    more than that.  residual_floor = sqrt(eps Q / (S n_x)) per point is that resolution: read a figure below its floor as "at most the
    floor" (one_step_error measures the one-step map's residual directly).  `kept` = the points of the model, as indices of the fit's."""

    def __init__(self, samples, counts, status, column, ridge, residual_rms, residual_floor, kept=None):
        self.samples, self.counts, self.status, self.column, self.ridge = samples, counts, status, column, ridge
        self.residual_rms, self.residual_floor, self.kept = residual_rms, residual_floor, kept

    def __repr__(self):
        ok = self.status == 0
        worst = float(np.nanmax(self.residual_rms[ok])) if np.any(ok) else float('nan')
        return 'TPWLFitResult(samples=%d, points=%d, solved=%d, ridge=%g, worst residual_rms=%g)' % (
            self.samples, len(self.counts), int(ok.sum()), self.ridge, worst)


class TPWLSysID:
    """Accumulates the per-point sums of the fit over any number of `add` calls and solves every point in one launch (the module's
    docstring states the fit).  q, v: (P, r); dist_weights = {'q': .., 'v': ..}."""

    def __init__(self, q, v, dist_weights, m, Ts):
        q, v = np.atleast_2d(np.asarray(q, dtype=np.float64)), np.atleast_2d(np.asarray(v, dtype=np.float64))
        if q.ndim != 2 or q.shape != v.shape or q.shape[0] < 1 or q.shape[1] < 1:
            raise RuntimeError('TPWLSysID: q and v must both have shape (P, r), got %r and %r' % (tuple(q.shape), tuple(v.shape)))
        if not (np.all(np.isfinite(q)) and np.all(np.isfinite(v))):
            raise RuntimeError('TPWLSysID: the points hold a non-finite entry')
        try:
            self.dist_weights = {'q': float(dist_weights['q']), 'v': float(dist_weights['v'])}
        except (TypeError, KeyError):
            raise RuntimeError("TPWLSysID: dist_weights must be {'q': .., 'v': ..}")
        self.q, self.v = np.ascontiguousarray(q), np.ascontiguousarray(v)
        self.P, self.r, self.n_x, self.m, self.Ts = q.shape[0], q.shape[1], 2 * q.shape[1], int(m), float(Ts)
        if not self.Ts > 0 or not np.isfinite(self.Ts):
            raise RuntimeError('TPWLSysID: need a finite Ts > 0, got %r' % (Ts,))
        plan = fit_plan(self.P, self.r, self.m)                 # refuses n > 128 and the other limits, on the host
        self.n, self.rows_per_chunk = plan['n'], plan['rows_per_chunk']
        self.x_points = scutils.qv2x(self.q, self.v)
        self._h, self._samples = C.c_void_p(), 0

    @property
    def samples(self):
        return self._samples

    def _ensure(self):
        if not self._h:
            _lib.check(_bind().stpwl_fit_create(C.byref(self._h), self.P, self.r, self.m, _lib.dptr(self.q), _lib.dptr(self.v),
                                                self.dist_weights['q'], self.dist_weights['v'], self.Ts), 'stpwl_fit_create')

    def add(self, X, U, stride=1, shape=None, stream=None):
        """Adds records to the sums: X (E, T, n_x) or (T, n_x) and U alike, numpy arrays or _lib.DeviceBuffers with shape = (E, T)
        (device records are read in place on `stream`, which is synchronised).  Returns the samples added."""
        _check_stride(stride, 'TPWLSysID.add')
        X, U, E, T, dev = _records(X, U, self.n_x, self.m, shape, 'TPWLSysID.add')
        self._ensure()
        L = _bind()
        if dev:
            _lib.check(L.stpwl_fit_add_dev(self._h, X.ptr, U.ptr, E, T, int(stride), stream), 'stpwl_fit_add_dev')
        else:
            _lib.check(L.stpwl_fit_add(self._h, _lib.dptr(X), _lib.dptr(U), E, T, int(stride)), 'stpwl_fit_add')
        added = E * ((T - 1) // int(stride))
        self._samples += added
        return added

    def counts(self):
        """(P,) the samples of every point."""
        out = np.zeros(self.P, dtype=np.int64)
        if self._h:
            _lib.check(_bind().stpwl_fit_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))), 'stpwl_fit_counts')
        return out

    def sums(self, p):
        """{'G' (n x n), 'R' (n_x x n), 'Q', 'samples'} of point p as accumulated so far (synchronises the device)."""
        p = int(p)
        if not 0 <= p < self.P:
            raise RuntimeError('TPWLSysID.sums: point %d is outside 0 .. %d' % (p, self.P - 1))
        G, R, Q, S = np.zeros((self.n, self.n)), np.zeros((self.n_x, self.n)), C.c_double(0.0), C.c_int64(0)
        if self._h:
            _lib.check(_bind().stpwl_fit_sums(self._h, p, _lib.dptr(G), _lib.dptr(R), C.cast(C.byref(Q), _lib.c_double_p), C.byref(S)),
                       'stpwl_fit_sums')
        return {'G': G, 'R': R, 'Q': Q.value, 'samples': S.value}

    def solve_tables(self, ridge=0.0, min_samples=None):
        """{'A_c' (P, n_x, n_x), 'B_c' (P, n_x, m), 'd_c' (P, n_x), 'u' (P, m), 'status' (P), 'column' (P)} by the device's solve; a point
        that does not solve is reported in status (its tables are zeros)."""
        if not (ridge >= 0.0 and np.isfinite(ridge)):
            raise RuntimeError('TPWLSysID.solve: need a finite ridge >= 0, got %r' % (ridge,))
        if min_samples is not None and (int(min_samples) != min_samples or min_samples < 1):
            raise RuntimeError('TPWLSysID.solve: min_samples = %r, need an integer >= 1 (default n + 1 = %d)' % (min_samples, self.n + 1))
        if self._samples == 0:
            raise RuntimeError('TPWLSysID.solve: no samples have been added (S = 0)')
        P, nx, m = self.P, self.n_x, self.m
        out = dict(A_c=np.zeros((P, nx, nx)), B_c=np.zeros((P, nx, m)), d_c=np.zeros((P, nx)), u=np.zeros((P, m)),
                   status=np.zeros(P, dtype=np.int32), column=np.zeros(P, dtype=np.int32))
        _lib.check(_bind().stpwl_fit_solve(self._h, float(ridge), -1 if min_samples is None else int(min_samples),
                                           *[_lib.dptr(out[k]) for k in ('A_c', 'B_c', 'd_c', 'u')], _lib.iptr(out['status']),
                                           _lib.iptr(out['column'])), 'stpwl_fit_solve')
        return out

    def result(self, tables, ridge=0.0, kept=None):
        """TPWLFitResult of solved tables: the residuals per point from the sums."""
        P, nx = self.P, self.n_x
        counts = self.counts()
        rms, floor = np.full(P, np.nan), np.full(P, np.nan)
        eps = np.finfo(np.float64).eps
        for p in np.flatnonzero(tables['status'] == 0):
            s = self.sums(p)
            c = tables['d_c'][p] + tables['A_c'][p] @ self.x_points[p]
            Xc = np.hstack([tables['A_c'][p], tables['B_c'][p], c[:, None]])
            r2 = s['Q'] - 2.0 * np.sum(Xc * s['R']) + np.sum((Xc @ s['G']) * Xc)
            rms[p] = np.sqrt(max(r2, 0.0) / (max(1, s['samples']) * nx))
            floor[p] = np.sqrt(eps * s['Q'] / (max(1, s['samples']) * nx))
        return TPWLFitResult(int(counts.sum()), counts, tables['status'].copy(), tables['column'].copy(), float(ridge), rms, floor, kept)

    def describe_failures(self, tables):
        """One line per point that did not solve."""
        counts, lines = self.counts(), []
        for p in np.flatnonzero(tables['status'] != 0):
            if tables['status'][p] == 1:
                lines.append('point %d: %d samples, fewer than min_samples' % (p, counts[p]))
            else:
                lines.append('point %d: failing pivot at %s (column %d of phi): increase ridge' % (
                    p, column_name(int(tables['column'][p]), self.n_x, self.m), tables['column'][p]))
        return lines

    def model(self, tables, rom_info, on_fail='raise', Cf=None, Hf=None):
        """(TPWLATV, kept) of solved tables; see solve."""
        if on_fail not in ('raise', 'drop'):
            raise RuntimeError("TPWLSysID.solve: on_fail = %r, need 'raise' or 'drop'" % (on_fail,))
        bad = self.describe_failures(tables)
        if bad and on_fail == 'raise':
            raise RuntimeError('TPWLSysID.solve: %d of %d points did not solve (on_fail=\'drop\' leaves them out): %s'
                               % (len(bad), self.P, '; '.join(bad)))
        kept = np.flatnonzero(tables['status'] == 0)
        if kept.size == 0:
            raise RuntimeError('TPWLSysID.solve: no point solved: %s' % '; '.join(bad))
        data = dict(q=self.q[kept].copy(), v=self.v[kept].copy(), u=tables['u'][kept].copy(), A_c=tables['A_c'][kept].copy(),
                    B_c=tables['B_c'][kept].copy(), d_c=tables['d_c'][kept].copy(), rom_info=rom_info)
        mdl = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights=dict(self.dist_weights)), Cf=Cf, Hf=Hf, discr_method='fe')
        mdl.fit_Ts = self.Ts
        return mdl, kept

    def solve(self, rom_info, ridge=0.0, min_samples=None, on_fail='raise', Cf=None, Hf=None):
        """The fitted TPWLATV (discr_method='fe', tpwl_method='nn', the fit's dist_weights).  on_fail='raise' names the points that did
        not solve; 'drop' leaves them out of the model (`last_result.kept` lists the points that stayed)."""
        if on_fail not in ('raise', 'drop'):
            raise RuntimeError("TPWLSysID.solve: on_fail = %r, need 'raise' or 'drop'" % (on_fail,))
        tables = self.solve_tables(ridge, min_samples)
        mdl, kept = self.model(tables, rom_info, on_fail, Cf, Hf)
        self.last_result = self.result(tables, ridge, kept)
        return mdl

    def reset(self):
        """Sums and counts back to zero; the points stay."""
        if self._h:
            _lib.check(_bind().stpwl_fit_reset(self._h), 'stpwl_fit_reset')
        self._samples = 0

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                _lib.lib().stpwl_fit_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def fit_tpwl(X, U, q, v, dist_weights, Ts, rom_info, stride=1, ridge=0.0, min_samples=None, on_fail='raise', shape=None, m=None, Cf=None,
             Hf=None):
    """The one-call form: records and points -> (TPWLATV, TPWLFitResult).  Arrays give m by U's last axis; DeviceBuffers need
    shape = (E, T) and m."""
    if not isinstance(U, _lib.DeviceBuffer):
        m = np.shape(U)[-1]
    elif m is None:
        raise RuntimeError('fit_tpwl: DeviceBuffer records need m')
    sid = TPWLSysID(q, v, dist_weights, m, Ts)
    sid.add(X, U, stride=stride, shape=shape)
    mdl = sid.solve(rom_info, ridge=ridge, min_samples=min_samples, on_fail=on_fail, Cf=Cf, Hf=Hf)
    return mdl, sid.last_result


def one_step_error(model, X, U, stride=1, worst=False, Ts=None):
    """The residual of the model's one-step map x_i + Ts (A_c[p] x_i + B_c[p] u_i + d_c[p]), p the model's nearest point to x_i, on
    held-out records (arrays (E, T, n_x) / (T, n_x)) over the samples the fit defines: the rms over samples and coordinates, or with
    worst=True the largest 2-norm over the samples.  Ts defaults to the fit's (model.fit_Ts)."""
    _check_stride(stride, 'one_step_error')
    Ts = getattr(model, 'fit_Ts', None) if Ts is None else Ts
    if Ts is None:
        raise RuntimeError('one_step_error: the model carries no fit_Ts; give Ts')
    X, U, E, T, _ = _records(X, U, model.get_state_dim(), model.get_input_dim(), None, 'one_step_error')
    Xk, Uk = X[:, ::stride], U[:, ::stride]
    if Xk.shape[1] < 2:
        raise RuntimeError('one_step_error: the records hold no sample')
    x0 = np.ascontiguousarray(Xk[:, :-1].reshape(-1, X.shape[2]))
    u0, x1 = Uk[:, :-1].reshape(-1, U.shape[2]), Xk[:, 1:].reshape(-1, X.shape[2])
    A, B, d, _ = model.linearize_batch(x0)
    err = x1 - (x0 + Ts * (np.einsum('bij,bj->bi', A, x0) + np.einsum('bij,bj->bi', B, u0) + d))
    if worst:
        return float(np.sqrt((err * err).sum(axis=1)).max())
    return float(np.sqrt(np.mean(err * err)))


def points_from_records(X, k, random_state=0, n_init=10, stride=1):
    """(q, v), each (k, r): the k-means centroids of the kept states of records X ((E, T, n_x) / (T, n_x)), by the device k-means
    (mor.pod.compute_kmeans_centroids), split with x2qv."""
    from ..mor import pod
    _check_stride(stride, 'points_from_records')
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[None]
    if X.ndim != 3 or X.shape[2] % 2:
        raise RuntimeError('points_from_records: X must have shape (E, T, n_x) or (T, n_x) with n_x even, got %r' % (tuple(X.shape),))
    S = np.ascontiguousarray(X[:, ::stride].reshape(-1, X.shape[2]))
    if not 1 <= int(k) <= S.shape[0]:
        raise RuntimeError('points_from_records: k = %r, need 1 <= k <= %d kept states' % (k, S.shape[0]))
    cent = np.asarray(pod.compute_kmeans_centroids(S, int(k), n_init=n_init, random_state=random_state))
    q, v = scutils.x2qv(cent)
    return np.ascontiguousarray(q), np.ascontiguousarray(v)


MAX_POINTS = 1024


def select_plan(r, candidates):
    """stpwl_select_plan, on the host (no GPU): {'chunk', 'lds_bytes', 'launches'} of a scan of `candidates` kept rows."""
    a, b, c = C.c_int(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_bind().stpwl_select_plan(int(r), int(candidates), C.byref(a), C.byref(b), C.byref(c)), 'stpwl_select_plan')
    return {'chunk': a.value, 'lds_bytes': int(b.value), 'launches': int(c.value)}


class TPWLPointSelection:
    """The result of points_by_distance: q, v (P, r), the seed first; index (P_taken, 2): episode and row in the UNstrided record of every
    taken point; dmin (P_taken,), or (P_taken, 2) = (min dq, min dv) when separate: the smallest distance to the table at the moment the
    point was taken (+inf for an unconditional first point); complete; stopped_at = (episode, row) of the candidate that met the cap, or
    None; candidates = the kept rows of the records (those behind stopped_at were not examined); seeded = the points of the seed."""

    def __init__(self, q, v, index, dmin, complete, stopped_at, candidates, seeded=0):
        self.q, self.v, self.index, self.dmin = q, v, index, dmin
        self.complete, self.stopped_at, self.candidates, self.seeded = complete, stopped_at, candidates, seeded

    def __repr__(self):
        tail = '' if self.complete else ', stopped at episode %d row %d' % tuple(self.stopped_at)
        return 'TPWLPointSelection(%d points (%d seeded) from %d candidates%s)' % (len(self.q), self.seeded, self.candidates, tail)


def points_by_distance(X, dist_weights, threshold, separate=False, stride=1, shape=None, q0=None, v0=None, max_points=MAX_POINTS, stream=None):
    """The linearisation points of records by the reference's distance rule (the module's docstring states it): a TPWLPointSelection.
    X: (E, T, n_x) or (T, n_x) array, or a _lib.DeviceBuffer with shape = (E, T) or (E, T, n_x) (read in place on `stream`, which is synchronised);
    dist_weights = {'q': .., 'v': ..}; q0, v0: an optional seed, (P0, r) each.  TPWLSysID(sel.q, sel.v, dist_weights, m, Ts) takes the
    result unchanged."""
    who = 'points_by_distance'
    _check_stride(stride, who)
    try:
        w_q, w_v = float(dist_weights['q']), float(dist_weights['v'])
    except (TypeError, KeyError):
        raise RuntimeError("%s: dist_weights must be {'q': .., 'v': ..}" % who)
    threshold = float(threshold)
    if not (np.isfinite(threshold) and threshold > 0):
        raise RuntimeError('%s: threshold = %r, need a finite threshold > 0' % (who, threshold))
    for name, w in (('q', w_q), ('v', w_v)):
        if not (np.isfinite(w) and w >= 0):
            raise RuntimeError("%s: the weight dist_weights['%s'] = %r is negative or not finite" % (who, name, w))
    if w_q == 0 and w_v == 0:
        raise RuntimeError('%s: both weights are zero' % who)
    dev = isinstance(X, _lib.DeviceBuffer)
    if dev:
        if shape is None or len(tuple(shape)) not in (2, 3):
            raise RuntimeError('%s: DeviceBuffer records need shape = (E, T) or (E, T, n_x)' % who)
        E, T = int(shape[0]), int(shape[1])
        if len(tuple(shape)) == 3:
            n_x = int(shape[2])
        else:                                                   # (E, T) as TPWLSysID.add takes it: the buffer's size gives n_x
            if E < 1 or T < 1 or X.nbytes % (8 * E * T):
                raise RuntimeError('%s: a DeviceBuffer of %d bytes is not (E, T, n_x) = (%d, %d, ..) doubles; give shape = (E, T, n_x)'
                                   % (who, X.nbytes, E, T))
            n_x = X.nbytes // (8 * E * T)
    else:
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 2:
            X = X[None]
        if X.ndim != 3:
            raise RuntimeError('%s: X must have shape (E, T, n_x) or (T, n_x), got %r' % (who, tuple(X.shape)))
        E, T, n_x = X.shape
    if n_x < 2 or n_x % 2:
        raise RuntimeError('%s: n_x = %d, need n_x = 2 r with r >= 1 (x = [v; q])' % (who, n_x))
    if E < 1 or T < 1:
        raise RuntimeError('%s: need E >= 1 episodes of T >= 1 rows, got E = %d, T = %d' % (who, E, T))
    r = n_x // 2
    if dev and X.nbytes < 8 * E * T * n_x:
        raise RuntimeError('%s: the DeviceBuffer is smaller than (E, T, n_x) = (%d, %d, %d) doubles' % (who, E, T, n_x))
    if (q0 is None) != (v0 is None):
        raise RuntimeError('%s: a seed needs both q0 and v0' % who)
    if q0 is None:
        q0, v0 = np.zeros((0, r)), np.zeros((0, r))
    q0, v0 = np.asarray(q0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    q0, v0 = q0.reshape(-1, r) if q0.size == 0 else np.atleast_2d(q0), v0.reshape(-1, r) if v0.size == 0 else np.atleast_2d(v0)
    if q0.ndim != 2 or q0.shape != v0.shape or q0.shape[1] != r:
        raise RuntimeError('%s: the seed q0 and v0 must both have shape (P0, r) with r = %d, got %r and %r'
                           % (who, r, tuple(q0.shape), tuple(v0.shape)))
    if not (np.all(np.isfinite(q0)) and np.all(np.isfinite(v0))):
        bad = int(np.flatnonzero(~(np.isfinite(q0).all(axis=1) & np.isfinite(v0).all(axis=1)))[0])
        raise RuntimeError('%s: seed point %d holds a non-finite entry' % (who, bad))
    P0 = q0.shape[0]
    if int(max_points) != max_points or not max(P0, 1) <= max_points <= MAX_POINTS:
        raise RuntimeError('%s: max_points = %r, need an integer with max(P0, 1) = %d <= max_points <= %d'
                           % (who, max_points, max(P0, 1), MAX_POINTS))
    max_points = int(max_points)
    if not dev:
        X = _lib.f64(X)
        ok = np.isfinite(X[:, ::int(stride)]).all(axis=2)
        if not ok.all():
            ep, i = np.argwhere(~ok)[0]
            raise RuntimeError('%s: episode %d, row %d of the records is not finite; nothing was selected' % (who, ep, i * int(stride)))
    q0, v0 = np.ascontiguousarray(q0), np.ascontiguousarray(v0)
    nt = max_points - P0
    count, status = C.c_int(0), C.c_int(0)
    index, stopped = np.zeros((nt, 2), dtype=np.int64), np.zeros(2, dtype=np.int64)
    q, v, dmin = np.zeros((nt, r)), np.zeros((nt, r)), np.zeros((nt, 2) if separate else (nt,))
    i64p = C.POINTER(C.c_int64)
    args = [E, T, r, int(stride), w_q, w_v, threshold, 1 if separate else 0, P0, _lib.dptr(q0) if P0 else None, _lib.dptr(v0) if P0 else None,
            max_points, C.byref(count), index.ctypes.data_as(i64p), _lib.dptr(q), _lib.dptr(v), _lib.dptr(dmin), C.byref(status),
            stopped.ctypes.data_as(i64p)]
    L = _bind()
    if dev:
        _lib.check(L.stpwl_select_points_dev(X.ptr, *args, stream), 'stpwl_select_points_dev')
    else:
        _lib.check(L.stpwl_select_points(_lib.dptr(X), *args), 'stpwl_select_points')
    n = count.value - P0
    return TPWLPointSelection(np.vstack([q0, q[:n]]), np.vstack([v0, v[:n]]), index[:n].copy(), dmin[:n].copy(), status.value == 0,
                              None if status.value == 0 else (int(stopped[0]), int(stopped[1])), E * ((T - 1) // int(stride) + 1), P0)


HORIZON_MODES = ('l2', 'staged', 'staged_held')


def _horizon_model(model, who):
    """(P, r, m, n_z, w_v) of a nearest-point model; a weighting-mode model is refused by name."""
    method = getattr(model, 'tpwl_method', None)
    if method != 'nn':
        raise RuntimeError("%s: tpwl_method = %r: only nearest-point ('nn') models are offered, not weighting-mode models" % (who, method))
    n_x, m = int(model.get_state_dim()), int(model.get_input_dim())
    if n_x < 2 or n_x % 2:
        raise RuntimeError('%s: n_x = %d, need n_x = 2 r with r >= 1 (x = [v; q])' % (who, n_x))
    n_z = int(model.get_output_dim()) if getattr(model, 'H', None) is not None else 0
    return int(model.num_points), n_x // 2, m, n_z, float(model.dist_weights['v'])


def _horizon_ints(horizon, stride, every, who):
    _check_stride(stride, who)
    for name, val in (('horizon', horizon), ('every', every)):
        if int(val) != val or val < 1:
            raise RuntimeError('%s: %s = %r, need an integer %s >= 1' % (who, name, val, name))
    return int(horizon), int(stride), int(every)


def horizon_plan(model, E, T, horizon, stride=1, every=1):
    """stpwl_horizon_plan, on the host (no GPU), for horizon_error(model, records of E episodes of T rows, horizon, stride=, every=):
    {'windows', 'block' (windows of a workgroup), 'blocks', 'mode' ('l2' | 'staged' | 'staged_held'), 'lds_bytes', 'launches',
    'pred_cap_bytes' (the largest x_pred that predictions=True may ask for)}; raises when the call would be refused (n_x > 128, H > 1024,
    W = 0 windows, ..)."""
    who = 'horizon_plan'
    P, r, m, n_z, w_v = _horizon_model(model, who)
    H, stride, every = _horizon_ints(horizon, stride, every, who)
    w, bl, nb, mode, lds, ln, cap = C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_bind().stpwl_horizon_plan(r, m, P, n_z, w_v, int(E), int(T), H, stride, every, C.byref(w), C.byref(bl), C.byref(nb), C.byref(mode),
                                          C.byref(lds), C.byref(ln), C.byref(cap)), 'stpwl_horizon_plan')
    return {'windows': int(w.value), 'block': bl.value, 'blocks': int(nb.value), 'mode': HORIZON_MODES[mode.value], 'lds_bytes': int(lds.value),
            'launches': int(ln.value), 'pred_cap_bytes': int(cap.value)}


class TPWLHorizonError:
    """The result of horizon_error (the module's docstring defines every field): horizon, dt, windows, diverged, bad_rows; for
    k = 0 .. H: sse_x, rms_x, worst_x (H + 1,), worst_x_at (H + 1, 2) = (episode, unstrided row) of the worst window's start, and the same
    with z (None without an output model); on request final_x, final_z, status (W,) and x_pred (W, H + 1, n_x)."""

    def __init__(self, horizon, dt, windows, diverged, bad_rows, sse_x, rms_x, worst_x, worst_x_at, sse_z=None, rms_z=None, worst_z=None,
                 worst_z_at=None, final_x=None, final_z=None, status=None, x_pred=None):
        self.horizon, self.dt, self.windows, self.diverged, self.bad_rows = horizon, dt, windows, diverged, bad_rows
        self.sse_x, self.rms_x, self.worst_x, self.worst_x_at = sse_x, rms_x, worst_x, worst_x_at
        self.sse_z, self.rms_z, self.worst_z, self.worst_z_at = sse_z, rms_z, worst_z, worst_z_at
        self.final_x, self.final_z, self.status, self.x_pred = final_x, final_z, status, x_pred

    @property
    def windows_ok(self):
        return self.windows - self.diverged - self.bad_rows

    def __repr__(self):
        tail = '' if self.rms_z is None else ', rms_z[H]=%g' % self.rms_z[-1]
        return 'TPWLHorizonError(H=%d, %d windows (%d diverged, %d with bad rows), rms_x[H]=%g%s)' % (
            self.horizon, self.windows, self.diverged, self.bad_rows, self.rms_x[-1], tail)


def horizon_error(model, X, U, horizon, dt=None, stride=1, every=1, shape=None, per_window=False, predictions=False):
    """The k-step open-loop prediction error of a nearest-point TPWL model over records, k = 0 .. horizon, from every window start (the
    module's docstring states the definition): a TPWLHorizonError.  X (E, T, n_x) or (T, n_x) and U alike, numpy arrays or
    _lib.DeviceBuffers with shape = (E, T) (read in place); dt defaults to model.fit_Ts."""
    who = 'horizon_error'
    P, r, m, n_z, w_v = _horizon_model(model, who)
    H, stride, every = _horizon_ints(horizon, stride, every, who)
    n_x = 2 * r
    X, U, E, T, dev = _records(X, U, n_x, m, shape, who)
    plan = horizon_plan(model, E, T, H, stride, every)          # every refusal of the shapes, on the host
    W = plan['windows']
    if predictions and 8 * W * (H + 1) * n_x > plan['pred_cap_bytes']:
        raise RuntimeError('%s: predictions of %d windows x %d rows x %d need %d bytes, above the cap of %d bytes'
                           % (who, W, H + 1, n_x, 8 * W * (H + 1) * n_x, plan['pred_cap_bytes']))
    dt = getattr(model, 'fit_Ts', None) if dt is None else dt
    if dt is None:
        raise RuntimeError('%s: the model carries no fit_Ts; give dt' % who)
    h = model.handle_for(float(dt))
    sse, worst = np.zeros((2, H + 1)), np.zeros((2, H + 1))
    at, counts = np.zeros((2, H + 1, 2), dtype=np.int64), np.zeros(3, dtype=np.int64)
    fin = np.zeros((2, W)) if per_window else None
    status = np.zeros(W, dtype=np.int32) if per_window else None
    pred = np.zeros((W, H + 1, n_x)) if predictions else None
    i64p = C.POINTER(C.c_int64)
    args = [E, T, H, stride, every, _lib.dptr(sse), _lib.dptr(worst), at.ctypes.data_as(i64p), counts.ctypes.data_as(i64p),
            _lib.dptr(fin) if per_window else None, _lib.iptr(status) if per_window else None, _lib.dptr(pred) if predictions else None]
    L = _bind()
    if dev:
        _lib.check(L.stpwl_horizon_error_dev(h, X.ptr, U.ptr, *args, None), 'stpwl_horizon_error_dev')
    else:
        _lib.check(L.stpwl_horizon_error(h, _lib.dptr(X), _lib.dptr(U), *args), 'stpwl_horizon_error')
    ok = int(counts[0] - counts[1] - counts[2])

    def rms(s, dim):
        return np.sqrt(s / (ok * dim)) if ok > 0 else np.full(H + 1, np.nan)

    def none(a):                                                # no status-0 window: no maximum
        return np.where(a < 0, np.nan, a)

    out = TPWLHorizonError(H, float(dt), int(counts[0]), int(counts[1]), int(counts[2]), sse[0].copy(), rms(sse[0], n_x), none(worst[0]), at[0].copy())
    if n_z > 0:
        out.sse_z, out.rms_z, out.worst_z, out.worst_z_at = sse[1].copy(), rms(sse[1], n_z), none(worst[1]), at[1].copy()
    if per_window:
        out.final_x, out.final_z, out.status = fin[0].copy(), (fin[1].copy() if n_z > 0 else None), status
    out.x_pred = pred
    return out
