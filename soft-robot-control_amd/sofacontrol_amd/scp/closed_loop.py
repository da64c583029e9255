"""Batched closed-loop GuSTO: `batch` receding-horizon loops resident on the device (csrc/gusto_loop.hip).

Every rollout of a resident TPWL `GuSTO(batch=B)` is its own loop -- plan, apply `n_keep` inputs to a TPWL plant pre-discretised at
`dt_sim` under the scp controller's feedback law u = u_bar(t) + K[i_near(x_bar(t))] (x - x_bar(t)) (tpwl/controllers.py:298-333), shift
the plan (scp/ros.py:110-114), re-plan from the plant state: the reference's `mpc=True` policy with perfect state feedback.  `run(periods)`
is one launch sequence on the handle's stream and ONE host wait; only the records of the run cross PCIe.  What is shared by all loops --
the times of a period -- is computed on the host in float64 (`schedule`).

With `observer=` (a tpwl.observer.DiscreteEKFObserverBatch) the loop is the reference's output-feedback loop (tpwl/controllers.py:85-117):
the plans start from the filters' estimates, the law reads the estimate, and every plant step is followed by a measurement
y = C x + y_ref (+ v) and one step of every filter -- still one host wait per run.

`mpc=False` selects the reference's DEFAULT policy (tpwl/controllers.py:236): from period 1 on a plan starts from the previous plan at
n_keep dt_sim into it (`schedule_end`), not from the plant or the estimate; `record_tape=True` adds the nominal tape the reference
stitches (x_bar, u_bar of the result).  The default here stays mpc=True."""
import collections
import ctypes as C

import numpy as np

from .. import _lib

Schedule = collections.namedtuple('Schedule', 't_k idx0 j theta')


def schedule(N, dt, dt_sim, n_keep, t_start=0.0, k=0):
    """The schedule of period k, shared by all loops; plain numpy float64 arithmetic, no GPU and no library call.
    t_k = t_start + k (n_keep dt_sim); idx0 = the first row j of the previous plan's times t_{k-1} + dt arange(N + 1) that is >= t_k
    (scp/ros.py:109; 0 for k = 0; N when rounding at n_keep dt_sim == N dt leaves no such row, where the reference's argwhere would
    raise: the last row is then held throughout); for the sub-steps s = 0..n_keep-1 at tau = s dt_sim into the period: the plan
    interval j = min(int(tau / dt), N - 1) and the position theta = (tau - j dt) / dt inside it."""
    N, n_keep, k = int(N), int(n_keep), int(k)
    dt, dt_sim, t_start = float(dt), float(dt_sim), float(t_start)
    step = n_keep * dt_sim
    t_k = t_start + k * step
    idx0 = 0
    if k > 0:
        topt_prev = (t_start + (k - 1) * step) + dt * np.arange(N + 1)
        hits = np.argwhere(topt_prev >= t_k)
        idx0 = int(hits[0, 0]) if len(hits) else N
    tau = np.arange(n_keep) * dt_sim
    j = np.minimum((tau / dt).astype(np.int64), N - 1)
    theta = (tau - j * dt) / dt
    return Schedule(t_k, idx0, j, theta)


def schedule_end(N, dt, dt_sim, n_keep):
    """(j_end, theta_end): the rule of a sub-step at the period's end tau = n_keep dt_sim -- where the chained policy (mpc=False) reads
    the plan for the next period's start state, x_opt[-1] of tpwl/controllers.py:272.  At n_keep dt_sim == N dt: j_end = N - 1 and
    theta_end is 1 to rounding.  Plain float64 arithmetic, no GPU and no library call."""
    N, n_keep, dt, dt_sim = int(N), int(n_keep), float(dt), float(dt_sim)
    tau = n_keep * dt_sim
    j = min(int(tau / dt), N - 1)
    return j, (tau - j * dt) / dt


class ClosedLoopResult:
    """Records of one `run`: x (B, S + 1, n_x) or None, z (B, S + 1, n_z), u (B, S, n_u) with S = periods n_keep (row 0: the state the run
    started from); iters, status, J (periods, B) of the solves; t (S + 1,) the times of the rows."""

    # a loop with a Y (SSMClosedLoopBatch.set_reproject; None without one): y_used (B, S + 1, n_o) the measurements as the observer map read
    # them, proj (B, S + 1) int32 their status words: 0 inside Y, 1 projected, -1 no certified projection, -2 not finite
    y_used = proj = None

    def __init__(self, x, z, u, iters, status, J, t, x_hat=None, y=None, ekf_status=None, x_bar=None, u_bar=None):
        self.x, self.z, self.u, self.iters, self.status, self.J, self.t = x, z, u, iters, status, J, t
        # the chained policy's nominal tape (ClosedLoopBatch(mpc=False, record_tape=True); None otherwise): x_bar (B, S + 1, n_x), u_bar
        # (B, S + 1, n_u), the reference's x_opt / u_opt of save_controller_info at the rows' times
        self.x_bar, self.u_bar = x_bar, u_bar
        # the observed loop (None without an observer): x_hat (B, S + 1, n_x) the estimates, row 0 those the run started from; y (B, S,
        # n_y) the measurements; ekf_status (periods, B) the OR of the period's filter statuses
        self.x_hat, self.y, self.ekf_status = x_hat, y, ekf_status


def _ptr(a):
    return _lib.iptr(a) if a is not None and a.dtype == np.int32 else _lib.dptr(a)


class _LoopBatch:
    """What ClosedLoopBatch and SSMClosedLoopBatch share: the refusals that need no device, the target table, the arrays of a run, the
    times of its rows and the period count, and the accessors of the last period.  `_sym`: the prefix of the class's entry points in the
    library, `_max_iters`: the entry point that caps the plan's GuSTO iterations; has_zf stays None where a loop has no terminal target."""
    _sym = _max_iters = has_zf = None

    @classmethod
    def _check_periods(cls, gusto, dt_sim, n_keep):
        n_keep = int(n_keep)
        if n_keep < 1 or not dt_sim > 0:
            raise RuntimeError('%s: need n_keep >= 1 and dt_sim > 0' % cls.__name__)
        if n_keep * float(dt_sim) > gusto.N * float(gusto.dt):
            raise RuntimeError('%s: n_keep * dt_sim = %g exceeds the horizon N * dt = %g (the shift of the previous plan '
                               'would find no row)' % (cls.__name__, n_keep * float(dt_sim), gusto.N * float(gusto.dt)))
        return n_keep

    def _shape(self, gusto, dt_sim, n_keep, max_steps_per_run, z, u):
        self.B, self.N, self.dt = gusto.batch, gusto.N, float(gusto.dt)
        self.n_x, self.n_u, self.n_z = gusto.n_x, gusto.n_u, gusto.n_z
        self.dt_sim, self.n_keep = float(dt_sim), n_keep
        self.max_steps_per_run = int(max_steps_per_run) if max_steps_per_run is not None else 16 * n_keep
        self.has_z, self.has_u = z is not None, u is not None
        self.t_start, self._k = 0.0, None
        self._h = C.c_void_p()

    @classmethod
    def _check_reproject(cls, Y, n_y):
        """The admissible set of the measurements as the advance kernels take it: (A (rows, n_y), b (rows,)) of a
        Polyhedron(with_reproject=True), or None.  Everything else is refused here, before any device call."""
        if Y is None:
            return None
        from ..utils import Polyhedron
        name = cls.__name__
        if not isinstance(Y, Polyhedron):
            raise RuntimeError('%s: Y must be a Polyhedron(A, b, with_reproject=True), got %s' % (name, type(Y).__name__))
        if not Y.with_reproject:
            raise RuntimeError('%s: Y was made without with_reproject=True: the reference refuses to project onto it '
                               '(Polyhedron(A, b, with_reproject=True))' % name)
        A, b = np.asarray(Y.A, dtype=np.float64), np.asarray(Y.b, dtype=np.float64).reshape(-1)
        if A.ndim != 2 or A.shape[1] != n_y or A.shape[0] != b.shape[0]:
            raise RuntimeError('%s: Y needs A of shape (rows, n_y = %d) and b of rows entries, got A %s and b %s'
                               % (name, n_y, A.shape, b.shape))
        if n_y > 16 or A.shape[0] > 64 or A.shape[0] < 1:
            raise RuntimeError('%s: the re-projection onto Y is limited to n_y <= 16 and 1 <= rows <= 64 (got n_y = %d, rows = %d)'
                               % (name, n_y, A.shape[0]))
        if not (np.isfinite(A).all() and np.isfinite(b).all()):
            bad = int(np.argmax(~(np.isfinite(A).all(axis=1) & np.isfinite(b))))
            raise RuntimeError('%s: Y is not finite (row %d of A or b holds a NaN or an Inf)' % (name, bad))
        return _lib.f64(A), _lib.f64(b)

    _Y = None                                                      # (A, b) of the admissible set of the measurements, or None
    _n_meas = 'n_y'                                                # the attribute that holds the measurement's dimension

    def set_reproject(self, Y):
        """The admissible set of the measurements (the reference's `Y=` of KoopmanMPC and of the SSM scp controller): from the next reset on
        every measurement outside Y is replaced by its Euclidean projection before the controller reads it, inside the advance kernel.
        Y: a Polyhedron(A, b, with_reproject=True) in the raw measurement's coordinates, at most 16 dimensions and 64 rows; None removes
        it.  Refused by name, with the numbers, before any device call.  The loop needs a reset behind it.  Returns the loop."""
        Yab = self._check_reproject(Y, int(getattr(self, self._n_meas)))
        self._check_reproject_allowed(Yab)
        if Yab is None:
            self._call('_set_reproject', None, None, C.c_int(0))
        else:
            self._call('_set_reproject', _lib.dptr(Yab[0]), _lib.dptr(Yab[1]), C.c_int(Yab[0].shape[0]))
        self._Y, self._k = Yab, None
        return self

    def _check_reproject_allowed(self, Yab):
        pass

    def _call(self, entry, *args):
        _lib.check(getattr(_lib.lib(), self._sym + entry)(self._h, *args), self._sym + entry)

    def _set_target(self, t, z, u, phase):
        if z is None and u is None:
            return
        if t is None:
            raise RuntimeError('%s: a target table needs its times t' % type(self).__name__)
        t = _lib.f64(np.asarray(t).reshape(-1))
        T = t.shape[0]
        z = None if z is None else _lib.f64(np.asarray(z).reshape(T, self.n_z))
        u = None if u is None else _lib.f64(np.asarray(u).reshape(T, self.n_u))
        phase = None if phase is None else _lib.f64(np.asarray(phase).reshape(self.B))
        self._call('_set_target', C.c_int(T), _lib.dptr(t), _lib.dptr(z), _lib.dptr(u), _lib.dptr(phase))

    def __del__(self):
        try:
            if self._h:
                getattr(_lib.lib(), self._sym + '_destroy')(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _records(self, periods, record_x, z_width, **more):
        """(fits, the arrays a run of `periods` fills): x (or None), z (B, S + 1, z_width), u, iters, status, J and of `more` name -> (rows
        beyond S, width), or None for an int32 (periods, B) record.  What does not fit is refused by the library, with its message: it is
        handed dummies."""
        B, S = self.B, periods * self.n_keep
        fits = periods >= 1 and S <= self.max_steps_per_run
        f64 = lambda *shape: np.empty(shape if fits else 1)
        i32 = lambda: np.empty((periods, B) if fits else 1, dtype=np.int32)
        r = dict(x=f64(B, S + 1, self.n_x) if fits and record_x else None, z=f64(B, S + 1, z_width), u=f64(B, S, self.n_u), iters=i32(), status=i32(),
                 J=f64(periods, B))
        r.update((k, i32() if v is None else f64(B, S + v[0], v[1])) for k, v in more.items())
        return fits, r

    def _run(self, entry, periods, arrays, r):
        """The library's run on `arrays` (noise, then the records r in the entry point's order) -> ClosedLoopResult of r with its times."""
        _lib.check(getattr(_lib.lib(), self._max_iters)(self.gusto.plan, C.c_int(int(self.gusto.max_gusto_iters))), 'set_max_iters')
        self._call(entry, C.c_int(periods), *[_ptr(a) for a in arrays])
        t = schedule(self.N, self.dt, self.dt_sim, self.n_keep, self.t_start, self._k).t_k + self.dt_sim * np.arange(periods * self.n_keep + 1)
        self._k += periods
        res = ClosedLoopResult(r['x'], r['z'], r['u'], r['iters'], r['status'], r['J'], t, x_hat=r.get('x_hat'), y=r.get('y'), ekf_status=r.get('ekf_status'),
                               x_bar=r.get('x_bar'), u_bar=r.get('u_bar'))
        res.y_used, res.proj = r.get('y_used'), r.get('proj')
        return res

    def step(self):
        return self.run(1)

    def last_inputs(self):
        """The solver inputs of the last period: dict x0, u_init, x_init, z, zf (TPWL loops), u (None where the loop has none)."""
        B, N = self.B, self.N
        r = dict(x0=np.empty((B, self.n_x)), u_init=np.empty((B, N, self.n_u)), x_init=np.empty((B, N + 1, self.n_x)),
                 z=np.empty((B, N + 1, self.n_z)) if self.has_z else None)
        if self.has_zf is not None:
            r['zf'] = np.empty((B, self.n_z)) if self.has_zf else None
        r['u'] = np.empty((B, N, self.n_u)) if self.has_u else None
        self._call('_last_inputs', *[_lib.dptr(a) for a in r.values()])
        return r

    def last_plan(self):
        xo, uo = np.empty((self.B, self.N + 1, self.n_x)), np.empty((self.B, self.N, self.n_u))
        self._call('_last_plan', _lib.dptr(xo), _lib.dptr(uo))
        return xo, uo

    def stats(self):
        steps, waits = C.c_int64(0), C.c_int64(0)
        self._call('_stats', C.byref(steps), C.byref(waits))
        return {'steps': steps.value, 'waits_last_run': waits.value}


class ClosedLoopBatch(_LoopBatch):
    _sym, _max_iters = 'sgusto_loop', 'sgusto_plan_set_max_iters'

    def __init__(self, gusto, plant, dt_sim, n_keep, t=None, z=None, u=None, phase=None, K=None, max_steps_per_run=None, observer=None, mpc=True,
                 record_tape=False):
        """gusto: a GuSTO on a TPWLGuSTO model with batch=B (the fused resident plan); plant: a TPWLATV (it may be the planner's own
        dyn_sys), stepped at dt_sim; n_keep: plant steps per period (the reference's N_replan with the controller clock at dt_sim).
        t (T,), z (T, n_z), u (T, n_u): the target table, interpolated as scp/standalone.py:29-31 does; phase (B,): a time offset of
        every loop's target; K: the per-point gains of the scp controller (list of (n_u, n_x), or (P, n_u, n_x)), None: u = u_bar.
        max_steps_per_run: the longest run in plant steps (sizes the record blocks; default 16 periods).
        observer: a DiscreteEKFObserverBatch of the same batch, n_x and n_u; its model is stepped at dt_sim (it may be the planner's
        dyn_sys, and it need not be the plant).  The loop binds it to dt_sim and steps it on its own stream: do not step it elsewhere
        while the loop is in use.
        mpc: the reference's flag of the same name (tpwl/controllers.py:236).  True, the default HERE: every period re-plans from the
        plant state (the estimate with an observer).  False -- the REFERENCE's default, and what its TPWL drivers run
        (examples/diamond/diamond.py:249, examples/hardware/diamond.py:270, examples/trunk/trunk.py:266) --: the chained policy.  Period 0
        after a reset is the same; period k >= 1 starts from the previous plan at tau = n_keep dt_sim into it (`schedule_end`; x_opt[-1]
        of controllers.py:272), so the plans do not depend on the plant and only the law and the filters close the loop.  Warm start,
        targets, law and plant step are the same; one small launch per period is added (loop_chain_kernel).
        record_tape: with mpc=False, every run also returns the nominal tape the reference stitches (x_opt / u_opt of
        save_controller_info): x_bar (B, S + 1, n_x), u_bar (B, S + 1, n_u) of the result.  Row p n_keep + s is plan p at s dt_sim; at a
        junction row k n_keep (k >= 1) x_bar keeps the old plan's end and u_bar takes the new plan's first row, as the reference's
        concatenate does (controllers.py:313-315).  It is a property of the loop (`set_record_tape`), not of a call."""
        if not (getattr(gusto, '_fused', False) and not getattr(gusto, '_ssm', False)):
            raise RuntimeError('ClosedLoopBatch needs a GuSTO on a TPWLGuSTO model with a fused resident plan (not an SSM plan, not '
                               'the host loop): there is no device rollout / solve to chain otherwise')
        n_keep = self._check_periods(gusto, dt_sim, n_keep)
        if observer is not None:
            shape = (getattr(observer, 'batch', None), getattr(observer, 'state_dim', None), getattr(observer, 'input_dim', None))
            if shape != (gusto.batch, gusto.n_x, gusto.n_u):
                raise RuntimeError('ClosedLoopBatch: the observer has batch = %s, n_x = %s, n_u = %s; the loop needs batch = %d, n_x = %d, '
                                   'n_u = %d' % (shape + (gusto.batch, gusto.n_x, gusto.n_u)))
        self.gusto, self.plant, self.observer = gusto, plant, observer       # (kept alive: the handle points into all three)
        self._shape(gusto, dt_sim, n_keep, max_steps_per_run, z, u)
        self.has_zf, self.has_K = z is not None and gusto.Qzf is not None, K is not None
        lib = _lib.lib()
        _lib.check(lib.sgusto_loop_create(C.byref(self._h), gusto.plan, gusto.model.dyn_sys.handle_for(self.dt),
                                          plant.handle_for(self.dt_sim), C.c_double(self.dt_sim), C.c_int(n_keep),
                                          C.c_int64(self.max_steps_per_run)), 'sgusto_loop_create')
        self._set_target(t, z, u, phase)
        if K is not None:
            K = _lib.f64(np.stack([np.asarray(k) for k in K]).reshape(-1, self.n_u, self.n_x))
            if K.shape[0] != gusto.model.dyn_sys.num_points:
                raise RuntimeError('ClosedLoopBatch: K has %d gains, the planner\'s model %d points' % (K.shape[0], gusto.model.dyn_sys.num_points))
            self._call('_set_feedback', _lib.dptr(K))
        self.n_y = None
        if observer is not None:
            observer.bind(self.dt_sim)
            self.n_y = observer.meas_dim
            self._call('_set_observer', observer._h)
        self.mpc, self.record_tape = bool(mpc), False
        if not self.mpc:
            self._call('_set_chained', C.c_int(1))
        self.set_record_tape(record_tape)

    def set_record_tape(self, on):
        """Whether the runs from now on return the chained policy's tape (x_bar, u_bar of the result).  Refused with mpc=True: a loop
        that re-plans from the plant follows no nominal tape.  Returns the loop."""
        if on and self.mpc:
            raise RuntimeError('ClosedLoopBatch: record_tape=True needs mpc=False: a loop that re-plans from the plant every period '
                               '(mpc=True) follows no nominal tape')
        self.record_tape = bool(on)
        return self

    def reset(self, x0, t_start=0.0):
        """Plant states x0 (B, n_x) at t_start.  With an observer: reset_observed(x0, None, t_start) -- the estimates start at x0."""
        if self.observer is not None:
            return self.reset_observed(x0, None, t_start)
        x0 = _lib.f64(np.asarray(x0).reshape(self.B, self.n_x))
        self._call('_reset', _lib.dptr(x0), C.c_double(float(t_start)))
        self.t_start, self._k = float(t_start), 0

    def reset_observed(self, x0, x_hat0=None, t_start=0.0):
        """Plant states x0 and estimates x_hat0 (B, n_x; None: x0) at t_start.  x_hat0 is the caller's statement of where the reference's
        first observer.update at t = 0 leaves the filters; their covariances are re-installed from Sigma0, so a run is reproducible."""
        if self.observer is None:
            raise RuntimeError('ClosedLoopBatch.reset_observed: the loop has no observer (ClosedLoopBatch(..., observer=...))')
        x0 = _lib.f64(np.asarray(x0).reshape(self.B, self.n_x))
        if x_hat0 is not None:
            x_hat0 = np.asarray(x_hat0)
            if x_hat0.shape != (self.B, self.n_x):
                raise RuntimeError('ClosedLoopBatch.reset_observed: x_hat0 must have shape (B, n_x) = %s, got %s' % ((self.B, self.n_x), x_hat0.shape))
            x_hat0 = _lib.f64(x_hat0)
        self._call('_reset_observed', _lib.dptr(x0), _lib.dptr(x_hat0), C.c_double(float(t_start)))
        self.t_start, self._k = float(t_start), 0

    def run(self, periods, W=None, record_x=True):
        """`periods` periods from where the last run ended.  W (periods, n_keep, B, n_x): added to the plant's next state.
        With an observer: run_observed without measurement noise."""
        if self.observer is not None:
            return self.run_observed(periods, W=W, V=None, record_x=record_x)
        periods = int(periods)
        fits, r = self._records(periods, record_x, self.n_z)
        W = None if W is None or not fits else _lib.f64(np.asarray(W).reshape(periods, self.n_keep, self.B, self.n_x))
        if self.record_tape:
            return self._run_tape(periods, fits, [W, None], r, [None] * 3)
        return self._run('_run', periods, [W] + list(r.values()), r)

    def _run_tape(self, periods, fits, noise, r, observed):
        """sgusto_loop_run_tape: the records r, the observed loop's records (or three None), then the tape."""
        B, S = self.B, periods * self.n_keep
        r = dict(r, x_bar=np.empty((B, S + 1, self.n_x) if fits else 1), u_bar=np.empty((B, S + 1, self.n_u) if fits else 1))
        head = [r[k] for k in ('x', 'z', 'u', 'iters', 'status', 'J')]
        return self._run('_run_tape', periods, noise + head + observed + [r['x_bar'], r['u_bar']], r)

    def run_observed(self, periods, W=None, V=None, record_x=True):
        """run with the filters in the loop.  V (periods, n_keep, B, n_y): measurement noise, None: zero.  The result carries x_hat, y
        and ekf_status."""
        if self.observer is None:
            raise RuntimeError('ClosedLoopBatch.run_observed: the loop has no observer (ClosedLoopBatch(..., observer=...))')
        periods = int(periods)
        if V is not None:
            V = np.asarray(V)
            if V.shape != (periods, self.n_keep, self.B, self.n_y):
                raise RuntimeError('ClosedLoopBatch.run_observed: V must have shape (periods, n_keep, B, n_y) = %s, got %s'
                                   % ((periods, self.n_keep, self.B, self.n_y), V.shape))
            V = _lib.f64(V)
        fits, r = self._records(periods, record_x, self.n_z, x_hat=(1, self.n_x), y=(0, self.n_y), ekf_status=None)
        W = None if W is None or not fits else _lib.f64(np.asarray(W).reshape(periods, self.n_keep, self.B, self.n_x))
        if self.record_tape:
            return self._run_tape(periods, fits, [W, V if fits else None], r, [r['x_hat'], r['y'], r['ekf_status']])
        return self._run('_run_observed', periods, [W, V if fits else None] + list(r.values()), r)

    def _chain(self, xopt, uopt):
        """The chain kernel alone on host-supplied plans (for tests): xopt (B, N+1, n_x), uopt (B, N, n_u) -> x_next (B, n_x), the start
        state of the next period, and the tape rows s = 0..n_keep of a period: x_bar (B, n_keep + 1, n_x), u_bar (B, n_keep + 1, n_u)."""
        B, N, nk = self.B, self.N, self.n_keep
        xopt, uopt = np.asarray(xopt), np.asarray(uopt)
        if xopt.shape != (B, N + 1, self.n_x) or uopt.shape != (B, N, self.n_u):
            raise RuntimeError('ClosedLoopBatch._chain: xopt must have shape (B, N + 1, n_x) = %s and uopt (B, N, n_u) = %s, got %s and %s'
                               % ((B, N + 1, self.n_x), (B, N, self.n_u), xopt.shape, uopt.shape))
        xopt, uopt = _lib.f64(xopt), _lib.f64(uopt)
        xn, xb, ub = np.empty((B, self.n_x)), np.empty((B, nk + 1, self.n_x)), np.empty((B, nk + 1, self.n_u))
        _lib.check(_lib.lib().sgusto_loop_chain(self._h, _lib.dptr(xopt), _lib.dptr(uopt), _lib.dptr(xn), _lib.dptr(xb), _lib.dptr(ub)),
                   'sgusto_loop_chain')
        return xn, xb, ub

    def _advance(self, xopt, uopt, x, W=None):
        """The advance kernel alone on host-supplied plans (for tests): xopt (B, N+1, n_x), uopt (B, N, n_u), x (B, n_x), W (n_keep, B,
        n_x) -> X (B, n_keep, n_x), Z, U, and the points picked, idx_plant, idx_gain (B, n_keep; -1 without gains)."""
        B, N, nk = self.B, self.N, self.n_keep
        xopt = _lib.f64(np.asarray(xopt).reshape(B, N + 1, self.n_x)); uopt = _lib.f64(np.asarray(uopt).reshape(B, N, self.n_u))
        x = _lib.f64(np.asarray(x).reshape(B, self.n_x))
        W = None if W is None else _lib.f64(np.asarray(W).reshape(nk, B, self.n_x))
        X, Z, U = np.empty((B, nk, self.n_x)), np.empty((B, nk, self.n_z)), np.empty((B, nk, self.n_u))
        ip, ig = np.empty((B, nk), dtype=np.int32), np.empty((B, nk), dtype=np.int32)
        _lib.check(_lib.lib().sgusto_loop_advance(self._h, _lib.dptr(xopt), _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W), _lib.dptr(X),
                                                  _lib.dptr(Z), _lib.dptr(U), _lib.iptr(ip), _lib.iptr(ig)), 'sgusto_loop_advance')
        return X, Z, U, ip, ig

    def _advance_observed(self, xopt, uopt, x, x_hat, W=None, V=None):
        """The observed sub-step chain alone on host-supplied plans, states and estimates (for tests; the filters start from x_hat and
        Sigma0, and the loop needs a reset afterwards) -> dict X, Z, U, Xhat (B, n_keep, .), Y (B, n_keep, n_y), idx_plant, idx_gain,
        idx_filter (B, n_keep), ekf_status (B,)."""
        B, N, nk = self.B, self.N, self.n_keep
        xopt = _lib.f64(np.asarray(xopt).reshape(B, N + 1, self.n_x)); uopt = _lib.f64(np.asarray(uopt).reshape(B, N, self.n_u))
        x, x_hat = _lib.f64(np.asarray(x).reshape(B, self.n_x)), _lib.f64(np.asarray(x_hat).reshape(B, self.n_x))
        W = None if W is None else _lib.f64(np.asarray(W).reshape(nk, B, self.n_x))
        V = None if V is None else _lib.f64(np.asarray(V).reshape(nk, B, self.n_y))
        X, Z, U = np.empty((B, nk, self.n_x)), np.empty((B, nk, self.n_z)), np.empty((B, nk, self.n_u))
        Xh, Y = np.empty((B, nk, self.n_x)), np.empty((B, nk, self.n_y))
        ip, ig, jf = (np.empty((B, nk), dtype=np.int32) for _ in range(3))
        es = np.empty(B, dtype=np.int32)
        _lib.check(_lib.lib().sgusto_loop_advance_observed(self._h, _lib.dptr(xopt), _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(x_hat), _lib.dptr(W),
                                                           _lib.dptr(V), _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U), _lib.dptr(Xh), _lib.dptr(Y),
                                                           _lib.iptr(ip), _lib.iptr(ig), _lib.iptr(jf), _lib.iptr(es)),
                   'sgusto_loop_advance_observed')
        self._k = None
        return dict(X=X, Z=Z, U=U, Xhat=Xh, Y=Y, idx_plant=ip, idx_gain=ig, idx_filter=jf, ekf_status=es)
