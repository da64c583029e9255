"""Batched closed-loop Koopman MPC: `batch` loops of the reference's controller resident on the device (csrc/koopman_loop.hip).

Every problem of the loop's lift handle is its own loop of koopman.py:75-170 -- the delay-embedded, scaled measurements of the device
ring are lifted into the QP's state, the linear MPC on the lifted model is solved, its plan rows are applied to the plant at the
simulation step and every new measurement goes into the ring.  `run(periods)` is one launch sequence on the handle's stream and ONE host
wait; only the records of the run cross PCIe.

The controller step is the model's Ts, the simulation step dt_sim with Ts = r dt_sim (r an integer >= 1); a period is rollout_horizon
controller steps, n_keep = rollout_horizon r sub-steps; period p starts at t_p = t_start + p n_keep dt_sim.
  reset      the ring <- the `delays` older raw samples (y_hist, u_hist), oldest first, then (y_0, u_prev0) with y_0 = (C x0 + y_ref) + v0
             (or y0 given when there is no plant): add_measurement(y, u_prev) in front of the first compute_policy.  Row 0 of y is y_0.
  request    x0_p = W psi(zeta) of the ring as it stands; targets at (t_p + phase_b) + Ts k, zf the last row when the cost has Qf.
  solve      the trust-region-free QP on the constant (A_d, B_d), d = 0.
  fix-up     a member whose QP reports a non-zero status goes on with the previous plan moved up ONE row, its last row held
             (baselines/ros.py:223-227, whatever rollout_horizon is); in period 0: x0 in every state row, the scaled-down u0 in every
             input row.  The status is recorded either way.
  sub-steps  u_s = scale_up(uopt[s // r]); x_{s+1} = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s;
             y_{s+1} = (C x_{s+1} + y_ref) + v_s, or read from Y_plant; push (y_{s+1}, u_s) -- or (y_{s+1}, U_applied_s) -- into the ring.
  Y          the Y= re-projection of the measurement: behind set_reproject(Polyhedron(A, b, with_reproject=True)) every sample -- y_0 of the reset, every y_{s+1}, stepped or replayed -- that lies
             outside Y is replaced by its Euclidean projection before it enters the ring (koopman.py:150-151), inside the advance kernel,
             by the device function behind Polyhedron.project_to_polyhedron: the same bits.  The result's `y` stays the raw sample,
             `y_used` is what the ring received and `proj` its status word: 0 inside (bit for bit), 1 projected, -1 no certified
             projection (an empty Y), -2 the sample is not finite; with -1 and -2 the raw sample is used and the run goes on.  The
             y_hist rows are taken as given.  The plant is never touched.
The reference reads its input tape at its own knots, so input_hold changes nothing and is not a parameter.

Not offered: the start-up phase before t_delay (the reset states the history at the first solve), projecting the y_hist rows,
input clipping, dU, input_nullspace, nonlinear_observer, weighting-mode plants, the lifted model as its own plant."""
import ctypes as C_          # (C is the plant's measurement matrix in this module)

import numpy as np

from ... import _lib
from ...scp.closed_loop import _LoopBatch, _ptr, schedule


class KoopmanLoopResult:
    """Records of one `run` with S = periods n_keep: x (B, S + 1, n_plant) or None, y (B, S + 1, n_y) -- row 0 where the run started --,
    u (B, S, n_u), all raw; x_lift (periods, B, n_lift) the requests; iters, status, J (periods, B) of the solves; t (S + 1,) the times
    of the rows.  With a Y: y_used (B, S + 1, n_y) the samples as the ring received them and proj (B, S + 1) int32 their status words
    (0 inside, 1 projected, -1 no certified projection, -2 not finite); both None without one."""

    y_used = proj = None

    def __init__(self, x, y, u, x_lift, iters, status, J, t):
        self.x, self.y, self.u, self.x_lift = x, y, u, x_lift
        self.iters, self.status, self.J, self.t = iters, status, J, t


class KoopmanClosedLoopBatch(_LoopBatch):
    _sym = 'skoop_loop'

    def __init__(self, model, N, cost_params, plant, C, y_ref, dt_sim, rollout_horizon, t=None, z=None, u=None, phase=None, U=None, X=None,
                 Xf=None, x_char=None, u0=None, batch=1, max_steps_per_run=None, dU=None, input_nullspace=None):
        """model: a KoopmanModel (A_d, B_d, H, W, scaling, Ts); N, cost_params (Q on the scaled outputs, R, Qf), U, X, Xf, x_char: the QP,
        as KoopmanSolverNode builds it.  plant: a nearest-point TPWLATV stepped at dt_sim with the model's inputs, measured by
        y = C x + y_ref (C (n_y, n_plant), n_y the model's n), or None: replay only (run(Y_plant=...)).  rollout_horizon: controller
        steps per period.  t (T,), z (T, n_y), u (T, n_u) or (n_u,): the target table in the QP's scaled units; phase (B,): a time offset
        of every loop's target.  u0 (n_u) raw: the idle input (a failed first solve, and u_prev0 of a reset without one).  The loop owns
        its lift handle and so its measurement history.  The admissible set of the measurements is set behind the constructor:
        set_reproject(Y)."""
        from ...scp.locp import make_problem
        name = type(self).__name__
        if dU is not None:
            raise RuntimeError('%s: input-rate constraints (dU) are not offered by the resident loop' % name)
        if input_nullspace is not None and input_nullspace is not False:
            raise RuntimeError('%s: input_nullspace is not offered by the resident loop (use KoopmanMPC with an MPCSolverNode)' % name)
        if plant is not None and getattr(plant, 'tpwl_method', 'nn') != 'nn':
            raise RuntimeError("%s: weighting-mode plants (tpwl_method = '%s') are not stepped on the device: the plant must be a "
                               "nearest-point TPWL model" % (name, plant.tpwl_method))
        N, rh = int(N), int(rollout_horizon)
        Ts = float(model.Ts)
        if not dt_sim > 0 or not Ts > 0:
            raise RuntimeError('%s: need Ts > 0 and dt_sim > 0' % name)
        ratio = Ts / float(dt_sim)
        if abs(ratio - round(ratio)) > 1e-9 or round(ratio) < 1:
            raise RuntimeError('%s: Ts / dt_sim = %.12g is not an integer >= 1 (the controller step must be a whole number of simulation '
                               'steps)' % (name, ratio))
        if rh < 1 or rh > N:
            raise RuntimeError('%s: rollout_horizon = %d is outside 1 .. N = %d' % (name, rh, N))
        self.model, self.plant = model, plant                     # (kept alive: the handle points into the plant)
        self.B, self.N, self.dt = int(batch), N, Ts
        self.n_y, self.n_u, self.delays = int(model.n), int(model.m), int(model.delays)
        W = np.asarray(model.W)
        self.n_x = int(W.shape[0])                                # n_lift: the QP's states
        if self.n_x > 96:
            raise RuntimeError('%s: n_lift = %d exceeds the limit n_lift <= 96 of the QP (truncate the model with W)' % (name, self.n_x))
        if self.n_u > 16:
            raise RuntimeError('%s: n_u = %d exceeds the limit n_u <= 16 of the advance kernel' % (name, self.n_u))
        if np.shape(model.A_d) != (self.n_x, self.n_x):
            raise RuntimeError('%s: A_d is %s but the lift writes %d states' % (name, np.shape(model.A_d), self.n_x))
        self.n_plant = 0
        if plant is not None:
            self.n_plant = int(plant.get_state_dim())
            if self.n_plant > 128:
                raise RuntimeError('%s: the plant\'s n_x = %d exceeds the limit n_x <= 128 of the advance kernel' % (name, self.n_plant))
            if int(plant.get_input_dim()) != self.n_u:
                raise RuntimeError('%s: the plant has n_u = %d, the model n_u = %d' % (name, plant.get_input_dim(), self.n_u))
            if C is None or y_ref is None or np.shape(C) != (self.n_y, self.n_plant) or np.size(y_ref) != self.n_y:
                raise RuntimeError('%s: C must have shape (n_y, n_plant) = %s and y_ref n_y = %d entries, got %s and %s'
                                   % (name, (self.n_y, self.n_plant), self.n_y, None if C is None else np.shape(C),
                                      None if y_ref is None else np.shape(y_ref)))
        H = np.asarray(model.H, dtype=np.float64)
        self.n_z = H.shape[0]                                     # the QP's outputs: the target table
        self.r = int(round(ratio))
        self.rollout_horizon, self.dt_sim, self.n_keep = rh, float(dt_sim), rh * self.r
        self.max_steps_per_run = int(max_steps_per_run) if max_steps_per_run is not None else 16 * self.n_keep
        self.has_z, self.has_u = z is not None, u is not None
        self.has_zf = z is not None and cost_params.Qf is not None
        self.t_start, self._k = 0.0, None
        self._h = C_.c_void_p()
        self.u0 = _lib.f64(np.zeros(self.n_u) if u0 is None else np.asarray(u0).reshape(self.n_u))
        x_scale = None if x_char is None else 1. / np.abs(np.asarray(x_char, dtype=np.float64))
        self.lift = model.new_lift(project=True, batch=self.B)
        if self.lift.n_out != self.n_x:
            raise RuntimeError('%s: W has %d rows but the lift writes %d states' % (name, self.n_x, self.lift.n_out))
        self._prob, self._keep = make_problem(self.N, H, cost_params.Q, cost_params.R, cost_params.Qf, U, X, Xf, None, x_scale, tr_active=False)
        self._A, self._Bm = _lib.f64(model.A_d), _lib.f64(model.B_d)
        self._C = None if plant is None else _lib.f64(C)
        self._yref = None if plant is None else _lib.f64(np.ravel(y_ref))
        _lib.check(_lib.lib().skoop_loop_create(C_.byref(self._h), self.lift._h, C_.cast(C_.byref(self._prob), C_.c_void_p), _lib.dptr(self._A),
                                                _lib.dptr(self._Bm), C_.c_double(Ts), plant.handle_for(self.dt_sim) if plant is not None else None,
                                                _lib.dptr(self._C), _lib.dptr(self._yref), _lib.dptr(self.u0), C_.c_double(self.dt_sim),
                                                C_.c_int(rh), C_.c_int64(self.max_steps_per_run)), 'skoop_loop_create')
        if u is not None and np.ndim(u) == 1:
            if t is None:
                raise RuntimeError('%s: a target table needs its times t' % name)
            u = np.tile(np.asarray(u, dtype=np.float64).reshape(1, self.n_u), (np.size(t), 1))
        self._set_target(t, z, u, phase)

    def problem(self):
        """The slocp_problem of the loop's QP (a second plan of the same problem can be made from it)."""
        return self._prob

    def _shaped(self, what, a, shape):
        """`a` as a contiguous float64 array of exactly `shape` (None passes through)."""
        if a is None:
            return None
        a = np.asarray(a)
        if a.shape != shape:
            raise RuntimeError('%s: %s must have shape %s, got %s' % (type(self).__name__, what, shape, a.shape))
        return _lib.f64(a)

    def reset(self, x0=None, y0=None, y_hist=None, u_hist=None, u_prev0=None, v0=None, t_start=0.0):
        """The loop at its first solve, t_start: plant states x0 (B, n_plant), or -- without a plant -- the measurement y0 (B, n_y); the
        `delays` older raw samples y_hist (B, delays, n_y), u_hist (B, delays, n_u), oldest first; u_prev0 (B, n_u) raw: the input
        applied before the first solve (None: u0); v0 (B, n_y): the noise of the first measurement."""
        B, d = self.B, self.delays
        if self.plant is not None and x0 is None:
            raise RuntimeError('%s.reset: x0 is required' % type(self).__name__)
        if self.plant is None and y0 is None:
            raise RuntimeError('%s.reset: the loop has no plant (plant=None: replay only): y0 is required' % type(self).__name__)
        if d > 0 and (y_hist is None or u_hist is None):
            raise RuntimeError('%s.reset: the model has %d delays: y_hist and u_hist are required' % (type(self).__name__, d))
        x0 = self._shaped('x0 (B, n_plant)', x0, (B, self.n_plant)) if self.plant is not None else None
        y0 = self._shaped('y0 (B, n_y)', y0, (B, self.n_y)) if self.plant is None else None
        y_hist = self._shaped('y_hist (B, delays, n_y)', y_hist, (B, d, self.n_y))
        u_hist = self._shaped('u_hist (B, delays, n_u)', u_hist, (B, d, self.n_u))
        u_prev0 = self._shaped('u_prev0 (B, n_u)', u_prev0, (B, self.n_u))
        v0 = self._shaped('v0 (B, n_y)', v0, (B, self.n_y))
        self._call('_reset', *[_lib.dptr(a) for a in (x0, y0, y_hist, u_hist, u_prev0, v0)], C_.c_double(float(t_start)))
        self.t_start, self._k = float(t_start), 0

    def run(self, periods, W=None, V=None, Y_plant=None, U_applied=None, record_x=True):
        """`periods` periods from where the last run ended.  W (periods, n_keep, B, n_plant): added to the plant's next state; V (periods,
        n_keep, B, n_y): measurement noise; Y_plant (B, S + 1, n_y): the measurements are read from this record (a hardware log) instead
        of a stepped plant -- row 0 is where the run starts; U_applied (B, S, n_u): the inputs that go into the ring (the log's actually
        applied ones) instead of the loop's own."""
        name = type(self).__name__
        periods = int(periods)
        if self.plant is None and Y_plant is None:
            raise RuntimeError('%s.run: the loop has no plant (plant=None: replay only): Y_plant is required' % name)
        if self._k is None:
            raise RuntimeError('%s.run: no measurement history yet (call reset first)' % name)
        B, nk, S = self.B, self.n_keep, periods * self.n_keep
        W = self._shaped('W (periods, n_keep, B, n_plant)', W, (periods, nk, B, self.n_plant))
        V = self._shaped('V (periods, n_keep, B, n_y)', V, (periods, nk, B, self.n_y))
        Y_plant = self._shaped('Y_plant (B, S + 1, n_y)', Y_plant, (B, S + 1, self.n_y))
        U_applied = self._shaped('U_applied (B, S, n_u)', U_applied, (B, S, self.n_u))
        fits = periods >= 1 and S <= self.max_steps_per_run
        f64 = lambda *shape: np.empty(shape if fits else 1)
        i32 = lambda: np.empty((periods, B) if fits else 1, dtype=np.int32)
        stepped = self.plant is not None and Y_plant is None
        r = dict(x=f64(B, S + 1, self.n_plant) if fits and record_x and stepped else None, y=f64(B, S + 1, self.n_y), u=f64(B, S, self.n_u),
                 x_lift=f64(periods, B, self.n_x), J=f64(periods, B), status=i32(), iters=i32())
        if self._Y is not None:
            r.update(y_used=f64(B, S + 1, self.n_y), proj=np.empty((B, S + 1) if fits else 1, dtype=np.int32))
        if not fits:                                              # (refused by the library, with its message: it is handed dummies)
            W = V = U_applied = None
            Y_plant = None if Y_plant is None else np.empty(1)
        self._call('_run' if self._Y is None else '_run_reprojected', C_.c_int(periods),
                   *[_ptr(a) for a in [W, V, Y_plant, U_applied] + list(r.values())])
        t = schedule(self.N, self.dt, self.dt_sim, nk, self.t_start, self._k).t_k + self.dt_sim * np.arange(S + 1)
        self._k += periods
        res = KoopmanLoopResult(r['x'], r['y'], r['u'], r['x_lift'], r['iters'], r['status'], r['J'], t)
        res.y_used, res.proj = r.get('y_used'), r.get('proj')
        return res

    def step(self, W=None, V=None, Y_plant=None, U_applied=None, record_x=True):
        return self.run(1, W=W, V=V, Y_plant=Y_plant, U_applied=U_applied, record_x=record_x)

    def last_inputs(self):
        """The solver inputs of the last period: dict x0 (B, n_lift), z (B, N + 1, n_z), zf (B, n_z), u (B, N, n_u) (None where the loop
        has none)."""
        B, N = self.B, self.N
        r = dict(x0=np.empty((B, self.n_x)), z=np.empty((B, N + 1, self.n_z)) if self.has_z else None,
                 zf=np.empty((B, self.n_z)) if self.has_zf else None, u=np.empty((B, N, self.n_u)) if self.has_u else None)
        self._call('_last_inputs', *[_lib.dptr(a) for a in r.values()])
        return r

    def _fixup(self, xopt, uopt, x0, status, xopt_prev=None, uopt_prev=None, first=False):
        """The fix-up kernel alone on host arrays (for tests): the QP's answer xopt (B, N+1, n_lift), uopt (B, N, n_u), the request's x0
        (B, n_lift), status (B,), the previous plan (None when first) -> (xopt_out, uopt_out)."""
        B, N = self.B, self.N
        sx, su = (B, N + 1, self.n_x), (B, N, self.n_u)
        f = lambda a, shape: None if a is None else _lib.f64(np.asarray(a).reshape(shape))
        xopt, uopt, x0, xp, up = f(xopt, sx), f(uopt, su), f(x0, (B, self.n_x)), f(xopt_prev, sx), f(uopt_prev, su)
        status = np.ascontiguousarray(np.asarray(status).reshape(B), dtype=np.int32)
        xo, uo = np.empty(sx), np.empty(su)
        self._call('_fixup', _lib.dptr(xp), _lib.dptr(up), _lib.dptr(xopt), _lib.dptr(uopt), _lib.dptr(x0), _lib.iptr(status),
                   C_.c_int(1 if first else 0), _lib.dptr(xo), _lib.dptr(uo))
        return xo, uo

    def _advance(self, uopt, x=None, W=None, V=None, Y_plant=None, U_applied=None):
        """The advance kernel alone (for tests): plans uopt (B, N, n_u), plant states x (B, n_plant), W (n_keep, B, n_plant), V (n_keep,
        B, n_y), Y_plant (B, n_keep + 1, n_y), U_applied (B, n_keep, n_u) -> dict X (B, n_keep, n_plant; None in replay) and Y after
        every sub-step, U and the plant's points idx (B, n_keep; -1 in replay) of every sub-step.  The samples go into the loop's own
        ring as it stands; the loop needs a reset before its next run.  With a Y also Y_used (B, n_keep, n_y), the samples as the ring
        received them, and proj (B, n_keep) int32, their status words."""
        B, N, nk = self.B, self.N, self.n_keep
        f = lambda a, *shape: None if a is None else _lib.f64(np.asarray(a).reshape(shape))
        uopt, x = f(uopt, B, N, self.n_u), f(x, B, self.n_plant)
        W, V = f(W, nk, B, self.n_plant), f(V, nk, B, self.n_y)
        Y_plant, U_applied = f(Y_plant, B, nk + 1, self.n_y), f(U_applied, B, nk, self.n_u)
        r = dict(X=None if Y_plant is not None else np.empty((B, nk, self.n_plant)), Y=np.empty((B, nk, self.n_y)),
                 U=np.empty((B, nk, self.n_u)), idx=np.empty((B, nk), dtype=np.int32))
        if self._Y is not None:
            r.update(Y_used=np.empty((B, nk, self.n_y)), proj=np.empty((B, nk), dtype=np.int32))
        self._k = None
        self._call('_advance' if self._Y is None else '_advance_reprojected',
                   *[_ptr(a) for a in [uopt, x, W, V, Y_plant, U_applied] + list(r.values())])
        return r
