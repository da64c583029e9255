"""Batched closed-loop ROMPC: `batch` loops of the reference's controller resident on the device (csrc/rompc_loop.hip).

Every problem of a `DiscreteLuenbergerObserver(batch=B)` is its own loop of rompc.py:57-141 -- the linear reduced-order MPC is solved
from the END of the stitched nominal trajectory (only the first plan starts from the estimate), the plant follows that trajectory under
u = ubar(t) + K (x_hat - xbar(t)), and the Luenberger observer is updated from the measurement y = C x + y_ref (+ v) of every step.
`run(periods)` is one launch sequence on the handle's stream and ONE host wait; only the records of the run cross PCIe.

Period p starts at t_p = t_start + p n_replan dt_sim.  Request: x0_p = x_hat0 of the reset, then the previous plan interpolated at
n_replan dt_sim; targets at (t_p + phase_b) + dt_mpc k.  Solve: the trust-region-free QP on the constant (A_d, B_d, d_d) of `mpc_model`.
Chain: row 0 of the plan's states <- x0_p; a member whose QP reports a non-zero status continues on the previous plan moved up one row
(baselines/ros.py:223-227; in period 0: x0 in every row, zero inputs).  Sub-steps: measure, input, observer update, plant step.

Not offered: the start-up phase before t_delay (x0 of a reset is the plant state at the first solve), the full-order state and its
projection per step, input clipping, dU rows, input_nullspace."""
import ctypes as C

import numpy as np

from ... import _lib
from ...scp.closed_loop import _LoopBatch, _ptr, schedule


class ROMPCLoopResult:
    """Records of one `run` with S = periods n_replan: x, x_hat, x_bar (B, S + 1, n_x) -- row 0 where the run started, the last row of
    x_bar the next request's x0 --, z (B, S + 1, n_z) = H x without z_ref, y (B, S, n_y), u, u_bar (B, S, n_u); iters, status, J
    (periods, B) of the solves; t (S + 1,) the times of the rows."""

    def __init__(self, x, x_hat, y, z, u, u_bar, x_bar, iters, status, J, t):
        self.x, self.x_hat, self.y, self.z, self.u, self.u_bar, self.x_bar = x, x_hat, y, z, u, u_bar, x_bar
        self.iters, self.status, self.J, self.t = iters, status, J, t


class ROMPCClosedLoopBatch(_LoopBatch):
    _sym = 'srompc_loop'

    def __init__(self, observer, mpc_model, N, dt_mpc, cost_params, plant, dt_sim, n_replan, t=None, z=None, u=None, phase=None,
                 U=None, X=None, Xf=None, x_char=None, max_steps_per_run=None, dU=None, input_nullspace=None):
        """observer: a DiscreteLuenbergerObserver(model, Q, R, batch=B) with its K set (as ROMPC sets it); its model is the controller's
        at dt_sim.  mpc_model: a LinearROM at dt_mpc (A_d, B_d, d_d, H); N, cost_params (Q on the outputs, R, Qf), U, X, Xf, x_char: the
        QP, as KoopmanSolverNode builds it.  plant: a nearest-point TPWLATV stepped at dt_sim, or None: replay only (run(X_plant=...)).
        n_replan: controller steps per period (the reference's N_replan).  t (T,), z (T, n_z), u (T, n_u): the target table; phase (B,):
        a time offset of every loop's target.  The loop keeps its estimate in the observer's device buffer: do not step the observer
        elsewhere between a reset and the end of the runs that follow."""
        from ...scp.locp import make_problem
        name = type(self).__name__
        if dU is not None:
            raise RuntimeError('%s: input-rate constraints (dU) are not offered by the resident loop' % name)
        if input_nullspace is not None and input_nullspace is not False:
            raise RuntimeError('%s: input_nullspace is not offered by the resident loop (use ROMPC with an MPCSolverNode)' % name)
        if plant is not None and getattr(plant, 'tpwl_method', 'nn') != 'nn':
            raise RuntimeError("%s: weighting-mode plants (tpwl_method = '%s') are not stepped on the device: the plant must be a "
                               "nearest-point TPWL model" % (name, plant.tpwl_method))
        n_replan = int(n_replan)
        if n_replan < 1 or not dt_sim > 0:
            raise RuntimeError('%s: need n_replan >= 1 and dt_sim > 0' % name)
        if n_replan * float(dt_sim) > int(N) * float(dt_mpc):
            raise RuntimeError('%s: n_replan * dt_sim = %g exceeds the horizon N * dt_mpc = %g (the next request would start behind the '
                               'plan)' % (name, n_replan * float(dt_sim), int(N) * float(dt_mpc)))
        self.observer, self.mpc_model, self.plant = observer, mpc_model, plant        # (kept alive: the handle points into them)
        self.B, self.N, self.dt = int(observer.batch), int(N), float(dt_mpc)
        self.n_x, self.n_u, self.n_y = observer.n_x, observer.n_u, observer.n_y
        if self.n_u > 16 or self.n_x > 128:
            raise RuntimeError('%s: n_x = %d, n_u = %d exceeds the limit n_x <= 128, n_u <= 16 of the advance kernel' % (name, self.n_x, self.n_u))
        self.n_zc = observer.n_z                                  # the controller's output map: the z record
        H = np.asarray(mpc_model.H, dtype=np.float64)
        self.n_z = H.shape[0]                                     # the QP's outputs: the target table
        if plant is not None and (plant.get_state_dim(), plant.get_input_dim()) != (self.n_x, self.n_u):
            raise RuntimeError('%s: the plant has n_x = %d, n_u = %d, the controller n_x = %d, n_u = %d'
                               % (name, plant.get_state_dim(), plant.get_input_dim(), self.n_x, self.n_u))
        self.dt_sim, self.n_keep = float(dt_sim), n_replan
        self.n_replan = n_replan
        self.max_steps_per_run = int(max_steps_per_run) if max_steps_per_run is not None else 16 * n_replan
        self.has_z, self.has_u = z is not None, u is not None
        self.has_zf = z is not None and cost_params.Qf is not None
        self.t_start, self._k = 0.0, None
        self._h = C.c_void_p()
        x_scale = None if x_char is None else 1. / np.abs(np.asarray(x_char, dtype=np.float64))
        self._prob, self._keep = make_problem(self.N, H, cost_params.Q, cost_params.R, cost_params.Qf, U, X, Xf, None, x_scale, tr_active=False)
        d_d = getattr(mpc_model, 'd_d', None)
        self._A, self._B = _lib.f64(mpc_model.A_d), _lib.f64(mpc_model.B_d)
        self._d = _lib.f64(np.zeros(self.n_x) if d_d is None else np.ravel(d_d))
        _lib.check(_lib.lib().srompc_loop_create(C.byref(self._h), observer._h, C.cast(C.byref(self._prob), C.c_void_p), _lib.dptr(self._A),
                                                 _lib.dptr(self._B), _lib.dptr(self._d), C.c_double(self.dt),
                                                 plant.handle_for(self.dt_sim) if plant is not None else None, C.c_double(self.dt_sim),
                                                 C.c_int(n_replan), C.c_int64(self.max_steps_per_run)), 'srompc_loop_create')
        self._set_target(t, z, u, phase)

    def problem(self):
        """The slocp_problem of the loop's QP (a second plan of the same problem can be made from it)."""
        return self._prob

    def reset(self, x0, x_hat0=None, t_start=0.0):
        """Plant states x0 and estimates x_hat0 (B, n_x; None: x0) at the first solve, t_start.  The controller's gains and model are read
        from the observer here."""
        x0 = _lib.f64(np.asarray(x0).reshape(self.B, self.n_x))
        if x_hat0 is not None:
            x_hat0 = _lib.f64(np.asarray(x_hat0).reshape(self.B, self.n_x))
        self._call('_reset', _lib.dptr(x0), _lib.dptr(x_hat0), C.c_double(float(t_start)))
        self.t_start, self._k = float(t_start), 0

    def run(self, periods, W=None, V=None, X_plant=None, record_x=True):
        """`periods` periods from where the last run ended.  W (periods, n_replan, B, n_x): added to the plant's next state; V (periods,
        n_replan, B, n_y): measurement noise; X_plant (B, S + 1, n_x): the plant's states are read from this record (a hardware log)
        instead of being stepped -- row 0 is where the run starts."""
        periods = int(periods)
        if self.plant is None and X_plant is None:
            raise RuntimeError('%s.run: the loop has no plant (plant=None: replay only): X_plant is required' % type(self).__name__)
        if self._k is None:
            raise RuntimeError('%s.run: no plant state and estimate yet (call reset first)' % type(self).__name__)
        B, S = self.B, periods * self.n_keep
        fits = periods >= 1 and S <= self.max_steps_per_run
        f64 = lambda *shape: np.empty(shape if fits else 1)
        i32 = lambda: np.empty((periods, B) if fits else 1, dtype=np.int32)
        r = dict(x=f64(B, S + 1, self.n_x) if fits and record_x else None, x_hat=f64(B, S + 1, self.n_x), y=f64(B, S, self.n_y),
                 z=f64(B, S + 1, self.n_zc), u=f64(B, S, self.n_u), u_bar=f64(B, S, self.n_u), x_bar=f64(B, S + 1, self.n_x), J=f64(periods, B),
                 status=i32(), iters=i32())
        shaped = lambda a, *shape: None if a is None or not fits else _lib.f64(np.asarray(a).reshape(shape))
        W = shaped(W, periods, self.n_keep, B, self.n_x)
        V = shaped(V, periods, self.n_keep, B, self.n_y)
        if X_plant is not None and fits:
            X_plant = shaped(X_plant, B, S + 1, self.n_x)
        elif X_plant is not None:
            X_plant = np.empty(1)
        self._call('_run', C.c_int(periods), *[_ptr(a) for a in [W, V, X_plant] + list(r.values())])
        t = schedule(self.N, self.dt, self.dt_sim, self.n_keep, self.t_start, self._k).t_k + self.dt_sim * np.arange(S + 1)
        self._k += periods
        return ROMPCLoopResult(r['x'], r['x_hat'], r['y'], r['z'], r['u'], r['u_bar'], r['x_bar'], r['iters'], r['status'], r['J'], t)

    def step(self, W=None, V=None, X_plant=None, record_x=True):
        return self.run(1, W=W, V=V, X_plant=X_plant, record_x=record_x)

    def last_inputs(self):
        """The solver inputs of the last period: dict x0 (B, n_x), z (B, N + 1, n_z), zf (B, n_z), u (B, N, n_u) (None where the loop has
        none)."""
        B, N = self.B, self.N
        r = dict(x0=np.empty((B, self.n_x)), z=np.empty((B, N + 1, self.n_z)) if self.has_z else None,
                 zf=np.empty((B, self.n_z)) if self.has_zf else None, u=np.empty((B, N, self.n_u)) if self.has_u else None)
        self._call('_last_inputs', *[_lib.dptr(a) for a in r.values()])
        return r

    def _chain(self, xopt, uopt, x0, status, xopt_prev=None, uopt_prev=None, first=False):
        """The chain kernel alone on host arrays (for tests): the QP's answer xopt (B, N+1, n_x), uopt (B, N, n_u), the request's x0
        (B, n_x), status (B,), the previous plan (None when first) -> (xopt_out, uopt_out, x0_next)."""
        B, N = self.B, self.N
        sx, su = (B, N + 1, self.n_x), (B, N, self.n_u)
        f = lambda a, shape: None if a is None else _lib.f64(np.asarray(a).reshape(shape))
        xopt, uopt, x0, xp, up = f(xopt, sx), f(uopt, su), f(x0, (B, self.n_x)), f(xopt_prev, sx), f(uopt_prev, su)
        status = np.ascontiguousarray(np.asarray(status).reshape(B), dtype=np.int32)
        xo, uo, xn = np.empty(sx), np.empty(su), np.empty((B, self.n_x))
        self._call('_chain', _lib.dptr(xp), _lib.dptr(up), _lib.dptr(xopt), _lib.dptr(uopt), _lib.dptr(x0), _lib.iptr(status),
                   C.c_int(1 if first else 0), _lib.dptr(xo), _lib.dptr(uo), _lib.dptr(xn))
        return xo, uo, xn

    def _advance(self, xopt, uopt, x, x_hat, W=None, V=None, X_plant=None):
        """The advance kernel alone on host arrays (for tests): plans, x, x_hat (B, n_x), W (n_replan, B, n_x), V (n_replan, B, n_y),
        X_plant (B, n_replan + 1, n_x) -> dict X, XH (B, n_replan, n_x) and Z after every sub-step, Y, U, Ubar, Xbar of every sub-step.
        The controller's constants are read from the observer at the call."""
        B, N, nk = self.B, self.N, self.n_keep
        f = lambda a, *shape: None if a is None else _lib.f64(np.asarray(a).reshape(shape))
        xopt, uopt = f(xopt, B, N + 1, self.n_x), f(uopt, B, N, self.n_u)
        x, x_hat = f(x, B, self.n_x), f(x_hat, B, self.n_x)
        W, V, X_plant = f(W, nk, B, self.n_x), f(V, nk, B, self.n_y), f(X_plant, B, nk + 1, self.n_x)
        r = dict(X=np.empty((B, nk, self.n_x)), XH=np.empty((B, nk, self.n_x)), Y=np.empty((B, nk, self.n_y)), Z=np.empty((B, nk, self.n_zc)),
                 U=np.empty((B, nk, self.n_u)), Ubar=np.empty((B, nk, self.n_u)), Xbar=np.empty((B, nk, self.n_x)))
        self._call('_advance', *[_lib.dptr(a) for a in [xopt, uopt, x, x_hat, W, V, X_plant] + list(r.values())])
        return r
