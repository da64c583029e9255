"""Batched closed-loop GuSTO on SSM models: `batch` receding-horizon loops resident on the device (csrc/gusto_ssm_loop.hip).

Every rollout of a resident SSM `GuSTO(batch=B)` is its own loop of the reference's hardware driver (examples/hardware/diamond_SSM.py:
353-361): plan, apply `n_keep` inputs u = u_bar(t) of the plan to an SSM plant stepped at `dt_sim` (SSM/controllers.py:204, 237: no
feedback gain), measure y = (C_plant(x) + z_ref_plant) + v, estimate x_hat = W_map(y - z_ref) with the CONTROLLER's model (SSMObserver:
a polynomial map, no filter), shift the plan (scp/ros.py:110-114), re-plan from the estimate.  `run(periods)` is one launch sequence on
the handle's stream and ONE host wait; only the records of the run cross PCIe.  The times of a period are those of the TPWL loop:
`closed_loop.schedule`."""
import ctypes as C

import numpy as np

from .. import _lib
from .closed_loop import ClosedLoopResult, schedule

_MODES = {'fe': 1, 'be': 2, 'bil': 3}


def _plant_mode(plant):
    """The discretisation the plant is stepped in: its discrete map (4) or its discr_method (1 fe, 2 be, 3 bil)."""
    if getattr(plant, 'discrete', False):
        return 4
    if plant.discr_method not in _MODES:
        raise RuntimeError('SSMClosedLoopBatch: the plant\'s discr_method must be in [fe, be, bil] (or the plant discrete)')
    return _MODES[plant.discr_method]


class SSMClosedLoopBatch:
    def __init__(self, gusto, plant, dt_sim, n_keep, t=None, z=None, u=None, phase=None, observe=True, max_steps_per_run=None):
        """gusto: a GuSTO on an SSMGuSTO model with batch=B whose SSM plan is resident; plant: an SSMDynamics of the same n_x, n_u and n_o
        (it may be the planner's own dyn_sys, or another model), stepped at dt_sim in its own discretisation (fe, be, bil, or its discrete
        map); n_keep: plant steps per period.  t (T,), z (T, n_z), u (T, n_u): the target table, z in the shifted coordinates the solver
        takes (zfyf_to_zy); phase (B,): a time offset of every loop's target.  observe: plans start from the estimate (True, the
        reference's loop) or from the plant state (False, perfect state feedback); the measurement and the estimate are recorded either
        way.  max_steps_per_run: the longest run in plant steps (sizes the record blocks; default 16 periods)."""
        if not getattr(gusto, '_ssm', False):
            raise RuntimeError('SSMClosedLoopBatch needs a GuSTO on an SSMGuSTO model whose SSM plan is resident on the device (not a TPWL plan -- '
                               'that is ClosedLoopBatch -- and not the host loop): there is no device solve to chain otherwise')
        if getattr(gusto, '_rate_rows', 0):
            raise RuntimeError('SSMClosedLoopBatch: the plan has %d input-rate rows (dU): a rollout whose trust region binds under them returns '
                               'status -78 for the host loop, which a loop resident on the device cannot serve' % gusto._rate_rows)
        n_keep = int(n_keep)
        if n_keep < 1 or not dt_sim > 0:
            raise RuntimeError('SSMClosedLoopBatch: need n_keep >= 1 and dt_sim > 0')
        if n_keep * float(dt_sim) > gusto.N * float(gusto.dt):
            raise RuntimeError('SSMClosedLoopBatch: n_keep * dt_sim = %g exceeds the horizon N * dt = %g (the shift of the previous plan '
                               'would find no row)' % (n_keep * float(dt_sim), gusto.N * float(gusto.dt)))
        self.gusto, self.plant = gusto, plant                      # (kept alive: the handle points into both)
        self.B, self.N, self.dt = gusto.batch, gusto.N, float(gusto.dt)
        self.n_x, self.n_u, self.n_z = gusto.n_x, gusto.n_u, gusto.n_z
        self.n_o = plant.output_dim
        self.dt_sim, self.n_keep, self.observe = float(dt_sim), n_keep, bool(observe)
        self.max_steps_per_run = int(max_steps_per_run) if max_steps_per_run is not None else 16 * n_keep
        self.has_z, self.has_u = z is not None, u is not None
        self.t_start, self._k = 0.0, None
        self._h = C.c_void_p()
        lib = _lib.lib()
        _lib.check(lib.sgusto_ssm_loop_create(C.byref(self._h), gusto.plan, gusto.model.dyn_sys.handle, plant.handle, C.c_int(_plant_mode(plant)),
                                              C.c_double(self.dt_sim), C.c_int(n_keep), C.c_int(1 if self.observe else 0),
                                              C.c_int64(self.max_steps_per_run)), 'sgusto_ssm_loop_create')
        if z is not None or u is not None:
            if t is None:
                raise RuntimeError('SSMClosedLoopBatch: a target table needs its times t')
            t = _lib.f64(np.asarray(t).reshape(-1))
            T = t.shape[0]
            z = None if z is None else _lib.f64(np.asarray(z).reshape(T, self.n_z))
            u = None if u is None else _lib.f64(np.asarray(u).reshape(T, self.n_u))
            phase = None if phase is None else _lib.f64(np.asarray(phase).reshape(self.B))
            _lib.check(lib.sgusto_ssm_loop_set_target(self._h, C.c_int(T), _lib.dptr(t), _lib.dptr(z), _lib.dptr(u), _lib.dptr(phase)),
                       'sgusto_ssm_loop_set_target')

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sgusto_ssm_loop_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _shaped(self, what, a, shape):
        """`a` as a contiguous float64 array of exactly `shape` (None passes through)."""
        if a is None:
            return None
        a = np.asarray(a)
        if a.shape != shape:
            raise RuntimeError('SSMClosedLoopBatch: %s must have shape %s, got %s' % (what, shape, a.shape))
        return _lib.f64(a)

    def reset(self, x0, t_start=0.0, v0=None):
        """Plant states x0 (B, n_x) at t_start; v0 (B, n_o): the noise of the first measurement.  The device forms row 0 of the records:
        x0, C_plant(x0), y0 = (C_plant(x0) + z_ref_plant) + v0 and x_hat0 = W_map(y0 - z_ref) -- the reference's first observer.update
        before its first compute_policy."""
        v0 = self._shaped('v0 (B, n_o)', v0, (self.B, self.n_o))
        x0 = _lib.f64(np.asarray(x0).reshape(self.B, self.n_x))
        _lib.check(_lib.lib().sgusto_ssm_loop_reset(self._h, _lib.dptr(x0), _lib.dptr(v0), C.c_double(float(t_start))), 'sgusto_ssm_loop_reset')
        self.t_start, self._k = float(t_start), 0

    def run(self, periods, W=None, V=None, record_x=True):
        """`periods` periods from where the last run ended.  W (periods, n_keep, B, n_x): added to the plant's next state; V (periods,
        n_keep, B, n_o): added to the measurement.  Returns a ClosedLoopResult with x (B, S + 1, n_x) or None, z, y (B, S + 1, n_o),
        x_hat (B, S + 1, n_x), u (B, S, n_u), S = periods n_keep, row 0 where the run started; iters, status, J (periods, B); t."""
        periods = int(periods)
        B, S = self.B, periods * self.n_keep
        W = self._shaped('W (periods, n_keep, B, n_x)', W, (periods, self.n_keep, B, self.n_x))
        V = self._shaped('V (periods, n_keep, B, n_o)', V, (periods, self.n_keep, B, self.n_o))
        if periods >= 1 and S <= self.max_steps_per_run:       # (what does not fit is refused by the library, with its message)
            x = np.empty((B, S + 1, self.n_x)) if record_x else None
            z, y, xh = np.empty((B, S + 1, self.n_o)), np.empty((B, S + 1, self.n_o)), np.empty((B, S + 1, self.n_x))
            u = np.empty((B, S, self.n_u))
            iters, status = np.empty((periods, B), dtype=np.int32), np.empty((periods, B), dtype=np.int32)
            J = np.empty((periods, B))
        else:
            x = W = V = None
            z = y = xh = u = J = np.empty(1)
            iters = status = np.empty(1, dtype=np.int32)
        lib = _lib.lib()
        _lib.check(lib.sgusto_ssm_plan_set_max_iters(self.gusto.plan, C.c_int(int(self.gusto.max_gusto_iters))), 'set_max_iters')
        _lib.check(lib.sgusto_ssm_loop_run(self._h, C.c_int(periods), _lib.dptr(W), _lib.dptr(V), _lib.dptr(x), _lib.dptr(z), _lib.dptr(u),
                                           _lib.dptr(y), _lib.dptr(xh), _lib.iptr(iters), _lib.iptr(status), _lib.dptr(J)), 'sgusto_ssm_loop_run')
        t = schedule(self.N, self.dt, self.dt_sim, self.n_keep, self.t_start, self._k).t_k + self.dt_sim * np.arange(S + 1)
        self._k += periods
        return ClosedLoopResult(x, z, u, iters, status, J, t, x_hat=xh, y=y)

    def step(self):
        return self.run(1)

    def last_inputs(self):
        """The solver inputs of the last period: dict x0, u_init, x_init, z, u (None where the loop has none)."""
        B, N = self.B, self.N
        x0, ui, xi = np.empty((B, self.n_x)), np.empty((B, N, self.n_u)), np.empty((B, N + 1, self.n_x))
        z = np.empty((B, N + 1, self.n_z)) if self.has_z else None
        ud = np.empty((B, N, self.n_u)) if self.has_u else None
        _lib.check(_lib.lib().sgusto_ssm_loop_last_inputs(self._h, _lib.dptr(x0), _lib.dptr(ui), _lib.dptr(xi), _lib.dptr(z), _lib.dptr(ud)),
                   'sgusto_ssm_loop_last_inputs')
        return dict(x0=x0, u_init=ui, x_init=xi, z=z, u=ud)

    def last_plan(self):
        xo, uo = np.empty((self.B, self.N + 1, self.n_x)), np.empty((self.B, self.N, self.n_u))
        _lib.check(_lib.lib().sgusto_ssm_loop_last_plan(self._h, _lib.dptr(xo), _lib.dptr(uo)), 'sgusto_ssm_loop_last_plan')
        return xo, uo

    def stats(self):
        steps, waits = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.lib().sgusto_ssm_loop_stats(self._h, C.byref(steps), C.byref(waits)), 'sgusto_ssm_loop_stats')
        return {'steps': steps.value, 'waits_last_run': waits.value}


def advance(plant, observer_model, dt_sim, N, j, theta, uopt, x, W=None, V=None, xopt=None):
    """sgusto_ssm_loop_advance: the advance kernel alone on host arrays, without a plan or a loop (for tests).  plant, observer_model:
    SSMDynamics; j, theta (n_keep): the schedule; uopt (B, N, n_u), x (B, n_x), W (n_keep, B, n_x), V (n_keep, B, n_o) ->
    dict X, Xhat (B, n_keep, n_x), Z, Y (B, n_keep, n_o), U (B, n_keep, n_u)."""
    uopt = _lib.f64(np.asarray(uopt))
    B, n, m, no, nk = uopt.shape[0], plant.state_dim, plant.input_dim, plant.output_dim, len(j)
    uopt = _lib.f64(uopt.reshape(B, N, m)); x = _lib.f64(np.asarray(x).reshape(B, n))
    xopt = None if xopt is None else _lib.f64(np.asarray(xopt).reshape(B, N + 1, n))
    W = None if W is None else _lib.f64(np.asarray(W).reshape(nk, B, n))
    V = None if V is None else _lib.f64(np.asarray(V).reshape(nk, B, no))
    j = np.ascontiguousarray(j, dtype=np.int32); theta = _lib.f64(np.asarray(theta).reshape(nk))
    X, Xh, Z, Y, U = np.empty((B, nk, n)), np.empty((B, nk, n)), np.empty((B, nk, no)), np.empty((B, nk, no)), np.empty((B, nk, m))
    _lib.check(_lib.lib().sgusto_ssm_loop_advance(plant.handle, C.c_int(_plant_mode(plant)), observer_model.handle, C.c_double(float(dt_sim)),
                                                  C.c_int(int(N)), C.c_int(nk), C.c_int64(B), _lib.iptr(j), _lib.dptr(theta), _lib.dptr(xopt),
                                                  _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W), _lib.dptr(V), _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U),
                                                  _lib.dptr(Y), _lib.dptr(Xh)), 'sgusto_ssm_loop_advance')
    return dict(X=X, Z=Z, U=U, Y=Y, Xhat=Xh)
