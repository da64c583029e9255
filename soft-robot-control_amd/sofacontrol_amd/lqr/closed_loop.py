"""Batched closed-loop iLQR: `batch` loops of tpwl.controllers.ilqr resident on the device (csrc/ilqr_loop.hip, the resident plan of
csrc/lqr.hip).

Every member tracks a per-step policy u = u_bar[k] + K[k] (x - x_bar[k]) (tpwl/controllers.py:199-215) on a TPWL plant pre-discretised at
`dt_sim`: the policy its own iLQR plan has just solved (`plan()`: x, u and above all K, B x N x n_u x n_x doubles, never leave the
device), or an uploaded one (`set_policy`: TrajTracking's TV-LQR gains, or any other).  `run(steps)` is one launch sequence on the
handle's stream and ONE host wait; only the records cross PCIe.

Order of a simulation step s (since the last reset; dt = r dt_sim):
  1. if s % r == 0 controller step j = s / r fires: u = u_bar[row_j] + K[row_j] (xl - x_bar[row_j]), xl the filter's estimate with an
     observer, else the plant state; otherwise the held u
  2. x <- d_d[i] + A_d[i] x + B_d[i] u (+ w_s), i the plant's nearest point to x
  3. z = H x
  4. with an observer: y = (C x + y_ref) + v_s, then one step of every filter with (u, y)
The row: the reference computes step = int(t_step / dt) from a t_step rounded to four decimals, which is not j (at dt = 0.05 the steps
3, 6, 7 read rows 2, 5, 6).  `policy_rows` states that table on the host in float64; the kernel does no time arithmetic.  Where the
reference would raise IndexError (row_j == N) and behind final_time the member applies the idle input u0.

A TrajTracking or ilqr controller of tpwl.controllers goes in unchanged: loop.set_policy(ctrl.x_bar, ctrl.u_bar, ctrl.K) (see
`policy_of`).  Not offered: SSM plants or plans, weighting-mode plants, input clipping, re-planning during a run, the start-up phase
before t_delay."""
import collections
import ctypes as C

import numpy as np

from .. import _lib

ILQRLoopResult = collections.namedtuple('ILQRLoopResult', 'x z u x_hat y ekf_status t')


def policy_rows(N, dt, count=None, final_time=None):
    """The policy row of the controller steps j = 0 .. count-1 (default N + 2: every later step is idle): row_j = int(round(j dt, 4) / dt),
    the expression of tpwl.controllers._tracking_input at the clock's t_step = round(j dt, 4), in float64; -1 (the idle input u0) where
    row_j >= N or round(j dt, 4) > final_time."""
    N, dt = int(N), float(dt)
    count = N + 2 if count is None else int(count)
    rows = np.empty(count, dtype=np.int32)
    for j in range(count):
        t_step = round(j * dt, 4)
        row = int(t_step / dt)
        if row >= N or (final_time is not None and t_step > final_time):
            row = -1
        rows[j] = row
    return rows


def policy_of(ctrl):
    """(x_bar, u_bar, K) of a tpwl.controllers.ilqr / TrajTracking whose policy has been computed, as arrays for `set_policy`."""
    if ctrl.x_bar is None or ctrl.u_bar is None or ctrl.K is None:
        raise RuntimeError('policy_of: the controller has no policy yet (compute_policy has not run)')
    return np.asarray(ctrl.x_bar, dtype=np.float64), np.asarray(ctrl.u_bar, dtype=np.float64), np.asarray(ctrl.K, dtype=np.float64)


class ILQRClosedLoopBatch:
    _sym = 'silqr_loop'

    def __init__(self, policy, plant, dt_sim, batch, z=None, observer=None, u0=None, max_steps_per_run=None, final_time=None):
        """policy: an lqr.ilqr.iLQR on a TPWL model (its dt, model, cost_params, planning_horizon and params make the resident plan);
        plant: a nearest-point TPWLATV with an output model (it may be the policy's own model), stepped at dt_sim; z: the plan's target,
        (N+1, n_z) shared by all members or (B, N+1, n_z) (see set_target); observer: a tpwl.observer.DiscreteEKFObserverBatch of the
        same batch, n_x and n_u (the loop binds it to dt_sim and steps it on its own stream: do not step it elsewhere while the loop is
        in use); u0 (n_u): the idle input; max_steps_per_run: the longest run (sizes the record blocks; default 16 N r); final_time: the
        controller's final_time (None: the policy's last row ends it)."""
        from ..SSM.ssm import SSM
        name = type(self).__name__
        if isinstance(getattr(policy, 'model', None), SSM):
            raise RuntimeError('%s: SSM iLQR plans are not offered by the resident loop' % name)
        if getattr(plant, 'tpwl_method', 'nn') != 'nn':
            raise RuntimeError("%s: weighting-mode plants (tpwl_method = '%s') are not stepped on the device: the plant must be a "
                               "nearest-point TPWL model" % (name, plant.tpwl_method))
        dt = float(policy.dt)
        if not dt_sim > 0 or not dt > 0:
            raise RuntimeError('%s: need dt > 0 and dt_sim > 0' % name)
        ratio = dt / float(dt_sim)
        if abs(ratio - round(ratio)) > 1e-9 or round(ratio) < 1:
            raise RuntimeError('%s: dt / dt_sim = %.12g is not an integer >= 1 (the controller step must be a whole number of simulation '
                               'steps)' % (name, ratio))
        self.B, self.N, self.dt, self.dt_sim, self.r = int(batch), int(policy.planning_horizon), dt, float(dt_sim), int(round(ratio))
        self.n_x, self.n_u = int(policy.state_dim), int(policy.input_dim)
        if self.n_u > 16:
            raise RuntimeError('%s: n_u = %d exceeds the limit n_u <= 16 of the advance kernel' % (name, self.n_u))
        if int(plant.get_state_dim()) > 128:
            raise RuntimeError('%s: the plant\'s n_x = %d exceeds the limit n_x <= 128 of the advance kernel' % (name, plant.get_state_dim()))
        if (int(plant.get_state_dim()), int(plant.get_input_dim())) != (self.n_x, self.n_u):
            raise RuntimeError('%s: the plant has n_x = %d, n_u = %d, the policy n_x = %d, n_u = %d'
                               % (name, plant.get_state_dim(), plant.get_input_dim(), self.n_x, self.n_u))
        if getattr(plant, 'H', None) is None:
            raise RuntimeError('%s: the plant has no output model (z = H x is recorded at every step): set Hf' % name)
        if self.B < 1 or self.N < 1:
            raise RuntimeError('%s: need batch >= 1 and a planning horizon >= 1' % name)
        if observer is not None:
            shape = (getattr(observer, 'batch', None), getattr(observer, 'state_dim', None), getattr(observer, 'input_dim', None))
            if shape != (self.B, self.n_x, self.n_u):
                raise RuntimeError('%s: the observer has batch = %s, n_x = %s, n_u = %s; the loop needs batch = %d, n_x = %d, n_u = %d'
                                   % ((name,) + shape + (self.B, self.n_x, self.n_u)))
        self.policy, self.plant, self.observer = policy, plant, observer      # (kept alive: the handles point into all three)
        self.n_z = int(plant.get_output_dim())
        self.n_y = None if observer is None else int(observer.meas_dim)
        self.max_steps_per_run = int(max_steps_per_run) if max_steps_per_run is not None else 16 * self.N * self.r
        self.final_time = None if final_time is None else float(final_time)
        self._steps = None
        self._h, self._plan = C.c_void_p(), C.c_void_p()
        lib = _lib.lib()
        cp = policy.cost_params
        par = policy._params()
        _lib.check(lib.silqr_plan_create(C.byref(self._plan), policy.model.handle_for(dt), C.c_int(self.N), C.c_int64(self.B),
                                         _lib.dptr(_lib.f64(cp.Q)), _lib.dptr(_lib.f64(cp.R)), _lib.dptr(_lib.f64(cp.Qf)), C.byref(par)),
                   'silqr_plan_create')
        _lib.check(lib.silqr_loop_create(C.byref(self._h), self._plan, plant.handle_for(self.dt_sim), C.c_int(self.N), C.c_int(self.r),
                                         C.c_int64(self.B), C.c_int64(self.max_steps_per_run)), 'silqr_loop_create')
        self.rows = policy_rows(self.N, dt, final_time=self.final_time)
        self._call('_set_rows', _lib.iptr(self.rows), C.c_int64(len(self.rows)))
        self.u0 = _lib.f64(np.zeros(self.n_u) if u0 is None else np.asarray(u0).reshape(self.n_u))
        self._call('_set_idle_input', _lib.dptr(self.u0))
        if observer is not None:
            observer.bind(self.dt_sim)
            self._call('_set_observer', observer._h)
        if z is not None:
            self.set_target(z)

    def _call(self, entry, *args):
        _lib.check(getattr(_lib.lib(), self._sym + entry)(self._h, *args), self._sym + entry)

    def __del__(self):
        try:
            lib = _lib.lib()
            if self._h:
                lib.silqr_loop_destroy(self._h)
                self._h = C.c_void_p()
            if self._plan:
                lib.silqr_plan_destroy(self._plan)
                self._plan = C.c_void_p()
        except Exception:
            pass

    def _shaped(self, what, a, shape):
        a = np.asarray(a)
        if a.shape != shape:
            raise RuntimeError('%s: %s must have shape %s, got %s' % (type(self).__name__, what, shape, a.shape))
        return _lib.f64(a)

    def set_target(self, z):
        """The plan's target: (N+1, n_z) shared by all members (it crosses PCIe once and is replicated on the device) or (B, N+1, n_z);
        absolute, as iLQR.set_target's."""
        z = np.asarray(z)
        shared = z.ndim == 2
        z = self._shaped('z', z, (self.N + 1, self.n_z) if shared else (self.B, self.N + 1, self.n_z))
        _lib.check(_lib.lib().silqr_plan_set_target(self._plan, _lib.dptr(z), C.c_int(1 if shared else 0)), 'silqr_plan_set_target')

    def set_policy(self, x_bar, u_bar, K):
        """Install a policy: x_bar (N+1, n_x), u_bar (N, n_u), K (N, n_u, n_x) shared by all members, or each with a leading B."""
        N, n, m = self.N, self.n_x, self.n_u
        shared = np.ndim(x_bar) == 2
        lead = () if shared else (self.B,)
        x_bar = self._shaped('x_bar', x_bar, lead + (N + 1, n))
        u_bar = self._shaped('u_bar', u_bar, lead + (N, m))
        K = self._shaped('K', K, lead + (N, m, n))
        self._call('_set_policy', _lib.dptr(x_bar), _lib.dptr(u_bar), _lib.dptr(K), C.c_int(1 if shared else 0))

    def reset(self, x0, x_hat0=None):
        """Plant states x0 (B, n_x); the step counter returns to 0 and every member holds u0.  With an observer the estimates start at
        x_hat0 (None: x0) -- the caller's statement of where the reference's first observer.update leaves the filters -- and the
        covariances are re-installed from Sigma0."""
        x0 = self._shaped('x0', x0, (self.B, self.n_x))
        if x_hat0 is not None:
            if self.observer is None:
                raise RuntimeError('%s.reset: x_hat0 given but the loop has no observer' % type(self).__name__)
            x_hat0 = self._shaped('x_hat0', x_hat0, (self.B, self.n_x))
        self._call('_reset', _lib.dptr(x0), _lib.dptr(x_hat0))
        self._steps = 0

    def plan(self, u_warmstart=None):
        """Solve the members' iLQR problems from their beliefs where they stand on the device (the estimates with an observer, else the
        plant states); the solution becomes the policy in place.  u_warmstart (B, N, n_u) or None; u_last is the policy object's."""
        uw = None if u_warmstart is None else _lib.f64(np.broadcast_to(u_warmstart, (self.B, self.N, self.n_u)))
        ul = _lib.f64(np.broadcast_to(self.policy.u_last, (self.B, self.n_u)))
        _lib.check(_lib.lib().silqr_plan_set_u_last(self._plan, _lib.dptr(ul)), 'silqr_plan_set_u_last')
        self._call('_plan', _lib.dptr(uw))

    def run(self, steps, W=None, V=None, record_x=True):
        """`steps` simulation steps from where the last run ended.  W (steps, B, n_x): added to the plant's next state; V (steps, B, n_y):
        measurement noise (with an observer).  Returns ILQRLoopResult: x (B, steps + 1, n_x) or None, z (B, steps + 1, n_z) -- row 0
        where the run started --, u (B, steps, n_u); with an observer x_hat (B, steps + 1, n_x), y (B, steps, n_y), ekf_status (B,) the
        OR of the run's filter statuses, else None; t (steps + 1,) the times of the rows since the reset."""
        steps = int(steps)
        B = self.B
        fits = 1 <= steps <= self.max_steps_per_run                      # (what does not fit is refused by the library: it is handed dummies)
        S = steps if fits else 0
        obs = self.observer is not None
        if V is not None and not obs:
            raise RuntimeError('%s.run: V given but the loop has no observer' % type(self).__name__)
        W = None if W is None or not fits else self._shaped('W', W, (S, B, self.n_x))
        V = None if V is None or not fits else self._shaped('V', V, (S, B, self.n_y))
        f64 = lambda *shape: np.empty(shape if fits else 1)
        x = f64(B, S + 1, self.n_x) if record_x else None
        z, u = f64(B, S + 1, self.n_z), f64(B, S, self.n_u)
        xh = f64(B, S + 1, self.n_x) if obs else None
        y = f64(B, S, self.n_y) if obs else None
        es = np.empty(B, dtype=np.int32) if obs else None
        self._call('_run', C.c_int64(steps), _lib.dptr(W), _lib.dptr(V), _lib.dptr(x), _lib.dptr(z), _lib.dptr(u), _lib.dptr(xh), _lib.dptr(y),
                   _lib.iptr(es))
        t = self.dt_sim * (self._steps + np.arange(steps + 1))
        self._steps += steps
        return ILQRLoopResult(x, z, u, xh, y, es, t)

    def last_policy(self):
        """(x_bar, u_bar, K) in use, in the shape they were installed: with a leading B after plan() or a per-member set_policy."""
        N, n, m = self.N, self.n_x, self.n_u
        shared = C.c_int(0)
        self._call('_last_policy', None, None, None, C.byref(shared))
        lead = () if shared.value else (self.B,)
        xb, ub, K = np.empty(lead + (N + 1, n)), np.empty(lead + (N, m)), np.empty(lead + (N, m, n))
        self._call('_last_policy', _lib.dptr(xb), _lib.dptr(ub), _lib.dptr(K), None)
        return xb, ub, K

    def plan_info(self):
        """{'cost' (B,), 'iters' (B,)} of the last plan()."""
        cost, iters = np.empty(self.B), np.empty(self.B, dtype=np.int32)
        self._call('_plan_info', _lib.dptr(cost), _lib.iptr(iters))
        return {'cost': cost, 'iters': iters}

    def stats(self):
        steps, waits = C.c_int64(0), C.c_int64(0)
        self._call('_stats', C.byref(steps), C.byref(waits))
        return {'steps': steps.value, 'waits_last_run': waits.value}

    def _advance(self, x, steps, step0=0, u_held=None, W=None):
        """The advance kernel alone under the policy in use (for tests; no observer): plant states x (B, n_x), `steps` steps with the step
        counter starting at step0, held inputs u_held (B, n_u; None: u0), W (steps, B, n_x) -> X (B, steps, n_x), Z, U and the plant's
        picks idx (B, steps).  The loop's own state is not touched."""
        B, S = self.B, int(steps)
        x = self._shaped('x', x, (B, self.n_x))
        u_held = None if u_held is None else self._shaped('u_held', u_held, (B, self.n_u))
        W = None if W is None else self._shaped('W', W, (S, B, self.n_x))
        X, Z, U = np.empty((B, S, self.n_x)), np.empty((B, S, self.n_z)), np.empty((B, S, self.n_u))
        idx = np.empty((B, S), dtype=np.int32)
        self._call('_advance', _lib.dptr(x), _lib.dptr(u_held), C.c_int64(S), C.c_int64(int(step0)), _lib.dptr(W), _lib.dptr(X), _lib.dptr(Z),
                   _lib.dptr(U), _lib.iptr(idx))
        return X, Z, U, idx
