"""Batched closed-loop GuSTO on SSM models: `batch` receding-horizon loops resident on the device (csrc/gusto_ssm_loop.hip).

Every rollout of a resident SSM `GuSTO(batch=B)` is its own loop of the reference's hardware driver (examples/hardware/diamond_SSM.py:
353-361): plan, apply `n_keep` inputs u = u_bar(t) of the plan to an SSM plant stepped at `dt_sim` (SSM/controllers.py:204, 237: no
feedback gain), measure y = (C_plant(x) + z_ref_plant) + v, estimate x_hat = W_map(y - z_ref) with the CONTROLLER's model (SSMObserver:
a polynomial map, no filter), shift the plan (scp/ros.py:110-114), re-plan from the estimate.  `run(periods)` is one launch sequence on
the handle's stream and ONE host wait; only the records of the run cross PCIe.  The times of a period are those of the TPWL loop:
`closed_loop.schedule`.

The plant may also be a nearest-point TPWL model of more states than the SSM model, of which the controller sees only the measured tip
y = (C x + y_ref) + v (the reference's drivers): `SSMClosedLoopBatch.on_plant(..., C=, y_ref=)`, `advance_tpwl`.

Behind `set_reproject(Polyhedron(A, b, with_reproject=True))` (either plant kind) every measurement that lies outside Y -- the reset's first one included
-- is replaced by its Euclidean projection before the observer map reads it (SSM/controllers.py:96-97), inside the advance kernel, by the
device function behind Polyhedron.project_to_polyhedron: the same bits.  The result's `y` stays the raw measurement, `y_used` is what the
map read and `proj` its status word: 0 inside (bit for bit), 1 projected, -1 no certified projection (an empty Y), -2 the sample is not
finite; with -1 and -2 the raw sample is used and the run goes on."""
import ctypes
import ctypes as C

import numpy as np

from .. import _lib
from .closed_loop import ClosedLoopResult, _LoopBatch, schedule          # noqa: F401  (the result type and the one schedule, under this name too)

_MODES = {'fe': 1, 'be': 2, 'bil': 3}


def _plant_mode(plant):
    """The discretisation the plant is stepped in: its discrete map (4) or its discr_method (1 fe, 2 be, 3 bil)."""
    if getattr(plant, 'discrete', False):
        return 4
    if plant.discr_method not in _MODES:
        raise RuntimeError('SSMClosedLoopBatch: the plant\'s discr_method must be in [fe, be, bil] (or the plant discrete)')
    return _MODES[plant.discr_method]


class SSMClosedLoopBatch(_LoopBatch):
    _sym, _max_iters = 'sgusto_ssm_loop', 'sgusto_ssm_plan_set_max_iters'

    def __init__(self, gusto, plant, dt_sim, n_keep, t=None, z=None, u=None, phase=None, observe=True, max_steps_per_run=None):
        """gusto: a GuSTO on an SSMGuSTO model with batch=B whose SSM plan is resident; plant: an SSMDynamics of the same n_x, n_u and n_o
        (it may be the planner's own dyn_sys, or another model), stepped at dt_sim in its own discretisation (fe, be, bil, or its discrete
        map); n_keep: plant steps per period.  t (T,), z (T, n_z), u (T, n_u): the target table, z in the shifted coordinates the solver
        takes (zfyf_to_zy); phase (B,): a time offset of every loop's target.  observe: plans start from the estimate (True, the
        reference's loop) or from the plant state (False, perfect state feedback); the measurement and the estimate are recorded either
        way.  max_steps_per_run: the longest run in plant steps (sizes the record blocks; default 16 periods).  The admissible set of
        the measurements is set behind the constructor: set_reproject(Y) (refused with observe=False: no measurement is read there).
        A nearest-point TPWL plant needs its measurement as well: SSMClosedLoopBatch.on_plant(..., C=, y_ref=)."""
        self._build(gusto, plant, dt_sim, n_keep, t, z, u, phase, observe, max_steps_per_run, None, None)

    @classmethod
    def on_plant(cls, gusto, plant, dt_sim, n_keep, t=None, z=None, u=None, phase=None, observe=True, max_steps_per_run=None, C=None, y_ref=None):
        """The constructor with the plant's measurement: every argument of SSMClosedLoopBatch(...), then C (n_o, n_plant) and y_ref (n_o,).
        plant may be a nearest-point TPWL model (a TPWLATV, taken through plant.handle_for(dt_sim)) of n_plant <= 128 states and the plan's
        n_u: the loop steps it by the TPWL step rule, measures y = (C x + y_ref) + v and estimates x_hat = W_map(y - z_ref) with the
        planner's model, whose n_o is C's row count.  reset then takes x0 (B, n_plant), run takes W (periods, n_keep, B, n_plant) and
        returns x (B, S + 1, n_plant); z is C x.  The plans always start from the estimate (observe=False is refused: the plant state is
        not the planner's state).  With an SSM plant C and y_ref are refused: its measurement is its own map."""
        self = cls.__new__(cls)
        self._build(gusto, plant, dt_sim, n_keep, t, z, u, phase, observe, max_steps_per_run, C, y_ref)
        return self

    _n_meas = 'n_o'

    def _check_reproject_allowed(self, Yab):
        if Yab is not None and not self.observe:
            raise RuntimeError('SSMClosedLoopBatch: Y together with observe=False is refused: the plans start from the plant state, no '
                               'measurement is read, a Y would change nothing')

    def _build(self, gusto, plant, dt_sim, n_keep, t, z, u, phase, observe, max_steps_per_run, Cm, y_ref):
        if not getattr(gusto, '_ssm', False):
            raise RuntimeError('SSMClosedLoopBatch needs a GuSTO on an SSMGuSTO model whose SSM plan is resident on the device (not a TPWL plan -- '
                               'that is ClosedLoopBatch -- and not the host loop): there is no device solve to chain otherwise')
        if getattr(gusto, '_rate_rows', 0):
            raise RuntimeError('SSMClosedLoopBatch: the plan has %d input-rate rows (dU): a rollout whose trust region binds under them returns '
                               'status -78 for the host loop, which a loop resident on the device cannot serve' % gusto._rate_rows)
        n_keep = self._check_periods(gusto, dt_sim, n_keep)
        if hasattr(plant, 'handle_for'):
            return self._build_on_tpwl(gusto, plant, dt_sim, n_keep, t, z, u, phase, observe, max_steps_per_run, Cm, y_ref)
        if Cm is not None or y_ref is not None:
            raise RuntimeError('SSMClosedLoopBatch: C and y_ref belong to a TPWL plant; an SSM plant is measured by its own map '
                               '(y = C_plant(x) + z_ref_plant)')
        self.gusto, self.plant = gusto, plant                      # (kept alive: the handle points into both)
        self._shape(gusto, dt_sim, n_keep, max_steps_per_run, z, u)
        self.n_o, self.observe = plant.output_dim, bool(observe)
        lib = _lib.lib()
        _lib.check(lib.sgusto_ssm_loop_create(C.byref(self._h), gusto.plan, gusto.model.dyn_sys.handle, plant.handle, C.c_int(_plant_mode(plant)),
                                              C.c_double(self.dt_sim), C.c_int(n_keep), C.c_int(1 if self.observe else 0),
                                              C.c_int64(self.max_steps_per_run)), 'sgusto_ssm_loop_create')
        self._set_target(t, z, u, phase)

    def _build_on_tpwl(self, gusto, plant, dt_sim, n_keep, t, z, u, phase, observe, max_steps_per_run, Cm, y_ref):
        """The loop on a nearest-point TPWL plant (sgusto_ssm_loop_create_tpwl); the refusals come before any device call."""
        if getattr(plant, 'tpwl_method', 'nn') != 'nn':
            raise RuntimeError("SSMClosedLoopBatch: weighting-mode plants (tpwl_method = '%s') are not stepped on the device: the plant must be "
                               "a nearest-point TPWL model" % plant.tpwl_method)
        if not observe:
            raise RuntimeError('SSMClosedLoopBatch: observe=False is not offered on a TPWL plant: the plant state is not the planner\'s state '
                               '(the plans start from the estimate)')
        if Cm is None or y_ref is None:
            raise RuntimeError('SSMClosedLoopBatch: a TPWL plant needs its measurement C (n_o, n_plant) and y_ref (n_o,): '
                               'SSMClosedLoopBatch.on_plant(..., C=, y_ref=)')
        n_plant, n_o = int(plant.get_state_dim()), int(gusto.model.dyn_sys.output_dim)
        if n_plant > 128:
            raise RuntimeError('SSMClosedLoopBatch: the plant\'s n_x = %d exceeds the limit n_x <= 128 of the advance kernel' % n_plant)
        if int(plant.get_input_dim()) != int(gusto.n_u):
            raise RuntimeError('SSMClosedLoopBatch: the plant has n_u = %d, the plan n_u = %d' % (plant.get_input_dim(), gusto.n_u))
        if np.shape(Cm) != (n_o, n_plant):
            raise RuntimeError('SSMClosedLoopBatch: C must have shape (n_o, n_plant) = %s, got %s' % ((n_o, n_plant), np.shape(Cm)))
        if np.shape(y_ref) != (n_o,):
            raise RuntimeError('SSMClosedLoopBatch: y_ref must have shape (n_o,) = %s, got %s' % ((n_o,), np.shape(y_ref)))
        self.gusto, self.plant = gusto, plant                      # (kept alive: the handle points into both)
        self._shape(gusto, dt_sim, n_keep, max_steps_per_run, z, u)
        self.n_o, self.observe, self.n_plant = n_o, True, n_plant
        self._C, self._yref = _lib.f64(Cm), _lib.f64(y_ref)
        _lib.check(_lib.lib().sgusto_ssm_loop_create_tpwl(C.byref(self._h), gusto.plan, gusto.model.dyn_sys.handle, plant.handle_for(self.dt_sim),
                                                          _lib.dptr(self._C), _lib.dptr(self._yref), C.c_int(n_o), C.c_double(self.dt_sim),
                                                          C.c_int(n_keep), C.c_int64(self.max_steps_per_run)), 'sgusto_ssm_loop_create_tpwl')
        self._set_target(t, z, u, phase)

    n_plant = None                                                 # states of a TPWL plant (None: an SSM plant of the planner's n_x)

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
        before its first compute_policy.  On a TPWL plant x0 is (B, n_plant) and the first measurement is (C x0 + y_ref) + v0."""
        v0 = self._shaped('v0 (B, n_o)', v0, (self.B, self.n_o))
        if self.n_plant is not None:
            x0 = self._shaped('x0 (B, n_plant)', x0, (self.B, self.n_plant))
        else:
            x0 = _lib.f64(np.asarray(x0).reshape(self.B, self.n_x))
        self._call('_reset', _lib.dptr(x0), _lib.dptr(v0), C.c_double(float(t_start)))
        self.t_start, self._k = float(t_start), 0

    def run(self, periods, W=None, V=None, record_x=True):
        """`periods` periods from where the last run ended.  W (periods, n_keep, B, n_x): added to the plant's next state; V (periods,
        n_keep, B, n_o): added to the measurement.  Returns a ClosedLoopResult with x (B, S + 1, n_x) or None, z, y (B, S + 1, n_o),
        x_hat (B, S + 1, n_x), u (B, S, n_u), S = periods n_keep, row 0 where the run started; iters, status, J (periods, B); t.
        On a TPWL plant W and x have n_plant columns.  With a Y also y_used (B, S + 1, n_o) and proj (B, S + 1) int32 (y stays raw)."""
        periods = int(periods)
        if self.n_plant is not None:
            W = self._shaped('W (periods, n_keep, B, n_plant)', W, (periods, self.n_keep, self.B, self.n_plant))
        else:
            W = self._shaped('W (periods, n_keep, B, n_x)', W, (periods, self.n_keep, self.B, self.n_x))
        V = self._shaped('V (periods, n_keep, B, n_o)', V, (periods, self.n_keep, self.B, self.n_o))
        fits, r = self._records(periods, record_x, self.n_o, y=(1, self.n_o), x_hat=(1, self.n_x))
        if self.n_plant is not None and r['x'] is not None:
            r['x'] = np.empty((self.B, periods * self.n_keep + 1, self.n_plant))
        if not fits:
            W = V = None
        names = ('x', 'z', 'u', 'y', 'x_hat', 'iters', 'status', 'J')
        if self._Y is not None:
            S = periods * self.n_keep
            r['y_used'] = np.empty((self.B, S + 1, self.n_o) if fits else 1)
            r['proj'] = np.empty((self.B, S + 1) if fits else 1, dtype=np.int32)
            return self._run('_run_reprojected', periods, [W, V] + [r[k] for k in names + ('y_used', 'proj')], r)
        return self._run('_run', periods, [W, V] + [r[k] for k in names], r)


def _Y_arrays(who, Y, n_o):
    """(A, b, rows) of a Y handed to a stand-alone advance entry, checked as the loops check it."""
    class _Named(_LoopBatch):
        pass
    _Named.__name__ = who
    A, b = _Named._check_reproject(Y, int(n_o))
    return A, b, A.shape[0]


def advance(plant, observer_model, dt_sim, N, j, theta, uopt, x, W=None, V=None, xopt=None, Y=None):
    """sgusto_ssm_loop_advance: the advance kernel alone on host arrays, without a plan or a loop (for tests).  plant, observer_model:
    SSMDynamics; j, theta (n_keep): the schedule; uopt (B, N, n_u), x (B, n_x), W (n_keep, B, n_x), V (n_keep, B, n_o) ->
    dict X, Xhat (B, n_keep, n_x), Z, Y (B, n_keep, n_o), U (B, n_keep, n_u).  With Y (a Polyhedron(with_reproject=True)) the
    measurements pass through it (sgusto_ssm_loop_advance_reprojected): also Y_used (B, n_keep, n_o) and proj (B, n_keep) int32."""
    uopt = _lib.f64(np.asarray(uopt))
    B, n, m, no, nk = uopt.shape[0], plant.state_dim, plant.input_dim, plant.output_dim, len(j)
    uopt = _lib.f64(uopt.reshape(B, N, m)); x = _lib.f64(np.asarray(x).reshape(B, n))
    xopt = None if xopt is None else _lib.f64(np.asarray(xopt).reshape(B, N + 1, n))
    W = None if W is None else _lib.f64(np.asarray(W).reshape(nk, B, n))
    V = None if V is None else _lib.f64(np.asarray(V).reshape(nk, B, no))
    j = np.ascontiguousarray(j, dtype=np.int32); theta = _lib.f64(np.asarray(theta).reshape(nk))
    if Y is not None:
        YA, Yb, yrows = _Y_arrays('advance', Y, no)
        X, Xh, Z, Ym, U = np.empty((B, nk, n)), np.empty((B, nk, n)), np.empty((B, nk, no)), np.empty((B, nk, no)), np.empty((B, nk, m))
        Yu, pj = np.empty((B, nk, no)), np.empty((B, nk), dtype=np.int32)
        _lib.check(_lib.lib().sgusto_ssm_loop_advance_reprojected(
            plant.handle, C.c_int(_plant_mode(plant)), observer_model.handle, C.c_double(float(dt_sim)), C.c_int(int(N)), C.c_int(nk), C.c_int64(B),
            _lib.iptr(j), _lib.dptr(theta), _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W), _lib.dptr(V), _lib.dptr(YA), _lib.dptr(Yb), C.c_int(yrows),
            _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U), _lib.dptr(Ym), _lib.dptr(Xh), _lib.dptr(Yu), _lib.iptr(pj)), 'sgusto_ssm_loop_advance_reprojected')
        return dict(X=X, Z=Z, U=U, Y=Ym, Xhat=Xh, Y_used=Yu, proj=pj)
    X, Xh, Z, Y, U = np.empty((B, nk, n)), np.empty((B, nk, n)), np.empty((B, nk, no)), np.empty((B, nk, no)), np.empty((B, nk, m))
    _lib.check(_lib.lib().sgusto_ssm_loop_advance(plant.handle, C.c_int(_plant_mode(plant)), observer_model.handle, C.c_double(float(dt_sim)),
                                                  C.c_int(int(N)), C.c_int(nk), C.c_int64(B), _lib.iptr(j), _lib.dptr(theta), _lib.dptr(xopt),
                                                  _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W), _lib.dptr(V), _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U),
                                                  _lib.dptr(Y), _lib.dptr(Xh)), 'sgusto_ssm_loop_advance')
    return dict(X=X, Z=Z, U=U, Y=Y, Xhat=Xh)


def advance_tpwl_reprojected(plant, C, y_ref, observer_model, dt_sim, N, j, theta, uopt, x, Y, W=None, V=None):
    """advance_tpwl with the admissible set Y of the measurements (sgusto_ssm_loop_advance_tpwl_reprojected): also Y_used (B, n_keep, n_o)
    and proj (B, n_keep) int32."""
    return _advance_tpwl(plant, C, y_ref, observer_model, dt_sim, N, j, theta, uopt, x, W, V, Y)


def advance_tpwl(plant, C, y_ref, observer_model, dt_sim, N, j, theta, uopt, x, W=None, V=None):
    """sgusto_ssm_loop_advance_tpwl: the TPWL-plant advance kernel alone on host arrays (for tests; the arrays are those of _advance_tpwl)."""
    return _advance_tpwl(plant, C, y_ref, observer_model, dt_sim, N, j, theta, uopt, x, W, V, None)


def _advance_tpwl(plant, C, y_ref, observer_model, dt_sim, N, j, theta, uopt, x, W, V, Y):
    """sgusto_ssm_loop_advance_tpwl: the TPWL-plant advance kernel alone on host arrays, without a plan or a loop (for tests).  plant: a
    nearest-point TPWLATV (its handle_for(dt_sim)); C (n_o, n_plant), y_ref (n_o,): its measurement; observer_model: the SSMDynamics
    whose V and z_ref form x_hat; j, theta (n_keep): the schedule; uopt (B, N, n_u), x (B, n_plant), W (n_keep, B, n_plant), V (n_keep, B,
    n_o) -> dict X (B, n_keep, n_plant), Z, Y (B, n_keep, n_o), U (B, n_keep, n_u), Xhat (B, n_keep, n_x), idx (B, n_keep) int32: the
    plant's point of every sub-step.  With Y (a Polyhedron(with_reproject=True)): also Y_used (B, n_keep, n_o), proj (B, n_keep) int32."""
    admissible = Y                                                 # (Y names the measurement record below)
    uopt = _lib.f64(np.asarray(uopt))
    C = _lib.f64(np.asarray(C))
    B, n_p, m, n, nk = uopt.shape[0], int(plant.get_state_dim()), int(plant.get_input_dim()), observer_model.state_dim, len(j)
    no = C.shape[0]
    if C.shape != (no, n_p) or np.shape(y_ref) != (no,):
        raise RuntimeError('advance_tpwl: C must have shape (n_o, n_plant) = (n_o, %d) and y_ref (n_o,), got %s and %s' % (n_p, C.shape, np.shape(y_ref)))
    y_ref = _lib.f64(np.asarray(y_ref))
    uopt = _lib.f64(uopt.reshape(B, N, m)); x = _lib.f64(np.asarray(x).reshape(B, n_p))
    W = None if W is None else _lib.f64(np.asarray(W).reshape(nk, B, n_p))
    V = None if V is None else _lib.f64(np.asarray(V).reshape(nk, B, no))
    j = np.ascontiguousarray(j, dtype=np.int32); theta = _lib.f64(np.asarray(theta).reshape(nk))
    X, Xh, Z, Y, U = np.empty((B, nk, n_p)), np.empty((B, nk, n)), np.empty((B, nk, no)), np.empty((B, nk, no)), np.empty((B, nk, m))
    idx = np.empty((B, nk), dtype=np.int32)
    if admissible is not None:
        YA, Yb, yrows = _Y_arrays('advance_tpwl', admissible, no)
        Ym, Yu, pj = np.empty((B, nk, no)), np.empty((B, nk, no)), np.empty((B, nk), dtype=np.int32)
        _lib.check(_lib.lib().sgusto_ssm_loop_advance_tpwl_reprojected(
            plant.handle_for(float(dt_sim)), _lib.dptr(C), _lib.dptr(y_ref), ctypes.c_int(no), observer_model.handle, ctypes.c_double(float(dt_sim)),
            ctypes.c_int(int(N)), ctypes.c_int(nk), ctypes.c_int64(B), _lib.iptr(j), _lib.dptr(theta), _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W),
            _lib.dptr(V), _lib.dptr(YA), _lib.dptr(Yb), ctypes.c_int(yrows), _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U), _lib.dptr(Ym), _lib.dptr(Xh),
            _lib.iptr(idx), _lib.dptr(Yu), _lib.iptr(pj)), 'sgusto_ssm_loop_advance_tpwl_reprojected')
        return dict(X=X, Z=Z, U=U, Y=Ym, Xhat=Xh, idx=idx, Y_used=Yu, proj=pj)
    _lib.check(_lib.lib().sgusto_ssm_loop_advance_tpwl(plant.handle_for(float(dt_sim)), _lib.dptr(C), _lib.dptr(y_ref), ctypes.c_int(no),
                                                       observer_model.handle, ctypes.c_double(float(dt_sim)), ctypes.c_int(int(N)), ctypes.c_int(nk), ctypes.c_int64(B),
                                                       _lib.iptr(j), _lib.dptr(theta), _lib.dptr(uopt), _lib.dptr(x), _lib.dptr(W), _lib.dptr(V),
                                                       _lib.dptr(X), _lib.dptr(Z), _lib.dptr(U), _lib.dptr(Y), _lib.dptr(Xh), _lib.iptr(idx)),
               'sgusto_ssm_loop_advance_tpwl')
    return dict(X=X, Z=Z, U=U, Y=Y, Xhat=Xh, idx=idx)
