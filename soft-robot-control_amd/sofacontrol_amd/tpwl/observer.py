"""Observers (sofacontrol/tpwl/observer.py).  FullStateObserver (lines 3-30) is pure bookkeeping; the
DiscreteEKFObserver (lines 33-126) keeps its estimate and covariance in HBM and runs one kernel per step
(`sekf_step`, csrc/observer.hip).  DiscreteEKFObserverBatch runs `batch` such filters over one model with one launch per
step (`sekf_batch_step`)."""
import ctypes as C

import numpy as np

from .. import _lib


class FullStateObserver:
    def __init__(self, n_x, H=None):
        self.x = None
        self.z = None
        self.meas_dim = n_x
        self.state_dim = n_x
        self.H = H

    def get_meas_dim(self):
        return self.meas_dim

    def get_observer_params(self):
        return {'meas_dim': self.meas_dim, 'state_dim': self.state_dim}

    def update(self, u, y, dt, x=None):
        self.x = x
        self.z = self.H @ x if self.H is not None else x


class DiscreteEKFObserver:
    """observer.py:33-126.  `Sigma` is read back from the device on access."""

    def __init__(self, dyn_sys, **kwargs):
        self.dyn_sys = dyn_sys
        if self.dyn_sys.C is None:
            raise RuntimeError('Need to set meas. model in dyn_sys')
        self.C = self.dyn_sys.C
        self.state_dim = self.dyn_sys.get_state_dim()
        self.meas_dim = self.C.shape[0]
        self._Sigma0 = np.array(kwargs.get('Sigma0', np.eye(self.state_dim)), dtype=np.float64)
        self.W = kwargs.get('W', 100 * np.eye(self.state_dim))
        self.V = kwargs.get('V', np.eye(self.meas_dim))
        self._h = C.c_void_p()
        self._filter_dt = None
        self.x = None
        self._z = None
        self._make_filter(None, self._Sigma0, None)
        self.initialize(self.dyn_sys.rom.x_ref)

    def _make_filter(self, dt, Sigma, x):
        """(Re)create the device filter on the model handle whose tables are discretised at `dt` (the planner and
        the simulation usually run different time steps: each keeps its own tables, tpwl.handle_for)."""
        if self._h:
            _lib.lib().sekf_destroy(self._h)
            self._h = C.c_void_p()
        nn = getattr(self.dyn_sys, 'tpwl_method', 'nn') == 'nn'
        mh = self.dyn_sys.handle_for(dt if nn else None)
        Cm, yr = _lib.f64(self.C), _lib.f64(self.dyn_sys.y_ref)
        S0, W, V = _lib.f64(Sigma), _lib.f64(self.W), _lib.f64(self.V)
        _lib.check(_lib.lib().sekf_create(C.byref(self._h), mh, _lib.dptr(Cm), _lib.dptr(yr),
                                          C.c_int(self.meas_dim), _lib.dptr(S0), _lib.dptr(W), _lib.dptr(V)),
                   'sekf_create')
        if x is not None:
            xx = _lib.f64(x)
            _lib.check(_lib.lib().sekf_set_state(self._h, _lib.dptr(xx), None), 'sekf_set_state')
        self._filter_dt = dt

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            try:
                _lib.lib().sekf_destroy(h)
            except Exception:
                pass
            self._h = None

    def get_meas_dim(self):
        return self.meas_dim

    def get_observer_params(self):
        return {'W': self.W, 'V': self.V, 'meas_dim': self.meas_dim, 'state_dim': self.state_dim,
                'C': self.C, 'H': self.dyn_sys.H}

    def kernel_plan(self):
        """Which filter kernel the live device handle runs (_lib.ekf_handle_plan)."""
        return _lib.ekf_handle_plan(self._h)

    @property
    def Sigma(self):
        S = np.empty((self.state_dim, self.state_dim))
        _lib.check(_lib.lib().sekf_get_state(self._h, None, _lib.dptr(S)), 'sekf_get_state')
        return S

    @Sigma.setter
    def Sigma(self, S):
        S = _lib.f64(S)
        _lib.check(_lib.lib().sekf_set_state(self._h, None, _lib.dptr(S)), 'sekf_set_state')

    # z follows x (observer.py:92-95, 123-126); it is evaluated when read, so a control loop that only uses the
    # estimate does not pay a sparse product per simulation step
    @property
    def z(self):
        if self._z is None and self.x is not None:
            if self.dyn_sys.H is not None:
                self._z = self.dyn_sys.x_to_zfyf(self.x, zf=True)
            else:
                self._z = self.dyn_sys.x_to_zfyf(self.x, yf=True)
        return self._z

    @z.setter
    def z(self, value):
        self._z = value

    def _set_z(self):
        self._z = None

    def initialize(self, xf):
        """observer.py:76-86."""
        self.x = self.dyn_sys.rom.compute_RO_state(xf=xf)
        x = _lib.f64(self.x)
        _lib.check(_lib.lib().sekf_set_state(self._h, _lib.dptr(x), None), 'sekf_set_state')
        self._set_z()

    def _step(self, u, y, dt):
        A = B = d = None
        if u is not None:
            if getattr(self.dyn_sys, 'tpwl_method', 'nn') == 'nn':
                if self._filter_dt != dt:                   # first predictor step, or a new time step
                    self._make_filter(dt, self.Sigma, self.x)
            else:
                A, B, d = [_lib.f64(a) for a in self.dyn_sys.get_jacobians(self.x, dt)]
            u = _lib.f64(u)
        if y is not None:
            y = _lib.f64(y)
        x = np.empty(self.state_dim)
        _lib.check(_lib.lib().sekf_step(self._h, _lib.dptr(u), _lib.dptr(y), _lib.dptr(A), _lib.dptr(B),
                                        _lib.dptr(d), _lib.dptr(x)), 'sekf_step')
        self.x = x

    def update_projected(self, rom, xf, u, y, dt):
        """The per-simulation-step pair rom.compute_RO_state(xf=xf); update(u, y, dt) in one library call
        (`sekf_step_projected`: the projection runs on a side stream beside the filter kernel).  Returns the projected
        state.  Models that hand the filter external Jacobians (weighting modes) take the two separate calls."""
        if u is None or getattr(self.dyn_sys, 'tpwl_method', 'nn') != 'nn' or getattr(rom, 'handle', None) is None:
            x_reduced = rom.compute_RO_state(xf=xf)
            self.update(u, y, dt)
            return x_reduced
        if self._filter_dt != dt:
            self._make_filter(dt, self.Sigma, self.x)
        xf, u, y = _lib.f64(xf), _lib.f64(u), _lib.f64(y)
        n_f, r = rom.U.shape
        if xf.shape != (2 * n_f,):
            raise RuntimeError('sekf_step_projected: expected a full-order state of %d entries, got %s'
                               % (2 * n_f, xf.shape))
        x_reduced, x = np.empty(2 * r), np.empty(self.state_dim)
        _lib.check(_lib.lib().sekf_step_projected(self._h, rom.handle, _lib.dptr(xf), _lib.dptr(u), _lib.dptr(y),
                                                  _lib.dptr(x_reduced), _lib.dptr(x)), 'sekf_step_projected')
        self.x = x
        self._set_z()
        return x_reduced

    def update(self, u, y, dt, **kwargs):
        """observer.py:88-95: predictor + filter update in one kernel."""
        self._step(u, y, dt)
        self._set_z()

    def predict_state(self, u, dt):
        """observer.py:97-106."""
        self._step(u, None, dt)

    def update_state(self, y):
        """observer.py:108-126."""
        self._step(None, y, None)
        self._set_z()
        return self.x


class DiscreteEKFObserverBatch:
    """`batch` DiscreteEKFObserver filters over one nearest-point model, stepped together: one kernel launch and one host wait per
    call (`sekf_batch_step`).  C, y_ref, W, V and the model's tables are shared; estimate, covariance and status are per filter,
    and each predictor takes the table point nearest to its own estimate.  Member b computes what a DiscreteEKFObserver fed
    member b's numbers computes, bit for bit.  Sigma0 (n_x x n_x) is installed in every filter.

    A filter whose innovation covariance is not positive definite keeps its x and Sigma and sets status[b] = 1; the call then
    raises (as the single observer does) after `x` has been refreshed, and the other filters have stepped."""

    def __init__(self, dyn_sys, batch, **kwargs):
        self.dyn_sys = dyn_sys
        if self.dyn_sys.C is None:
            raise RuntimeError('Need to set meas. model in dyn_sys')
        method = getattr(self.dyn_sys, 'tpwl_method', 'nn')
        if method != 'nn':
            raise RuntimeError('DiscreteEKFObserverBatch: weighting-mode models (tpwl_method = %r) are not batched: the batched '
                               'filter takes the nearest-point tables (tpwl_method = \'nn\') only' % (method,))
        if int(batch) != batch or int(batch) < 1:
            raise RuntimeError('DiscreteEKFObserverBatch: batch must be an integer >= 1, got %r' % (batch,))
        self.batch = int(batch)
        self.C = self.dyn_sys.C
        self.state_dim = self.dyn_sys.get_state_dim()
        self.input_dim = self.dyn_sys.get_input_dim()
        self.meas_dim = self.C.shape[0]
        n, ny = self.state_dim, self.meas_dim
        self._Sigma0 = self._shaped(kwargs.get('Sigma0', np.eye(n)), (n, n), 'Sigma0')
        self.W = self._shaped(kwargs.get('W', 100 * np.eye(n)), (n, n), 'W')
        self.V = self._shaped(kwargs.get('V', np.eye(ny)), (ny, ny), 'V')
        if np.shape(self.C) != (ny, n):
            raise RuntimeError('DiscreteEKFObserverBatch: C must be (n_y, n_x = %d), got %s' % (n, np.shape(self.C)))
        if _lib.ekf_plan(n, ny)['path'] == 0:
            raise RuntimeError('DiscreteEKFObserverBatch: no filter kernel takes n_x = %d, n_y = %d (need 0 < n_y <= n_x and a step '
                               'that fits the 160 KB LDS)' % (n, ny))
        self._h = C.c_void_p()
        self._filter_dt = None
        self._bound = False
        self._x = None
        self._make_filter(None, None, None)

    def bind(self, dt):
        """Put the filters on the model handle discretised at `dt` and keep them there: a ClosedLoopBatch that steps these filters on
        the device holds on to the handle, so a later step at another dt is refused instead of re-creating it."""
        if self._filter_dt != dt:
            if self._bound:
                raise RuntimeError('DiscreteEKFObserverBatch: the filters are bound to dt = %g by a closed loop; dt = %g would re-create '
                                   'them' % (self._filter_dt, dt))
            self._make_filter(dt, self.Sigma, self._x)
        self._bound = True

    @staticmethod
    def _shaped(a, shape, name):
        a = _lib.f64(a)
        if a.shape != shape:
            raise RuntimeError('DiscreteEKFObserverBatch: %s must have shape %s, got %s' % (name, shape, a.shape))
        return a

    def _make_filter(self, dt, Sigma, x):
        """(Re)create the device filters on the model handle whose tables are discretised at `dt` (DiscreteEKFObserver._make_filter)."""
        self._destroy()
        mh = self.dyn_sys.handle_for(dt)
        Cm, yr = _lib.f64(self.C), _lib.f64(self.dyn_sys.y_ref)
        _lib.check(_lib.lib().sekf_batch_create(C.byref(self._h), mh, _lib.dptr(Cm), _lib.dptr(yr), C.c_int(self.meas_dim),
                                                _lib.dptr(self._Sigma0), _lib.dptr(self.W), _lib.dptr(self.V), C.c_int64(self.batch)),
                   'sekf_batch_create')
        if x is not None or Sigma is not None:
            _lib.check(_lib.lib().sekf_batch_set_state(self._h, _lib.dptr(_lib.f64(x)), _lib.dptr(_lib.f64(Sigma))), 'sekf_batch_set_state')
        self._filter_dt = dt

    def _destroy(self):
        if self._h:
            _lib.lib().sekf_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._destroy()
        except Exception:
            pass

    def get_meas_dim(self):
        return self.meas_dim

    def kernel_plan(self):
        """Which filter kernel the live device handle runs, as DiscreteEKFObserver.kernel_plan, plus 'batch'."""
        path, lds, gain, batch = C.c_int(0), C.c_size_t(0), C.c_int(0), C.c_int64(0)
        _lib.check(_lib.lib().sekf_batch_plan(self._h, C.byref(path), C.byref(lds), C.byref(gain), C.byref(batch)), 'sekf_batch_plan')
        return dict(_lib._ekf_plan_dict(path, lds, gain), batch=int(batch.value))

    @property
    def x(self):
        """(batch, n_x): the estimates as the last call left them."""
        return self._x

    @property
    def Sigma(self):
        S = np.empty((self.batch, self.state_dim, self.state_dim))
        _lib.check(_lib.lib().sekf_batch_get_state(self._h, None, _lib.dptr(S), None), 'sekf_batch_get_state')
        return S

    @Sigma.setter
    def Sigma(self, S):
        S = self._shaped(S, (self.batch, self.state_dim, self.state_dim), 'Sigma')
        _lib.check(_lib.lib().sekf_batch_set_state(self._h, None, _lib.dptr(S)), 'sekf_batch_set_state')

    @property
    def status(self):
        """(batch,) int32: 1 where the filter's last step found its innovation covariance not positive definite."""
        st = np.empty(self.batch, dtype=np.int32)
        _lib.check(_lib.lib().sekf_batch_get_state(self._h, None, None, _lib.iptr(st)), 'sekf_batch_get_state')
        return st

    @property
    def points(self):
        """(batch,) int32: the table point each filter's last predictor took (-1 before the first)."""
        idx = np.empty(self.batch, dtype=np.int32)
        _lib.check(_lib.lib().sekf_batch_last_points(self._h, _lib.iptr(idx)), 'sekf_batch_last_points')
        return idx

    def initialize(self, x):
        """Install the reduced-order estimates x (batch, n_x); the covariances stay."""
        x = self._shaped(x, (self.batch, self.state_dim), 'x')
        _lib.check(_lib.lib().sekf_batch_set_state(self._h, _lib.dptr(x), None), 'sekf_batch_set_state')
        self._x = x.copy()

    def _step(self, u, y, dt):
        if u is not None:
            u = self._shaped(u, (self.batch, self.input_dim), 'u')
        if y is not None:
            y = self._shaped(y, (self.batch, self.meas_dim), 'y')
        if u is not None and self._filter_dt != dt:            # first predictor step, or a new time step
            if self._bound:
                raise RuntimeError('DiscreteEKFObserverBatch: the filters are bound to dt = %g by a closed loop; dt = %g would re-create '
                                   'them' % (self._filter_dt, dt))
            self._make_filter(dt, self.Sigma, self._x)
        x = np.empty((self.batch, self.state_dim))
        rc = _lib.lib().sekf_batch_step(self._h, _lib.dptr(u), _lib.dptr(y), _lib.dptr(x))
        if rc in (0, -4):                                      # SRH_ENUMERIC: the failed filters kept their state, x is valid
            self._x = x
        _lib.check(rc, 'sekf_batch_step')

    def update(self, u, y, dt):
        """Predictor + filter update of every member in one kernel: u (batch, n_u), y (batch, n_y)."""
        self._step(u, y, dt)

    def predict_state(self, u, dt):
        self._step(u, None, dt)

    def update_state(self, y):
        self._step(None, y, None)
        return self._x
