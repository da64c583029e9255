"""Luenberger observer of the ROMPC baseline -- surface of sofacontrol/baselines/rompc/observer.py:3-46.

The estimate lives on the device in an `srompc_t` handle (csrc/rompc.hip); `update` is one `srompc_step` with the input
given, `initialize` one `srompc_initialize` (POD projection straight into the estimate).  `batch` > 1 runs that many
independent loops on the same model; with batch == 1 every array has the reference's 1-D shape."""
import ctypes as C

import numpy as np

from ... import _lib
from ...lqr.lqr import dare, dare_wide

_BOUND = False


def _bind():
    global _BOUND
    L = _lib.lib()
    if _BOUND:
        return L
    vp, dp, i64 = C.c_void_p, _lib.c_double_p, C.c_int64
    L.srompc_create.argtypes = [C.POINTER(vp), i64, C.c_int, C.c_int, C.c_int, C.c_int] + [dp] * 9
    L.srompc_destroy.argtypes = [vp]
    L.srompc_set_gains.argtypes = [vp, dp, dp]
    L.srompc_set_state.argtypes = [vp, dp]
    L.srompc_get_state.argtypes = [vp, dp, dp]
    L.srompc_initialize.argtypes = [vp, vp, dp, dp, dp]
    L.srompc_step.argtypes = [vp, vp] + [dp] * 8
    L.srompc_replay.argtypes = [vp, C.c_int] + [dp] * 7
    L.srompc_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.srompc_set_timing.argtypes = [vp, C.c_int]
    L.srompc_last_device_ms.argtypes = [vp, C.POINTER(C.c_double)]
    _BOUND = True
    return L


class DiscreteLuenbergerObserver:
    """x_hat <- A_d x_hat + B_d u + d_d + L ((yf - y_ref) - C x_hat), constant gain L from the dual DARE."""

    def __init__(self, dyn_sys, Q, R, batch=1, L=None):
        self.dyn_sys = dyn_sys
        if self.dyn_sys.C is None:
            raise RuntimeError('Need to set meas. model in dyn_sys')
        self.C = self.dyn_sys.C
        self.batch = int(batch)
        n_y = self.C.shape[0]
        if L is None:
            solve = dare if n_y <= 16 else dare_wide      # sric_dare takes at most 16 "inputs"
            gain, _ = solve(np.ascontiguousarray(self.dyn_sys.A_d.T), np.ascontiguousarray(self.C.T), Q, R)
            L = -gain.T
        self._L = _lib.f64(np.reshape(L, (self.dyn_sys.A_d.shape[0], n_y)))      # L given: no DARE is solved
        d = self.dyn_sys
        self.n_x, self.n_u, self.n_y = d.A_d.shape[0], d.B_d.shape[1], n_y
        self.n_z = d.H.shape[0] if d.H is not None else n_y
        self._K = np.zeros((self.n_u, self.n_x))
        self._h = C.c_void_p()
        f = _lib.f64
        keep = [f(d.A_d), f(d.B_d), f(np.ravel(d.d_d)), f(self.C), f(np.ravel(d.y_ref)), f(d.H),
                None if d.H is None else f(np.ravel(d.z_ref)), self._K, self._L]
        _lib.check(_bind().srompc_create(C.byref(self._h), C.c_int64(self.batch), self.n_x, self.n_u, self.n_y, self.n_z,
                                         *[_lib.dptr(a) for a in keep]), 'srompc_create')
        self.x = None
        self.z = None

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            try:
                _lib.lib().srompc_destroy(h)
            except Exception:
                pass
            self._h = None

    # gains: setting either one sends both to the device, where A_d - L C is folded again
    @property
    def L(self):
        return self._L

    @L.setter
    def L(self, value):
        self._L = _lib.f64(np.reshape(value, (self.n_x, self.n_y)))
        _lib.check(_bind().srompc_set_gains(self._h, None, _lib.dptr(self._L)), 'srompc_set_gains')

    @property
    def K(self):
        return self._K

    @K.setter
    def K(self, value):
        self._K = _lib.f64(np.reshape(value, (self.n_u, self.n_x)))
        _lib.check(_bind().srompc_set_gains(self._h, _lib.dptr(self._K), None), 'srompc_set_gains')

    def _shape(self, a, width):
        """(batch x width) contiguous view of a caller's array, None passing through."""
        return None if a is None else _lib.f64(np.reshape(a, (self.batch, width)))

    def _out(self, a):
        return a[0] if self.batch == 1 else a

    def _full_width(self):
        return 2 * self.dyn_sys.rom.U.shape[0]

    def initialize(self, xf):
        xf = self._shape(xf, self._full_width())
        x, z = np.empty((self.batch, self.n_x)), np.empty((self.batch, self.n_z))
        _lib.check(_bind().srompc_initialize(self._h, self.dyn_sys.rom.handle, _lib.dptr(xf), _lib.dptr(x), _lib.dptr(z)),
                   'srompc_initialize')
        self.x, self.z = self._out(x), self._out(z)

    def step(self, y, u=None, ubar=None, xbar=None, xf=None):
        """One `srompc_step`: optional re-initialisation from the full state xf, then u (given, or ubar + K (x - xbar)),
        then the observer update with the full-order measurement y.  Returns u."""
        B = self.batch
        xf = self._shape(xf, self._full_width()) if xf is not None else None
        u, ubar = self._shape(u, self.n_u), self._shape(ubar, self.n_u)
        xbar, y = self._shape(xbar, self.n_x), self._shape(y, self.n_y)
        uo, x, z = np.empty((B, self.n_u)), np.empty((B, self.n_x)), np.empty((B, self.n_z))
        _lib.check(_bind().srompc_step(self._h, self.dyn_sys.rom.handle if xf is not None else None, _lib.dptr(xf), _lib.dptr(u),
                                       _lib.dptr(ubar), _lib.dptr(xbar), _lib.dptr(y), _lib.dptr(uo), _lib.dptr(x), _lib.dptr(z)),
                   'srompc_step')
        self.x, self.z = self._out(x), self._out(z)
        return self._out(uo)

    def update(self, u, y):
        self.step(y, u=u)

    def update_z(self):
        z = np.empty((self.batch, self.n_z))
        _lib.check(_bind().srompc_get_state(self._h, None, _lib.dptr(z)), 'srompc_get_state')
        self.z = self._out(z)

    def set_state(self, x):
        x = self._shape(x, self.n_x)
        _lib.check(_bind().srompc_set_state(self._h, _lib.dptr(x)), 'srompc_set_state')
        self.x = self._out(x.copy())
        self.update_z()

    def replay(self, Y, U=None, ubar=None, xbar=None):
        """T steps over a record in one launch (`srompc_replay`): Y (T x [batch x] n_y) and the inputs U, or the nominal
        ubar / xbar for the feedback.  Returns (U, X, Z) of every step; the estimate ends at X[-1]."""
        B = self.batch
        T = np.shape(Y)[0]
        r3 = lambda a, w: None if a is None else _lib.f64(np.reshape(a, (T, B, w)))
        Y, U, ubar, xbar = r3(Y, self.n_y), r3(U, self.n_u), r3(ubar, self.n_u), r3(xbar, self.n_x)
        Uo, X, Z = np.empty((T, B, self.n_u)), np.empty((T, B, self.n_x)), np.empty((T, B, self.n_z))
        _lib.check(_bind().srompc_replay(self._h, T, _lib.dptr(Y), _lib.dptr(U), _lib.dptr(ubar), _lib.dptr(xbar), _lib.dptr(Uo),
                                         _lib.dptr(X), _lib.dptr(Z)), 'srompc_replay')
        self.x, self.z = self._out(X[-1].copy()), self._out(Z[-1].copy())
        if B == 1:
            return Uo[:, 0], X[:, 0], Z[:, 0]
        return Uo, X, Z

    def set_timing(self, on=True):
        """Bracket every following call with device events (`srompc_set_timing`); `stats()['device_ms']` reads the last one."""
        _lib.check(_bind().srompc_set_timing(self._h, 1 if on else 0), 'srompc_set_timing')

    def stats(self):
        """{'steps', 'waits_last_step', 'device_ms'}: steps taken, the blocking host waits of the last call and, with timing
        on, its device-side duration (`srompc_stats`, `srompc_last_device_ms`)."""
        n, w, ms = C.c_int64(), C.c_int64(), C.c_double()
        _lib.check(_bind().srompc_stats(self._h, C.byref(n), C.byref(w)), 'srompc_stats')
        _lib.check(_bind().srompc_last_device_ms(self._h, C.byref(ms)), 'srompc_last_device_ms')
        return dict(steps=n.value, waits_last_step=w.value, device_ms=ms.value)
