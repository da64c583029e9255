"""Infinite-horizon discrete and continuous LQR gains on the device (sofacontrol/lqr/lqr.py:6-64)."""
import ctypes as C

import numpy as np

from .. import _lib


def _dare_call(entry, A, B, Q, R, tol, max_iter):
    """One of the Riccati entry points (`sric_dare_fixed_point`, `sric_dare`, `sric_dare_wide`, `sric_care`: one argument list)
    on a single (A, B) pair or a stack of them: stacked (L, P, iterations)."""
    A, B = np.asarray(A), np.asarray(B)
    A = _lib.f64(A.reshape(-1, A.shape[-2], A.shape[-1]))
    B = _lib.f64(B.reshape(-1, B.shape[-2], B.shape[-1]))
    batch, n, m = B.shape
    L = np.empty((batch, m, n)); P = np.empty((batch, n, n)); it = np.empty(batch, dtype=np.int32)
    _lib.check(getattr(_lib.lib(), entry)(_lib.dptr(A), _lib.dptr(B), C.c_int64(batch), C.c_int(n), C.c_int(m),
                                          _lib.dptr(_lib.f64(Q)), _lib.dptr(_lib.f64(R)), C.c_double(tol), C.c_int(max_iter),
                                          _lib.dptr(L), _lib.dptr(P), _lib.iptr(it)), entry)
    return L, P, it


def _fixed_point(A, B, Q, R, tol, max_iter):
    return _dare_call('sric_dare_fixed_point', A, B, Q, R, tol, max_iter)


def solve_riccati(A, B, Q, R):
    """lqr.py:6-21: fixed-point DARE until ||L - L_old||_F <= 1e-4; returns (L, P), u = +L x."""
    L, P, _ = _fixed_point(A, B, Q, R, 1e-4, 1000000)
    return L[0], P[0]


def tvlqr(A, B, Q, R):
    """Finite-horizon TV-LQR for explicit per-step (A_i, B_i), i = 0..n-1 in forward time order, terminal P = Q
    (traj_tracking_lqr.py:18-48 without the TPWL lookup, `sric_tvlqr`): K (n, n_u, n_x), P (n + 1, n_x, n_x), u = +K x."""
    A, B = _lib.f64(A), _lib.f64(B)
    steps, n, m = B.shape
    if A.shape != (steps, n, n):
        raise RuntimeError('tvlqr: A %s does not match B %s' % (A.shape, B.shape))
    K = np.empty((steps, m, n)); P = np.empty((steps + 1, n, n))
    _lib.check(_lib.lib().sric_tvlqr(_lib.dptr(A), _lib.dptr(B), C.c_int(steps), C.c_int(n), C.c_int(m),
                                     _lib.dptr(_lib.f64(Q)), _lib.dptr(_lib.f64(R)), _lib.dptr(K), _lib.dptr(P)), 'sric_tvlqr')
    return K, P


def dare(Ad, Bd, Q, R):
    """lqr.py:24-31 (scipy.linalg.solve_discrete_are in the reference): the stabilising DARE solution and its gain
    K = -(R + B'PB)^-1 B'PA, by the structure-preserving doubling algorithm on the device (`sric_dare`)."""
    L, P, _ = _dare_call('sric_dare', Ad, Bd, Q, R, 1e-14, 100)
    return L[0], P[0]


def dare_wide(Ad, Bd, Q, R):
    """`dare` for an input block of up to 64 columns (`sric_dare_wide`, csrc/dare_wide.hip): what the ROMPC observer asks
    for, dare(A_d.T, C.T, Q, R) with one "input" per measurement (baselines/rompc/observer.py:27).  Same doubling steps,
    tolerance and sign (u = +K x); a stack of (A_d, B_d) pairs returns stacked (K, P)."""
    K, P, _ = _dare_call('sric_dare_wide', Ad, Bd, Q, R, 1e-14, 100)
    return (K, P) if np.ndim(Bd) == 3 else (K[0], P[0])


def dare_batch(Ad, Bd, Q, R, tol=1e-14):
    """Gains for a stack of (A_d, B_d) pairs in one launch (the per-point gains of the scp controller,
    tpwl/controllers.py:238-246)."""
    L, P, _ = _dare_call('sric_dare', Ad, Bd, Q, R, tol, 100)
    return L, P


def care(A, B, Q, R):
    """lqr.py:63 (control.lqr, i.e. slycot's continuous Riccati solver, in the reference): the stabilising solution P of
    A'P + P A - P B R^-1 B'P + Q = 0 and its gain K = -R^-1 B'P on the continuous pair (A, B), by a Cayley transform and the
    doubling loop of `dare` on the device (`sric_care`).  u = +K x as everywhere in this package; control.lqr returns -K."""
    K, P, _ = _dare_call('sric_care', A, B, Q, R, 1e-14, 100)
    return K[0], P[0]


def care_batch(A, B, Q, R, tol=1e-14):
    """Continuous-time gains for a stack of (A, B) pairs in one launch: stacked (K, P)."""
    K, P, _ = _dare_call('sric_care', A, B, Q, R, tol, 100)
    return K, P


class DLQR:
    """lqr.py:34-54."""

    def __init__(self, dt, model, cost_params):
        self.dt = dt
        self.model = model
        self.cost_params = cost_params

    def compute_policy(self, target):
        u_nom = np.atleast_1d(target.u)
        x_nom = target.x
        K = self.compute_gain_matrix(target.A, target.B, self.cost_params.Q, self.cost_params.R)
        return x_nom, u_nom, K

    def compute_gain_matrix(self, A, B, Q, R):
        Ad, Bd, _ = self.model.discretize_dynamics(A_c=A, B_c=B, d_c=np.zeros(self.model.get_state_dim()), dt=self.dt)
        K, _ = solve_riccati(Ad, Bd, Q, R)
        return K


class CLQR(DLQR):
    """lqr.py:57-64: infinite-horizon continuous LQR about one operating point; no discretisation.  The gain is stated for
    u = u_bar + K (x - x_bar), the form StateCLQR applies (the reference hands control.lqr's gain, made for u = -K x, to that same
    form: INTEGRATION.md, "Behavioural notes")."""

    def compute_gain_matrix(self, A, B, Q, R):
        return care(A, B, Q, R)[0]
