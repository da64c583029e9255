"""Reference statement of the sub-step chain of the batched SSM closed loop (csrc/gusto_ssm_loop.hip: ssm_loop_advance_kernel), written
once and parameterised by dtype: in np.longdouble it is built on tests/ssm_reference.py (the reference), in np.float64 on oracle/ssm.py
(the oracle whose distance from the reference, e_oracle, sets the tolerance of every device comparison).  Shift and window of a period are
those of tests/cl_reference.py.  Nothing here imports the package under test.

Per sub-step s (SSM/controllers.py:204, 237; SSM/ssm.py:198-218, 279-301; SSMObserver.update):
    u      = [uopt ; uopt[-1]] interpolated at (j_s, theta_s)                 no feedback gain
    x     <- A_d x + B_d u + d_d (+ w_s)    (A_d, B_d, d_d) = the PLANT's Jacobians at (x, u), discretised at dt_sim
    zeta   = C_plant(x)                     without z_ref
    y      = (zeta + z_ref_plant) + v_s     in this order of additions
    x_hat  = V_planner phi_s(y - z_ref_planner)"""
import numpy as np

import ssm_reference as sr
from cl_reference import LD, err, shift, window      # noqa: F401  (shift / window: re-exported for the loop tests)
from oracle import ssm as ossm


def _lib_of(dtype):
    return sr if dtype is LD else ossm


def jacobians(model, x, u, dt_sim, method, dtype):
    """(A_d, B_d, d_d) of `model` at (x, u); method: 'fe' | 'be' | 'bil' | 'map' (the Jacobians of the discrete map)."""
    if dtype is LD:
        return sr.jacobians(model, x, u, dt_sim, method)
    return ossm.jacobians(model, x, u, dt_sim, 'fe' if method == 'map' else method, discrete=method == 'map')


def measure(plant, planner, x, v, dtype):
    """zeta, y, x_hat of the plant state x; v: measurement noise or None."""
    lib = _lib_of(dtype)
    zeta = lib.observe(plant, x)
    y = zeta + plant['z_ref']
    if v is not None:
        y = y + np.asarray(v, dtype=dtype)
    return zeta, y, lib.reduce(planner, y)


def advance(plant, planner, method, dt_sim, uopt, x, j, theta, W, V, dtype):
    """n_keep sub-steps of one loop.  plant / planner: model dicts of the dtype's library (ssm_reference.make_model in long double,
    oracle.ssm.make_model in float64); uopt (N, n_u); x (n_x); j, theta (n_keep); W (n_keep, n_x), V (n_keep, n_o) or None.
    Returns X, Z, U, Y, Xhat, each (n_keep, .)."""
    c = lambda a: np.asarray(a, dtype=dtype)
    uopt, x = c(uopt), c(x)
    uext = np.vstack((uopt, uopt[-1:]))
    X, Z, U, Y, Xh = [], [], [], [], []
    for s in range(len(j)):
        js, th = int(j[s]), dtype(theta[s])
        u = uext[js] + th * (uext[js + 1] - uext[js])
        A, B, d = jacobians(plant, x, u, dt_sim, method, dtype)
        x = A @ x + B @ u + d
        if W is not None:
            x = x + c(W[s])
        zeta, y, xh = measure(plant, planner, x, None if V is None else V[s], dtype)
        X.append(x); Z.append(zeta); U.append(u); Y.append(y); Xh.append(xh)
    return tuple(np.stack(a) for a in (X, Z, U, Y, Xh))
