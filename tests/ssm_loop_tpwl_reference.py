"""Reference statement of the sub-step chain of the SSM closed loop on a TPWL plant (csrc/gusto_ssm_loop.hip:
ssm_loop_advance_tpwl_kernel), written once and parameterised by dtype: np.longdouble is the reference, np.float64 the oracle whose
distance from the reference, e_oracle, sets the tolerance of every device comparison.  The plant chain is cl_reference.advance without
gains (it records the nearest-point margin), the measurement and the estimate are those of ssm_loop_reference.measure with zeta = C x.
Nothing here imports the package under test.

Per sub-step s (SSM/controllers.py:204, 237; tpwl/tpwl.py:160-168, 336-339; SSMObserver.update):
    u      = [uopt ; uopt[-1]] interpolated at (j_s, theta_s)                 no feedback gain
    i      = argmin_i w_q |q_i - q| + w_v |v_i - v| of x = [v; q]             first minimum
    x     <- A_d[i] x + B_d[i] u + d_d[i] (+ w_s)
    zeta   = C x                            without y_ref
    y      = (zeta + y_ref) + v_s           in this order of additions
    x_hat  = V_observer phi_s(y - z_ref_observer)"""
import numpy as np

import cl_reference as cr
import ssm_loop_reference as slr
from cl_reference import LD, err, tolerance, E_ORACLE_MAX, MARGIN      # noqa: F401  (the project's rule, under this name too)

FIELDS = ('X', 'Z', 'U', 'Y', 'Xhat')


def measure(C, y_ref, observer, x, v, dtype):
    """zeta, y, x_hat of the plant state x; v: measurement noise or None (ssm_loop_reference.measure with zeta = C x)."""
    lib = slr._lib_of(dtype)
    zeta = np.asarray(C, dtype=dtype) @ np.asarray(x, dtype=dtype)
    y = zeta + np.asarray(y_ref, dtype=dtype)
    if v is not None:
        y = y + np.asarray(v, dtype=dtype)
    return zeta, y, lib.reduce(observer, y)


def advance(plant, C, y_ref, observer, uopt, x, j, theta, W, V, dtype):
    """n_keep sub-steps of one loop.  plant: dict q, v, w_q, w_v, A_d, B_d, d_d; C (n_o, n_p), y_ref (n_o); observer: the model dict of the
    dtype's library (ssm_reference.make_model in long double, oracle.ssm.make_model in float64); uopt (N, n_u); x (n_p); j, theta
    (n_keep); W (n_keep, n_p), V (n_keep, n_o) or None.  Returns X, Z, U, Y, Xhat (n_keep, .), the plant's picks (n_keep) and the least
    nearest-point margin."""
    N, n_p = np.shape(uopt)[0], np.shape(x)[0]
    X, U, _, picks, _, margin = cr.advance(None, plant, C, None, np.zeros((N + 1, n_p)), uopt, x, j, theta, W, dtype)
    Z, Y, Xh = [], [], []
    for s in range(len(j)):
        zeta, y, xh = measure(C, y_ref, observer, X[s], None if V is None else V[s], dtype)
        Z.append(zeta); Y.append(y); Xh.append(xh)
    return X, np.stack(Z), U, np.stack(Y), np.stack(Xh), picks, margin
