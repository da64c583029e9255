"""Reference statement of the observed sub-step of the batched closed loop (csrc/gusto_loop.hip with an observer): the scp controller's
law at the filter's estimate, the plant step, the measurement, and one predict + update of the filter (tpwl/controllers.py:85-117,
298-333; tpwl/observer.py:97-126).  It composes tests/cl_reference.py (the nearest-point rule with its margin, the plan interpolation as
cl_reference.advance states it; shift and window are used unchanged around it) and tests/ekf_reference.py (predict, update).  Like
cl_reference the same code runs in np.longdouble (the reference) and in np.float64 (the oracle whose distance from the reference,
e_oracle, sets the tolerance of every device comparison); the float64 filter step is oracle/observer.py's.

Sub-step s of one loop (j, theta from the schedule):
    x_bar = xopt[j] + theta (xopt[j+1] - xopt[j]);  u_bar alike on [uopt; uopt[-1]]
    u     = u_bar + K[g] (x_hat - x_bar),  g = planner's point nearest to x_bar          (u = u_bar without gains)
    x     = A_d[p] x + B_d[p] u + d_d[p] (+ w),  p = plant's point nearest to x
    y     = C x + y_ref (+ v)
    x_hat, Sigma = predict with u on the FILTER model's point f nearest to x_hat, then update with y"""
import numpy as np

import cl_reference as cr
import ekf_reference as er
from oracle import observer as oobs

from cl_reference import LD, err, shift, window          # noqa: F401  (used unchanged around the sub-step)


def filter_step(filt, C, y_ref, Wf, Vf, x_hat, Sigma, u, y, dtype):
    """One predict + update on the filter model's region nearest to x_hat -> x_hat, Sigma, the point, its margin."""
    f, mf = cr.nearest_with_margin(filt['q'], filt['v'], filt['w_q'], filt['w_v'], x_hat, dtype)
    A, B, d = filt['A_d'][f], filt['B_d'][f], filt['d_d'][f]
    if dtype is LD:
        xp, Sp = er.predict(A, B, d, x_hat, Sigma, u, Wf)
        xn, Sn = er.update(C, y_ref, xp, Sp, y, Vf)
    else:
        xp, Sp = A @ x_hat + B @ u + d, A @ Sigma @ A.T + Wf
        xn, Sn = oobs.update(C, y_ref, xp, Sp, y, Vf)
    return xn, Sn, f, mf


def observed_advance(planner, plant, filt, H, C, y_ref, Wf, Vf, K, xopt, uopt, x, x_hat, Sigma, j, theta, Wn, Vn, dtype):
    """n_keep observed sub-steps of one loop.  planner: dict q, v, w_q, w_v; plant / filt: the same plus A_d, B_d, d_d; H (n_z, n_x);
    C (n_y, n_x), y_ref (n_y); Wf, Vf the filter's noise covariances; K (P, n_u, n_x) or None; xopt (N+1, n_x), uopt (N, n_u); x, x_hat
    (n_x), Sigma (n_x, n_x); Wn (n_keep, n_x) / Vn (n_keep, n_y) disturbance / measurement noise or None.
    Returns dict X, U, Z, Xhat, Y (n_keep rows each), Sigma (the last), idx_plant, idx_gain (-1 without gains), idx_filter, margin (the
    least over all three lookups)."""
    c = lambda a: np.asarray(a, dtype=dtype)
    xopt, uopt, x, x_hat, Sigma, H, C, y_ref = c(xopt), c(uopt), c(x), c(x_hat), c(Sigma), c(H), c(C), c(y_ref)
    Ad, Bd, dd = c(plant['A_d']), c(plant['B_d']), c(plant['d_d'])
    filt = dict(filt, A_d=c(filt['A_d']), B_d=c(filt['B_d']), d_d=c(filt['d_d']))
    Wf, Vf = c(Wf), c(Vf)
    K = None if K is None else c(K)
    uext = np.vstack((uopt, uopt[-1:]))
    out = dict(X=[], U=[], Z=[], Xhat=[], Y=[], idx_plant=[], idx_gain=[], idx_filter=[])
    margin = float('inf')
    for s in range(len(j)):
        js, th = int(j[s]), dtype(theta[s])
        x_bar = xopt[js] + th * (xopt[js + 1] - xopt[js])
        u = uext[js] + th * (uext[js + 1] - uext[js])
        g = -1
        if K is not None:
            g, mg = cr.nearest_with_margin(planner['q'], planner['v'], planner['w_q'], planner['w_v'], x_bar, dtype)
            margin = min(margin, mg)
            u = u + K[g] @ (x_hat - x_bar)
        p, mp = cr.nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
        margin = min(margin, mp)
        x = Ad[p] @ x + Bd[p] @ u + dd[p]
        if Wn is not None:
            x = x + c(Wn[s])
        y = C @ x + y_ref
        if Vn is not None:
            y = y + c(Vn[s])
        x_hat, Sigma, f, mf = filter_step(filt, C, y_ref, Wf, Vf, x_hat, Sigma, u, y, dtype)
        margin = min(margin, mf)
        for k, v in (('X', x), ('U', u), ('Z', H @ x), ('Xhat', x_hat), ('Y', y), ('idx_plant', p), ('idx_gain', g), ('idx_filter', f)):
            out[k].append(v)
    out = {k: np.stack(v) if k[0] != 'i' else np.array(v) for k, v in out.items()}
    out['Sigma'], out['margin'] = Sigma, margin
    return out
