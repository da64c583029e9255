"""Reference statement of the batched closed-loop iLQR (csrc/ilqr_loop.hip): the row table of the controller's clock, the per-step law
u = u_bar[row] + K[row] (xl - x_bar[row]) (tpwl/controllers.py:199-215), the TPWL plant step at the simulation step (tpwl/tpwl.py:160-168,
336-339) and, with an observer, the measurement and one predict + update of the filter (tests/clobs_reference.py: filter_step).  The same
code runs in np.longdouble (the reference) and in np.float64 (the oracle whose distance from the reference, e_oracle, sets the tolerance
of every device comparison); it imports neither the package nor oracle/ directly.  Every nearest-point lookup records the relative gap
between the two smallest distances.

Simulation step s of one member (step = step0 + s since the reset, dt = r dt_sim):
    if step % r == 0:  j = step / r, row = rows[j] (idle beyond the table or outside 0 .. N-1)
                       u = u_bar[row] + K[row] (xl - x_bar[row]), or u0 when idle;   xl = x_hat with an observer, else x
    x = A_d[p] x + B_d[p] u + d_d[p] (+ w_s),  p = plant's point nearest to x;  z = H x
    observer:  y = C x + y_ref (+ v_s);  x_hat, Sigma = predict with u on the filter model's point nearest to x_hat, then update with y"""
import numpy as np

import cl_reference as cr
import clobs_reference as cor

from cl_reference import LD, err, tolerance, E_ORACLE_MAX, MARGIN          # noqa: F401


def rows_table(N, dt, count, final_time=None):
    """row_j = int(round(j dt, 4) / dt) for j = 0 .. count-1 in Python floats (IEEE doubles): the expression of _tracking_input at the
    clock's t_step = round(j dt, 4); -1 where row_j >= N (the reference raises IndexError at row_j == N) or t_step > final_time."""
    rows = []
    for j in range(count):
        t_step = round(j * dt, 4)
        row = int(t_step / dt)
        rows.append(-1 if row >= N or (final_time is not None and t_step > final_time) else row)
    return np.array(rows, dtype=np.int32)


def tracking_rows(dt, count):
    """The raw rows int(t_step / dt) of tpwl.controllers._tracking_input over the clock's first `count` steps (no horizon)."""
    return np.array([int(round(j * dt, 4) / dt) for j in range(count)])


def law(xbar, ubar, K, rows, N, r, u0, step, xl, u_held):
    """The input of simulation step `step`: the held one between controller steps."""
    if step % r != 0:
        return u_held
    j = step // r
    row = int(rows[j]) if j < len(rows) else -1
    if not 0 <= row < N:
        return u0
    return ubar[row] + K[row] @ (xl - xbar[row])


def advance(plant, H, xbar, ubar, K, rows, r, u0, x, u_held, steps, step0, W, dtype):
    """`steps` simulation steps of one member without an observer.  plant: dict q, v, w_q, w_v, A_d, B_d, d_d; H (n_z, n_x); xbar (N+1,
    n_x), ubar (N, n_u), K (N, n_u, n_x); u0, u_held (n_u); x (n_x); W (steps, n_x) or None.
    Returns X (steps, n_x), U, Z, plant picks, the least margin."""
    c = lambda a: np.asarray(a, dtype=dtype)
    xbar, ubar, K, u0, x, u, H = c(xbar), c(ubar), c(K), c(u0), c(x), c(u_held), c(H)
    Ad, Bd, dd = c(plant['A_d']), c(plant['B_d']), c(plant['d_d'])
    N = ubar.shape[0]
    X, U, Z, ip, margin = [], [], [], [], float('inf')
    for s in range(steps):
        u = law(xbar, ubar, K, rows, N, r, u0, step0 + s, x, u)
        p, mp = cr.nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
        margin = min(margin, mp)
        x = Ad[p] @ x + Bd[p] @ u + dd[p]
        if W is not None:
            x = x + c(W[s])
        X.append(x); U.append(u); Z.append(H @ x); ip.append(p)
    return np.stack(X), np.stack(U), np.stack(Z), np.array(ip), margin


def observed(plant, filt, H, C, y_ref, Wf, Vf, xbar, ubar, K, rows, r, u0, x, x_hat, Sigma, steps, Wn, Vn, dtype):
    """`steps` simulation steps from a reset of one member with an observer (the law reads x_hat).  filt: the filter model's tables;
    C (n_y, n_x), y_ref; Wf, Vf the filter's covariances; Wn (steps, n_x) / Vn (steps, n_y) or None.
    Returns dict X, U, Z, Xhat, Y (steps rows each), idx_plant, idx_filter, margin."""
    c = lambda a: np.asarray(a, dtype=dtype)
    xbar, ubar, K, u0, x, x_hat, Sigma, H, C, y_ref = c(xbar), c(ubar), c(K), c(u0), c(x), c(x_hat), c(Sigma), c(H), c(C), c(y_ref)
    Ad, Bd, dd = c(plant['A_d']), c(plant['B_d']), c(plant['d_d'])
    filt = dict(filt, A_d=c(filt['A_d']), B_d=c(filt['B_d']), d_d=c(filt['d_d']))
    Wf, Vf = c(Wf), c(Vf)
    N = ubar.shape[0]
    u = u0
    out = dict(X=[], U=[], Z=[], Xhat=[], Y=[], idx_plant=[], idx_filter=[])
    margin = float('inf')
    for s in range(steps):
        u = law(xbar, ubar, K, rows, N, r, u0, s, x_hat, u)
        p, mp = cr.nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
        x = Ad[p] @ x + Bd[p] @ u + dd[p]
        if Wn is not None:
            x = x + c(Wn[s])
        y = C @ x + y_ref
        if Vn is not None:
            y = y + c(Vn[s])
        x_hat, Sigma, f, mf = cor.filter_step(filt, C, y_ref, Wf, Vf, x_hat, Sigma, u, y, dtype)
        margin = min(margin, mp, mf)
        for k, v in (('X', x), ('U', u), ('Z', H @ x), ('Xhat', x_hat), ('Y', y), ('idx_plant', p), ('idx_filter', f)):
            out[k].append(v)
    out = {k: np.stack(v) if k[0] != 'i' else np.array(v) for k, v in out.items()}
    out['margin'] = margin
    return out
