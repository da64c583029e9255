"""Reference statement of the batched closed-loop ROMPC (csrc/rompc_loop.hip), one member at a time: the policy of
sofacontrol/baselines/rompc/rompc.py:57-141 (evaluate, solve_OCP, get_OCP_solution), rompc/observer.py:37-40 (update), baselines/ros.py:
223-227 (failure shift) and baselines/mpc.py get_target, around the solve.  The same code runs in np.longdouble (the reference) and in
np.float64 (the oracle whose distance from the reference, e_oracle, sets the tolerance of every device comparison); it imports neither
the package nor oracle/, and takes the target window, the nearest-point rule, the error measure and the tolerance from cl_reference.

THE POLICY.  B members, controller step dt_sim, QP horizon N at dt_mpc, n_replan sub-steps per period, n_replan dt_sim <= N dt_mpc.
Period p starts at t_p = t_start + p n_replan dt_sim.
  request    x0_p = x_hat0 of the reset for p = 0; for p > 0 the previous plan's states interpolated at tau = n_replan dt_sim: interval
             j = min(int(tau / dt_mpc), N - 1), theta = (tau - j dt_mpc) / dt_mpc (`end_point`, `request_state`).  Targets: the window
             at (t_p + phase_b) + dt_mpc k; zf its last row when the cost has Qf; u_des N rows (`targets`).
  solve      the trust-region-free QP with constant (A_mpc, B_mpc, d_mpc) -- not restated here.
  chain      row 0 of the plan's states <- x0_p; a member whose QP reports a non-zero status gets the previous plan moved up one row
             with its last row held, in period 0 x0_0 in every state row and zero inputs (`chain`).
  sub-steps  s = 0..n_replan-1 at tau = s dt_sim with (j_s, theta_s) of the schedule, ubar_s / xbar_s = lo + theta (hi - lo), the input
             held over the last interval (`advance`):
               1. y_s = (C x_s + y_ref) + v_s
               2. u_s = ubar_s + K (x_hat_s - xbar_s)
               3. x_hat_{s+1} = [F | B | L] [x_hat_s ; u_s ; y_s - y_ref] + d, F = A - L C
               4. x_{s+1} = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s, or x_{s+1} = X_plant[s + 1]."""
import numpy as np

from cl_reference import LD, err, nearest_with_margin, tolerance, window  # noqa: F401  (re-exported: one rule for both loops)


def end_point(N, dt_mpc, dt_sim, n_replan):
    """(j, theta) of tau = n_replan dt_sim in the plan: the schedule's rule (Python floats = IEEE doubles, every operation rounded)."""
    tau = n_replan * dt_sim
    j = min(int(tau / dt_mpc), N - 1)
    return j, (tau - j * dt_mpc) / dt_mpc


def request_state(xplan, j, theta, dtype):
    xplan = np.asarray(xplan, dtype=dtype)
    return xplan[j] + dtype(theta) * (xplan[j + 1] - xplan[j])


def chain(xsol, usol, x0, status, xprev, uprev, first, j_end, th_end, dtype):
    """The plan of a period after the fix-up, and the next request's state.  xsol (N+1, n), usol (N, m): the QP's answer."""
    c = lambda a: np.array(a, dtype=dtype)
    x0 = c(x0)
    if status == 0:
        xo, uo = c(xsol), c(usol)
    elif first:
        xo, uo = np.repeat(x0[None], np.shape(xsol)[0], axis=0), np.zeros(np.shape(usol), dtype=dtype)
    else:
        xo = np.concatenate((c(xprev)[1:], c(xprev)[-1:]))
        uo = np.concatenate((c(uprev)[1:], c(uprev)[-1:]))
    xo[0] = x0
    return xo, uo, request_state(xo, j_end, th_end, dtype)


def targets(t, z, u, t_p, phase, dt_mpc, N, has_Qf, dtype):
    """(z window (N+1, n_z) or None, zf or None, u_des (N, n_u) or None) of one member at period time t_p."""
    t0 = float(t_p) + float(phase)
    zw = None if z is None else window(t, z, t0, dt_mpc, N + 1, dtype)
    zf = zw[-1] if (has_Qf and zw is not None) else None
    uw = None if u is None else window(t, u, t0, dt_mpc, N, dtype)
    return zw, zf, uw


def advance(ctrl, plant, xopt, uopt, x, x_hat, j, theta, W, V, X_plant, dtype):
    """n_replan sub-steps of one member.  ctrl: dict A, B, d, C, y_ref, K, L, H of the controller's model; plant: dict q, v, w_q, w_v,
    A_d, B_d, d_d, or None with X_plant (n_replan + 1, n) the recorded plant (row 0 = x).  W (n_replan, n), V (n_replan, n_y) or None.
    Returns dict X, XH, Z (after every sub-step), Y, U, Ubar, Xbar (of every sub-step), picks (-1 in replay), margin."""
    c = lambda a: np.asarray(a, dtype=dtype)
    A, Bm, d, C, y_ref, K, L, H = (c(ctrl[k]) for k in ('A', 'B', 'd', 'C', 'y_ref', 'K', 'L', 'H'))
    F = A - L @ C
    xopt, uopt, x, xh = c(xopt), c(uopt), c(x), c(x_hat)
    uext = np.vstack((uopt, uopt[-1:]))
    if plant is not None and X_plant is None:
        Ad, Bd, dd = c(plant['A_d']), c(plant['B_d']), c(plant['d_d'])
    out = dict(X=[], XH=[], Z=[], Y=[], U=[], Ubar=[], Xbar=[], picks=[])
    margin = float('inf')
    for s in range(len(j)):
        js, th = int(j[s]), dtype(theta[s])
        x_bar = xopt[js] + th * (xopt[js + 1] - xopt[js])
        u_bar = uext[js] + th * (uext[js + 1] - uext[js])
        y = C @ x + y_ref
        if V is not None:
            y = y + c(V[s])
        u = u_bar + K @ (xh - x_bar)
        xh = F @ xh + Bm @ u + L @ (y - y_ref) + d
        if X_plant is not None:
            p, x = -1, c(X_plant[s + 1])
        else:
            p, mp = nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
            margin = min(margin, mp)
            x = Ad[p] @ x + Bd[p] @ u + dd[p]
            if W is not None:
                x = x + c(W[s])
        for k, v in (('X', x), ('XH', xh), ('Z', H @ x), ('Y', y), ('U', u), ('Ubar', u_bar), ('Xbar', x_bar), ('picks', p)):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items() if k != 'picks'}
    res['picks'] = np.array(out['picks'])
    res['margin'] = margin
    return res
