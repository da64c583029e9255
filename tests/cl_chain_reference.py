"""Reference statement of the chained policy of the batched closed loop (the reference's `mpc=False`, tpwl/controllers.py:269-274 and
update_policy, 298-315): where the next plan starts, and the rows one period adds to the nominal tape.  The same code runs in
np.longdouble (the reference) and in np.float64 (the oracle whose distance from the reference, e_oracle, sets the tolerance of every
device comparison, cl_reference.tolerance); it imports neither the package nor oracle/.

update_policy reads the plan (t_opt_p = t0 + dt arange(N + 1), x_opt_p, [u_opt_p; u_opt_p[-1]]) with interp1d at t0 + dt_sim s,
s = 0..n_keep.  In the loop's own terms that is, for tau = s dt_sim, the interval j = min(int(tau / dt), N - 1), the position
theta = (tau - j dt) / dt and the point lo + theta (hi - lo): `direct_end` states (j, theta) of the last of them, s = n_keep, as
cl_cases.direct_schedule states the others."""
import numpy as np

import cl_cases as cc
import cl_reference as cr


def direct_end(N, dt, dt_sim, n_keep):
    """(j_end, theta_end) stated directly (scalars, Python floats = IEEE doubles)."""
    tau = n_keep * dt_sim
    j = min(int(tau / dt), N - 1)
    return j, (tau - j * dt) / dt


def period_rows(xopt, uopt, j, theta, j_end, theta_end, dtype):
    """One plan (xopt (N+1, n), uopt (N, m)) read at the sub-steps (j, theta) and at the period's end: x rows (n_keep + 1, n), u rows
    (n_keep + 1, m); the input is held over the plan's last interval (controllers.py:299).  The last x row is x_opt[-1], the next
    plan's start state (controllers.py:272)."""
    xopt, uopt = np.asarray(xopt, dtype=dtype), np.asarray(uopt, dtype=dtype)
    uext = np.vstack((uopt, uopt[-1:]))
    js = [int(v) for v in j] + [int(j_end)]
    ths = [dtype(v) for v in theta] + [dtype(theta_end)]
    X = np.stack([xopt[a] + th * (xopt[a + 1] - xopt[a]) for a, th in zip(js, ths)])
    U = np.stack([uext[a] + th * (uext[a + 1] - uext[a]) for a, th in zip(js, ths)])
    return X, U


def chain_case(case, dtype):
    """The rows of every member of an ADVANCE row of cl_cases: X (B, n_keep + 1, n), U (B, n_keep + 1, m); X[:, -1] is the chain point."""
    name, mname, B, dt_sim, n_keep = case[:5]
    c = cc.advance_case(case)
    j_end, theta_end = direct_end(cc.N, cc.DT, dt_sim, n_keep)
    rows = [period_rows(c['xopt'][b], c['uopt'][b], c['j'], c['theta'], j_end, theta_end, dtype) for b in range(B)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def e_oracle(case):
    ref, f64 = chain_case(case, cr.LD), chain_case(case, np.float64)
    return max(cr.err(f64[0], ref[0]), cr.err(f64[1], ref[1]))


def stitch(rows):
    """The tape of consecutive periods from their rows [(X_k, U_k)], by the loop's rule: x row k n_keep (k >= 1) stays the OLD plan's
    end (row 0 of a later period is dropped), u row k n_keep is the NEW plan's first row (the old plan's end row gives way)."""
    X = np.concatenate([rows[0][0]] + [r[0][1:] for r in rows[1:]])
    U = np.concatenate([r[1][:-1] for r in rows[:-1]] + [rows[-1][1]])
    return X, U


def chained_plans(case, periods, member=0):
    """`periods` synthetic plans of one loop that chain: plan k + 1 is a plan of the ADVANCE row (members taken in turn, seeds apart)
    moved so that its row 0 IS the float64 chain point of plan k -- what a solve from that x0 returns when xopt[0] = x0."""
    name, mname, B, dt_sim, n_keep = case[:5]
    j_end, theta_end = direct_end(cc.N, cc.DT, dt_sim, n_keep)
    plans = []
    for k in range(periods):
        c = cc.advance_case(case[:7] + (case[7] + 100 * k,))
        xo, uo = c['xopt'][member % B].copy(), c['uopt'][member % B].copy()
        if plans:
            px, pu = plans[-1]
            xo[0] = px[j_end] + theta_end * (px[j_end + 1] - px[j_end])
        plans.append((xo, uo))
    return plans
