"""Reference statement of the batched closed-loop Koopman MPC (csrc/koopman_loop.hip), one member at a time: the policy of
sofacontrol/baselines/koopman/koopman.py:75-170 (compute_policy, evaluate), koopman_utils.py:16-47 (add_measurement, get_zeta), 86-107
(KoopmanScaling), 156-175 (the observables' order) and baselines/ros.py:223-227 (failure shift), around the solve.  The same code runs in
np.longdouble (the reference) and in np.float64 (the oracle whose distance from the reference, e_oracle, sets the tolerance of every
device comparison); it imports neither the package nor oracle/, and takes the target window, the nearest-point rule, the error measure
and the tolerance from cl_reference.

THE POLICY.  Controller step Ts, simulation step dt_sim, Ts = r dt_sim; rollout_horizon = rh, n_keep = rh r sub-steps per period; period
p starts at t_p = t_start + p n_keep dt_sim.
  reset      the history <- the `delays` older raw samples, oldest first, then (y_0, u_prev0), all scaled down (`scale_down`)
  request    x0_p = W psi(zeta) of the last delays + 1 samples (`zeta_of`, `lift`); targets: `window` at (t_p + phase) + Ts k
  solve      the trust-region-free QP with constant (A, B), d = 0 -- not restated here
  fix-up     a failed member goes on with the previous plan moved up one row, its last row held; in period 0 x0 in every state row and
             the scaled-down u0 in every input row (`fixup`)
  sub-steps  s = 0..n_keep-1 (`advance`): u_s = uopt[s // r] * u_factor + u_offset; x_{s+1} = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the
             plant's nearest point to x_s; y_{s+1} = (C x_{s+1} + y_ref) + v_s, or Y_plant[s + 1]; the sample (y_{s+1}, u_s) -- or
             (y_{s+1}, U_applied[s]) -- scaled down, joins the history."""
import itertools

import numpy as np

from cl_reference import LD, err, nearest_with_margin, tolerance, window  # noqa: F401  (re-exported: one rule for all loops)


def exponents(nzeta, degree, dmd):
    """(n_psi, nzeta) exponents of the observables in the order of get_lifting_function: graded, within a degree ascending in the
    exponent tuple read from the LAST variable to the first; then the constant (all zeros), unless dmd."""
    rows = []
    for deg in range(1, degree + 1):
        lvl = _level(nzeta, deg)
        rows += sorted(lvl, key=lambda e: e[::-1])
    if not dmd:
        rows.append((0,) * nzeta)
    return np.array(rows, dtype=np.int64)


def _level(nzeta, deg):
    """Every exponent tuple of total degree deg (multisets of `deg` variables)."""
    out = []
    for combo in itertools.combinations_with_replacement(range(nzeta), deg):
        e = [0] * nzeta
        for v in combo:
            e[v] += 1
        out.append(tuple(e))
    return out


def scale_down(v, off, fac, dtype):
    return (np.asarray(v, dtype=dtype) - np.asarray(off, dtype=dtype).ravel()) / np.asarray(fac, dtype=dtype).ravel()


def scale_up(v, off, fac, dtype):
    return np.asarray(v, dtype=dtype) * np.asarray(fac, dtype=dtype).ravel() + np.asarray(off, dtype=dtype).ravel()


def zeta_of(hist_y, hist_u, delays, dtype):
    """[y_t, y_{t-1} .. y_{t-d}, u_{t-1} .. u_{t-d}] of the scaled histories (rows oldest first; sample t is the last row, and row k
    of hist_u is the input pushed WITH y_k, the one applied before it -- get_zeta reads u_norm[step - (j + 1)])."""
    hy, hu = np.asarray(hist_y, dtype=dtype), np.asarray(hist_u, dtype=dtype)
    return np.concatenate([hy[-1]] + [hy[-1 - (j + 1)] for j in range(delays)] + [hu[-1 - (j + 1)] for j in range(delays)])


def lift(spec, hist_y, hist_u, dtype):
    """W psi(zeta) of the scaled histories.  spec: dict delays, degree, dmd, W (n_w, n_psi) or None."""
    z = zeta_of(hist_y, hist_u, spec['delays'], dtype)
    E = exponents(len(z), spec['degree'], spec['dmd'])
    psi = np.array([np.prod([z[i] ** int(e[i]) for i in range(len(z)) if e[i]] or [dtype(1)]) for e in E], dtype=dtype)
    W = spec.get('W')
    return psi if W is None else np.asarray(W, dtype=dtype) @ psi


def fixup(xsol, usol, x0, status, xprev, uprev, first, u0_scaled, dtype):
    """The plan of a period after the fix-up.  xsol (N+1, n), usol (N, m): the QP's answer."""
    c = lambda a: np.array(a, dtype=dtype)
    if status == 0:
        return c(xsol), c(usol)
    if first:
        return np.repeat(c(x0)[None], np.shape(xsol)[0], axis=0), np.repeat(c(u0_scaled)[None], np.shape(usol)[0], axis=0)
    return np.concatenate((c(xprev)[1:], c(xprev)[-1:])), np.concatenate((c(uprev)[1:], c(uprev)[-1:]))


def advance(spec, plant, C, y_ref, uopt, x, r, n_keep, W, V, Y_plant, U_applied, dtype):
    """n_keep sub-steps of one member.  spec: dict y_offset, y_factor, u_offset, u_factor; plant: dict q, v, w_q, w_v, A_d, B_d, d_d, or
    None with Y_plant (n_keep + 1, n_y) the recorded measurements (row 0 = where the launch starts); uopt (N, m) the scaled plan; x
    (n_plant); W (n_keep, n_plant), V (n_keep, n_y), U_applied (n_keep, m) or None.
    Returns dict X (None in replay), Y, U (raw), ring (n_keep, n_y + m) the scaled samples pushed, picks (-1 in replay), margin."""
    c = lambda a: np.asarray(a, dtype=dtype)
    uopt = c(uopt)
    replay = Y_plant is not None
    if not replay:
        Ad, Bd, dd, Cm, yr, x = c(plant['A_d']), c(plant['B_d']), c(plant['d_d']), c(C), c(y_ref), c(x)
    out = dict(X=[], Y=[], U=[], ring=[], picks=[])
    margin = float('inf')
    for s in range(n_keep):
        u = scale_up(uopt[s // r], spec['u_offset'], spec['u_factor'], dtype)
        if replay:
            p, y = -1, c(Y_plant[s + 1])
        else:
            p, mp = nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
            margin = min(margin, mp)
            x = Ad[p] @ x + Bd[p] @ u + dd[p]
            if W is not None:
                x = x + c(W[s])
            y = Cm @ x + yr
            if V is not None:
                y = y + c(V[s])
            out['X'].append(x)
        pushed_u = u if U_applied is None else c(U_applied[s])
        out['ring'].append(np.concatenate((scale_down(y, spec['y_offset'], spec['y_factor'], dtype),
                                           scale_down(pushed_u, spec['u_offset'], spec['u_factor'], dtype))))
        out['Y'].append(y); out['U'].append(u); out['picks'].append(p)
    res = {k: (np.stack(v) if v else None) for k, v in out.items() if k != 'picks'}
    res['picks'] = np.array(out['picks'])
    res['margin'] = margin
    return res


def replay(spec, y_hist, u_hist, y0, u_prev0, Y_plant, U_applied, r, rh, periods, t_start, dt_sim, solve, u0_scaled, dtype=np.float64):
    """The loop of one member on a recorded plant.  y_hist (delays, n_y), u_hist (delays, m): the older raw samples, oldest first; (y0,
    u_prev0) the sample at the first solve; Y_plant (S + 1, n_y) with row 0 = y0; U_applied (S, m) or None: the loop's own inputs join the
    history.  solve(p, t_p, x0) -> (xopt (N+1, n), uopt (N, m) scaled, status).
    Returns dict t (periods + 1,), x_lift (periods, n_lift), u (S, m) raw, y (S + 1, n_y), status (periods,)."""
    ny, n_keep = len(np.ravel(y0)), rh * r
    sd_y = lambda v: scale_down(v, spec['y_offset'], spec['y_factor'], dtype)
    sd_u = lambda v: scale_down(v, spec['u_offset'], spec['u_factor'], dtype)
    hy = [sd_y(v) for v in y_hist] + [sd_y(y0)]
    hu = [sd_u(v) for v in u_hist] + [sd_u(u_prev0)]
    step = n_keep * dt_sim
    out = dict(t=[], x_lift=[], u=[], y=[np.asarray(y0, dtype=dtype).ravel()], status=[])
    xprev = uprev = None
    for p in range(periods):
        t_p = t_start + p * step
        x0 = lift(spec, hy, hu, dtype)
        xs, us, status = solve(p, t_p, x0)
        xo, uo = fixup(xs, us, x0, status, xprev, uprev, p == 0, u0_scaled, dtype)
        rows = slice(p * n_keep, (p + 1) * n_keep)
        adv = advance(spec, None, None, None, uo, None, r, n_keep, None, None, Y_plant[p * n_keep:(p + 1) * n_keep + 1],
                      None if U_applied is None else U_applied[rows], dtype)
        hy += list(adv['ring'][:, :ny]); hu += list(adv['ring'][:, ny:])
        out['t'].append(t_p); out['x_lift'].append(x0); out['u'] += list(adv['U']); out['y'] += list(adv['Y']); out['status'].append(status)
        xprev, uprev = xo, uo
    out['t'].append(t_start + periods * step)
    return {k: np.array(v) for k, v in out.items()}
