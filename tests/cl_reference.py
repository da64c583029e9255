"""Reference statement of one period of the batched closed loop (csrc/gusto_loop.hip) around the solve: the shift of the previous plan
(scp/ros.py:110-114), the target window (scp/standalone.py:29, 46-53) and the plant advance under the scp controller's feedback law
(tpwl/controllers.py:298-333, tpwl/tpwl.py:160-168, 336-339).  The same code runs in np.longdouble (the reference) and in np.float64
(the oracle whose distance from the reference, e_oracle, sets the tolerance of every device comparison); it imports neither the package
nor oracle/.  Every nearest-point lookup records the relative gap between the two smallest distances."""
import numpy as np

LD = np.longdouble
TOL_FLOOR = 1e-13
E_ORACLE_MAX = 1e-11
MARGIN = 1e-6


def err(a, b):
    """max|a - b| / max(1, max|b|)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / max(LD(1), np.abs(b).max()))


def tolerance(e_oracle):
    return max(100.0 * e_oracle, TOL_FLOOR)


def shift(xopt, uopt, idx0):
    """Rows idx0.. of the previous plan to the front, its last row held over the rest (copies, any dtype)."""
    N = uopt.shape[0]
    u_init = np.repeat(uopt[-1:], N, axis=0)
    u_init[:N - idx0] = uopt[idx0:]
    x_init = np.repeat(xopt[-1:], N + 1, axis=0)
    x_init[:N + 1 - idx0] = xopt[idx0:]
    return u_init, x_init


def window(t, y, t0, dt, rows, dtype):
    """y interpolated linearly at t0 + dt j, j = 0..rows-1; the first / last row of the table outside it."""
    t, y = np.asarray(t, dtype=dtype), np.asarray(y, dtype=dtype)
    out = np.zeros((rows, y.shape[1]), dtype=dtype)
    for j in range(rows):
        tq = dtype(t0) + dtype(dt) * dtype(j)
        if tq < t[0]:
            out[j] = y[0]
        elif tq > t[-1]:
            out[j] = y[-1]
        else:
            i = min(max(int(np.searchsorted(t, tq)), 1), len(t) - 1)
            slope = (y[i] - y[i - 1]) / (t[i] - t[i - 1])
            out[j] = slope * (tq - t[i - 1]) + y[i - 1]
    return out


def nearest_with_margin(q, v, w_q, w_v, x, dtype):
    """argmin_i w_q |q_i - q| + w_v |v_i - v| for x = [v; q] (first minimum) and the relative gap of the two smallest distances."""
    q, v, x = np.asarray(q, dtype=dtype), np.asarray(v, dtype=dtype), np.asarray(x, dtype=dtype)
    r = q.shape[1]
    dist = dtype(w_q) * np.sqrt(((q - x[r:]) ** 2).sum(axis=1)) + dtype(w_v) * np.sqrt(((v - x[:r]) ** 2).sum(axis=1))
    i = int(np.argmin(dist))
    if len(dist) == 1:
        return i, float('inf')
    rest = np.delete(dist, i)
    d1 = rest.min()
    return i, float((d1 - dist[i]) / max(d1, dtype(1e-300)))


def advance(planner, plant, H, K, xopt, uopt, x, j, theta, W, dtype):
    """n_keep sub-steps of one loop.  planner / plant: dicts q, v, w_q, w_v (+ A_d, B_d, d_d for the plant); H (n_z, n_x); K (P, n_u, n_x)
    or None; xopt (N+1, n_x), uopt (N, n_u); x (n_x); j, theta (n_keep); W (n_keep, n_x) or None.
    Returns X (n_keep, n_x), U, Z, plant picks, gain picks (-1 without gains), the least margin."""
    c = lambda a: np.asarray(a, dtype=dtype)
    xopt, uopt, x, H = c(xopt), c(uopt), c(x), c(H)
    Ad, Bd, dd = c(plant['A_d']), c(plant['B_d']), c(plant['d_d'])
    K = None if K is None else c(K)
    uext = np.vstack((uopt, uopt[-1:]))
    X, U, Z, ip, ig, margin = [], [], [], [], [], float('inf')
    for s in range(len(j)):
        js, th = int(j[s]), dtype(theta[s])
        x_bar = xopt[js] + th * (xopt[js + 1] - xopt[js])
        u = uext[js] + th * (uext[js + 1] - uext[js])
        g = -1
        if K is not None:
            g, mg = nearest_with_margin(planner['q'], planner['v'], planner['w_q'], planner['w_v'], x_bar, dtype)
            margin = min(margin, mg)
            u = u + K[g] @ (x - x_bar)
        p, mp = nearest_with_margin(plant['q'], plant['v'], plant['w_q'], plant['w_v'], x, dtype)
        margin = min(margin, mp)
        x = Ad[p] @ x + Bd[p] @ u + dd[p]
        if W is not None:
            x = x + c(W[s])
        X.append(x); U.append(u); Z.append(H @ x); ip.append(p); ig.append(g)
    return np.stack(X), np.stack(U), np.stack(Z), np.array(ip), np.array(ig), margin
