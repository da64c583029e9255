"""The TPWL horizon error ("TPWL horizon error") as its definition states it, parameterised by dtype: np.longdouble is
the reference, float64 the numpy restatement of TPWL's own formulas.  No GPU and no product import.

  kept rows 0, s, 2s, .. (T' of them); windows start at the kept rows j0 = 0, w, 2w, .. of every episode while j0 + H <= T' - 1, numbered
  episode by episode in row order;
  xh_0 = x_{j0}, xh_{k+1} = A_d[i] xh_k + B_d[i] u_{j0+k} + d_d[i], i = the first minimum over the points of w_q |q_p - q| + w_v |v_p - v|
  (tpwl_fit_reference.nearest: every search records its margin);
  e_k = xh_k - x_{j0+k}, ez_k = H e_k; status 0 ok, 1 some xh_k not finite, 2 some record row of the window not finite (2 wins);
  sse_x[k] = sum over the status-0 windows of |e_k|^2, sse_z alike; worst_x[k] = the largest |e_k|_2 and the FIRST window that attains it.

THE BOUNDS (eps = 2^-53), for the device's sums against the long-double evaluation of the device's OWN predictions:
  sse_x.  The device forms e_j = fl(xh_j - x_j): one rounding, so e_j^2 carries (1 + d)^2, 2 eps; the product inside an fma is exact.  A
  term then passes through additions only: at most n_x W of them in any order (lane sums, the wave's tree, the block's accumulator, the
  join), each (1 + d).  All terms are non-negative, so the relative errors do not cancel against anything larger than the sum itself:
  |sse_dev - sse| <= (n_x W + 2) eps sse, and one more eps covers the long-double evaluation itself (its e = xh - x is rounded to 64
  bits): (n_x W + 3) eps sse, for any order of summation.
  sse_z.  ez_a = sum_j H_aj e_j: the device's e_j carries one rounding and the dot product at most n_x additions (any order), so
  |ez_dev - ez| <= D_a := (n_x + 2) eps sum_j |H_aj e_j|.  Then |ez_dev^2 - ez^2| <= 2 |ez| D_a + D_a^2, and the squares are non-negative
  terms that pass through at most n_z W additions and their own rounding: |sse_z_dev - sse_z| <= sum (2 |ez| D_a + D_a^2) (1 + ..) +
  (n_z W + 3) eps sse_z.  sse_z_bound returns the sum with the first part inflated by (1 + 2^-20) for the second-order terms.
  A window's norm is the correctly rounded sqrt of its sum of squares: its SQUARE lies within the bounds above with W = 1, plus 2 eps of
  itself for the sqrt's rounding and one for squaring it back: norms are compared through their squares."""
import numpy as np

import tpwl_fit_reference as fr

LD = np.longdouble
EPS = 2.0 ** -53


def windows(E, T, H, stride, every):
    """(W, 2) int64: (episode, kept start row j0) of every window in window order, by the formula."""
    Tk = (T - 1) // stride + 1
    We = (Tk - 1 - H) // every + 1 if Tk > H else 0
    ep, k = np.divmod(np.arange(E * We, dtype=np.int64), max(We, 1))
    return np.stack([ep, k * every], axis=1).reshape(-1, 2)


def windows_brute(E, T, H, stride, every):
    out = []
    for e in range(E):
        kept = list(range(0, T, stride))
        for j0 in range(0, len(kept), every):
            if j0 + H <= len(kept) - 1:
                out.append((e, j0))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def fe_tables(mdl, dt, dtype=np.float64):
    """Forward-Euler tables of a case's model in float64 (exact inputs of both chains)."""
    n = mdl['A_c'].shape[1]
    return (np.eye(n)[None] + dt * mdl['A_c']).astype(np.float64), (dt * mdl['B_c']).astype(np.float64), (dt * mdl['d_c']).astype(np.float64)


def gather(X, U, wins, H, stride):
    """(Xw (W, H + 1, n_x), Uw (W, H, m)): the record rows every window reads."""
    Xk, Uk = X[:, ::stride], U[:, ::stride]
    rows = wins[:, 1:2] + np.arange(H + 1)[None]
    return Xk[wins[:, :1], rows], Uk[wins[:, :1], rows[:, :H]]


def predict(tabs, q, v, w, X, U, H, stride=1, every=1, dtype=LD):
    """dict: x_pred (W, H + 1, n_x) in dtype, status (W,), margin = the least search margin over the searches of status-0 windows,
    regions (W, H), switches = the changes of region inside windows."""
    Ad, Bd, dd = [np.asarray(t).astype(dtype) for t in tabs]
    wins = windows(X.shape[0], X.shape[1], H, stride, every)
    Xw, Uw = gather(X, U, wins, H, stride)
    W, n = wins.shape[0], X.shape[2]
    status = np.where(~(np.isfinite(Xw).all(axis=(1, 2)) & np.isfinite(Uw).all(axis=(1, 2))), 2, 0).astype(np.int32)
    xp = np.full((W, H + 1, n), np.nan, dtype=dtype)
    xp[:, 0] = Xw[:, 0].astype(dtype)
    reg = np.zeros((W, H), dtype=np.int64)
    margin = np.inf
    live = status == 0
    with np.errstate(all='ignore'):
        for k in range(H):
            x = xp[:, k]
            idx, mg = fr.nearest(np.where(np.isfinite(x), x, 0), q, v, w, dtype)
            reg[:, k] = idx
            if live.any():
                margin = min(margin, float(np.min(mg[live])))
            u = Uw[:, k].astype(dtype)
            nxt = np.zeros((W, n), dtype=dtype)
            for p in np.unique(idx):
                s = idx == p
                nxt[s] = x[s] @ Ad[p].T + u[s] @ Bd[p].T + dd[p]
            xp[:, k + 1] = nxt
            fin = np.isfinite(nxt.astype(np.float64)).all(axis=1) if dtype is not np.float64 else np.isfinite(nxt).all(axis=1)
            status[live & ~fin] = 1
            live = live & fin
    sw = int((reg[status == 0][:, 1:] != reg[status == 0][:, :-1]).sum()) if H > 1 else 0
    return dict(x_pred=xp, status=status, margin=margin, regions=reg, switches=sw, windows=wins, Xw=Xw, Uw=Uw)


def curves(x_pred, Xw, Hm, status):
    """The long-double evaluation of predictions (any dtype) against the record rows Xw: dict of sq_x, sq_z (W, H + 1) per window,
    sse_x, sse_z (H + 1), worst_x, worst_z (H + 1) and their FIRST windows wx, wz (H + 1; -1 without a status-0 window), and the
    absolute sums az (W, H + 1, n_z) = sum_j |H_aj e_j| with ez (W, H + 1, n_z) that the z bound is stated on."""
    ok = status == 0
    with np.errstate(all='ignore'):
        e = np.asarray(x_pred).astype(LD) - Xw.astype(LD)
        e[~ok] = 0
        sq_x = (e * e).sum(axis=2)
        out = dict(ok=ok, sq_x=sq_x, sse_x=sq_x[ok].sum(axis=0))
        if Hm is not None:
            Hl = np.asarray(Hm).astype(LD)
            ez = e @ Hl.T
            az = np.abs(e) @ np.abs(Hl).T
            sq_z = (ez * ez).sum(axis=2)
            out.update(ez=ez, az=az, sq_z=sq_z, sse_z=sq_z[ok].sum(axis=0))
    for name in ('x', 'z') if Hm is not None else ('x',):
        sq = np.where(ok[:, None], out['sq_' + name], -1)
        out['worst_' + name] = np.sqrt(np.maximum(sq.max(axis=0), 0)) if ok.any() else np.full(sq.shape[1], np.nan)
        out['w' + name] = np.argmax(sq, axis=0) if ok.any() else np.full(sq.shape[1], -1)          # np.argmax: the first maximum
    return out


def sse_x_bound(cv, n_x, W=None):
    """(H + 1,) the bound on |sse_x_dev - sse_x|; W = the status-0 windows (per-window squares: W = 1 and cv['sq_x'])."""
    W = int(cv['ok'].sum()) if W is None else W
    return (n_x * W + 3) * EPS * cv['sse_x']


def sq_x_bound(cv, n_x):
    return (n_x + 3) * EPS * cv['sq_x']


def _z_terms(cv, n_x):
    D = (n_x + 2) * EPS * cv['az']
    return ((2 * np.abs(cv['ez']) * D + D * D).sum(axis=2)) * (1 + 2.0 ** -20)


def sse_z_bound(cv, n_x, n_z):
    W = int(cv['ok'].sum())
    return _z_terms(cv, n_x)[cv['ok']].sum(axis=0) + (n_z * W + 3) * EPS * cv['sse_z']


def sq_z_bound(cv, n_x, n_z):
    return _z_terms(cv, n_x) + (n_z + 3) * EPS * cv['sq_z']


def norm_sq_check(norm, sq_ref, sq_bound):
    """True where a norm (float64: a correctly rounded sqrt of a sum within sq_bound of sq_ref) is consistent: its square lies within
    sq_bound + 3 eps sq_ref (2 eps for the sqrt's rounding, squared back in long double)."""
    nl = np.asarray(norm).astype(LD)
    return np.abs(nl * nl - sq_ref) <= sq_bound * (1 + 4 * EPS) + 3 * EPS * sq_ref


def top_gap(sq, ok):
    """(H + 1,) the relative gap between the largest and the second largest DISTINCT-window square (inf with one window): the device's
    argmax is decided by rounding only when this is below the bound."""
    s = np.sort(np.where(ok[:, None], sq, -1).astype(LD), axis=0)
    if s.shape[0] < 2:
        return np.full(s.shape[1], np.inf)
    with np.errstate(all='ignore'):
        return np.where(s[-1] > 0, (s[-1] - s[-2]) / s[-1], np.inf).astype(np.float64)
