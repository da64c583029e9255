"""The SSM horizon error ("SSM horizon error") as its definition states it, parameterised by dtype: np.longdouble is the
reference (tests/ssm_reference.py: reduce, rollout, observe), float64 the restatement through oracle/ssm.py.  No GPU and no product import.

  kept rows 0, s, 2s, .. (T' of them); xo_j = V phi_s(y_j - z_ref) for every kept row; windows start at the kept rows j0 = 0, w, 2w, .. of
  every episode while j0 + H <= T' - 1, numbered episode by episode in row order (tpwl_horizon_reference.windows: the same rule);
  xh_0 = xo_{j0} (or x_start), xh_{k+1} = A_d xh_k + B_d u_{j0+k} + d_d re-linearised at every (xh_k, u_{j0+k}), zh_k = C_map(xh_k) + z_ref;
  ex_k = xh_k - xo_{j0+k}, ez_k = zh_k - y_{j0+k}; status 0 ok, 1 some xh_k or zh_k not finite, 2 some record row of the window not finite
  (y at j0 .. j0 + H, u at j0 .. j0 + H - 1; 2 wins: such a window is not rolled out);
  sse_x[k], sse_z[k] = sums over the status-0 windows; worst = the largest norm and the FIRST window that attains it.

THE BOUNDS (eps = 2^-53), for the device's sums against the long-double evaluation of the device's OWN x_pred, z_pred and x_obs.  Both
errors are one subtraction of returned numbers: the device forms e_j = fl(a_j - b_j), one rounding, so e_j^2 carries (1 + d)^2, 2 eps; the
product inside an fma is exact.  A term then passes through additions only: at most dim W of them in any order (lane sums, the wave's
tree, the block's accumulator, the join), each (1 + d).  All terms are non-negative, so |sse_dev - sse| <= (dim W + 2) eps sse, and one
more eps covers the long-double evaluation itself: (dim W + 3) eps sse for any order of summation (dim = n_x for ex, n_o for ez) -- the
derivation of tpwl_horizon_reference.sse_x_bound.  A window's norm is the correctly rounded sqrt of its sum of squares: its SQUARE lies
within the bound with W = 1, plus 2 eps for the sqrt and one for squaring it back (tpwl_horizon_reference.norm_sq_check)."""
import numpy as np

import ssm_reference as sr
import tpwl_horizon_reference as hr
from oracle import ssm as ossm

LD = np.longdouble
EPS = hr.EPS
windows, windows_brute, norm_sq_check, top_gap = hr.windows, hr.windows_brute, hr.norm_sq_check, hr.top_gap


def gather(Yk, Uk, Xo, wins, H):
    """(Yw (W, H + 1, n_o), Uw (W, H, m), Xow (W, H + 1, n_x)): the kept rows every window reads."""
    rows = wins[:, 1:2] + np.arange(H + 1)[None]
    return Yk[wins[:, :1], rows], Uk[wins[:, :1], rows[:, :H]], Xo[wins[:, :1], rows]


def predict(M, method, dt, Y, U, H, stride=1, every=1, x_start=None, dtype=LD):
    """M: the model of ssm_reference.make_model (dtype LD) or oracle.ssm.make_model (float64); method 'fe' | 'be' | 'bil' | 'map'.
    dict: x_obs (E, T', n_x), x_pred (W, H + 1, n_x), z_pred (W, H + 1, n_o) in dtype (NaN behind the row at which a window left its
    loop; all NaN for status 2), status (W,), windows (W, 2), Yw, Uw, Xow."""
    ld = dtype is LD
    E, T, n = Y.shape[0], Y.shape[1], M['n']
    Yk, Uk = Y[:, ::stride], U[:, ::stride]
    wins = windows(E, T, H, stride, every)
    with np.errstate(all='ignore'):
        Xo = np.array([[sr.reduce(M, y) if ld else ossm.reduce(M, y) for y in Ye] for Ye in Yk], dtype=dtype)
    Yw, Uw, Xow = gather(Yk, Uk, Xo, wins, H)
    W = wins.shape[0]
    status = np.where(~(np.isfinite(Yw).all(axis=(1, 2)) & np.isfinite(Uw).all(axis=(1, 2))), 2, 0).astype(np.int32)
    xp, zp = np.full((W, H + 1, n), np.nan, dtype=dtype), np.full((W, H + 1, M['n_o'] if ld else n), np.nan, dtype=dtype)
    with np.errstate(all='ignore'):
        for w in range(W):
            if status[w]:
                continue
            x0 = Xow[w, 0] if x_start is None else np.asarray(x_start, dtype=dtype)
            if ld:
                x, z = sr.rollout(M, x0, Uw[w], dt, method)
            else:
                x, z = ossm.rollout(M, x0, Uw[w], dt, 'fe' if method == 'map' else method, discrete=method == 'map')
            fin = np.isfinite(np.asarray(x, dtype=np.float64)).all(axis=1) & np.isfinite(np.asarray(z, dtype=np.float64)).all(axis=1)
            last = H if fin.all() else int(np.argmin(fin))                # the row at which the window leaves its loop
            xp[w, :last + 1], zp[w, :last + 1] = x[:last + 1], z[:last + 1]
            if not fin.all():
                status[w] = 1
    return dict(x_obs=Xo, x_pred=xp, z_pred=zp, status=status, windows=wins, Yw=Yw, Uw=Uw, Xow=Xow)


def curves(x_pred, z_pred, Xow, Yw, status):
    """The long-double evaluation of predictions (any dtype) against the observed states and the record rows: dict of ok, sq_x, sq_z
    (W, H + 1) per window, sse_x, sse_z (H + 1), worst_x, worst_z (H + 1) and their FIRST windows wx, wz (-1 without a status-0 window)."""
    ok = status == 0
    out = dict(ok=ok)
    with np.errstate(all='ignore'):
        for name, a, b in (('x', x_pred, Xow), ('z', z_pred, Yw)):
            e = np.asarray(a).astype(LD) - np.asarray(b).astype(LD)
            e[~ok] = 0
            sq = (e * e).sum(axis=2)
            out['sq_' + name], out['sse_' + name] = sq, sq[ok].sum(axis=0)
            sqm = np.where(ok[:, None], sq, -1)
            out['worst_' + name] = np.sqrt(np.maximum(sqm.max(axis=0), 0)) if ok.any() else np.full(sq.shape[1], np.nan)
            out['w' + name] = np.argmax(sqm, axis=0) if ok.any() else np.full(sq.shape[1], -1)      # np.argmax: the first maximum
    return out


def sse_bound(sse, dim, W):
    """(H + 1,) the bound on |sse_dev - sse| over W status-0 windows of `dim` entries; per-window squares: W = 1."""
    return (dim * W + 3) * EPS * sse


def rel_err(got, ref):
    """max |got - ref| relative to the largest entry of ref (finite entries of ref only), in long double."""
    got, ref = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
    m = np.isfinite(ref.astype(np.float64))
    scale = np.abs(ref[m]).max()
    return float(np.abs(got[m] - ref[m]).max() / scale) if scale > 0 else float(np.abs(got[m]).max())
