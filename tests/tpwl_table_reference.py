"""Extended-precision statement of the TPWL table operations behind csrc/tpwl_dev.h and csrc/tpwl.hip (test infrastructure only):
the distances to the stored points, the nearest point, the softmin weights and the blended tables, as sofacontrol/tpwl/tpwl.py:160-191 and
244-248 state them.  Plain numpy in np.longdouble (80-bit on x86: eps 1.1e-19), like tests/lq_reference.py and tests/ekf_reference.py.
Nothing here imports the package under test or the float64 oracle: oracle/tpwl.py is *measured* against this module
(tests/test_tpwl_table_reference_cpu.py) and the kernels are held to it (tests/test_tpwl_table_exact_gpu.py).

A model is the dict of oracle/tpwl.py: q (P, r), v (P, r), w_q, w_v and the tables; the state is x = [v; q].

  d_i = w_q ||q_i - q|| + w_v ||v_i - v||
  nearest point: first_min(d), the smallest index among the minima (np.argmin)
  weights:       w_i = exp(-beta d_i / d_min) / sum_j exp(-beta d_j / d_min); one-hot at the first minimum when d_min == 0
  blend:         sum_i w_i T_i

Three rules that the reference's float64 code leaves to the number format are stated here:
  - NO MINIMUM.  If no d_i is a number below +inf (all +inf, or all NaN: a diverged state, a NaN of a failed solve upstream), the
    index is 0 -- what np.argmin returns for such a vector, and an index of the table.
  - RANGE.  The distances are float64 quantities: a squared norm above the largest float64 is +inf (a finite state of 1e200 "overflows"
    although 80 bits could hold its square).
  - w_v == 0 DOES NOT READ THE VELOCITY.  The product skips the velocity term when w_v == 0 on every search path, so a NaN in the
    velocity part of the state changes nothing there.  numpy's 0 * NaN would make every d_i NaN and the index 0 (INTEGRATION.md,
    behavioural notes).  w_q is always applied: w_q = 0 with a NaN position gives NaN distances and the index 0."""
import numpy as np

from lq_reference import LD, ld

EPS = float(np.finfo(np.float64).eps)
F64_MAX = LD(np.finfo(np.float64).max)


def _norms(tab, y):
    sq = ((ld(tab) - ld(y)) ** 2).sum(axis=1)
    sq = np.where(sq > F64_MAX, LD(np.inf), sq)               # RANGE (a NaN compares false and stays)
    return np.sqrt(sq)


def distances(model, x):
    """d (P,) in long double for the state x = [v; q]."""
    r = model['q'].shape[1]
    x = np.asarray(x)
    with np.errstate(all='ignore'):
        d = LD(model['w_q']) * _norms(model['q'], x[r:])
        if model['w_v'] != 0:
            d = d + LD(model['w_v']) * _norms(model['v'], x[:r])
    return d


def first_min(d):
    """The smallest index among the minima of d; 0 when no d_i is a number below +inf."""
    d = np.asarray(d)
    ok = d < np.inf
    if not ok.any():
        return 0
    return int(np.flatnonzero(d == d[ok].min())[0])


def nearest(model, X):
    return np.array([first_min(distances(model, x)) for x in np.atleast_2d(X)], dtype=np.int32)


def decided(d, r):
    """True when float64 arithmetic cannot change first_min(d): the relative gap between the smallest and the second-smallest DISTINCT
    distance exceeds 32 (r + 4) eps: four times 8 (r + 4) eps, a generous a-priori bound on the relative error with which float64
    compares two computed distances (each one: two r-term fma sums of squared rounded differences, two square roots, the weighted
    sum -- about (r + 11) eps / 4 to first order).  Exact ties are decided: the first index wins, and the cases build them so that no
    rounding can break them (identical rows, mirrored dyadic offsets).  A vector without a number below +inf is decided by the NO
    MINIMUM rule."""
    d = np.asarray(d)
    vals = np.unique(d[d < np.inf])
    if len(vals) < 2:
        return True
    return bool((vals[1] - vals[0]) / vals[1] > 32 * (r + 4) * EPS)


def weights(model, x, beta):
    """(P,) long double; a state that is not a number gives a row of NaN."""
    d = distances(model, x)
    i = first_min(d)
    m = d[i]
    if m == 0:
        w = np.zeros(len(d), dtype=LD)
        w[i] = 1
        return w
    with np.errstate(all='ignore'):
        w = np.exp(-LD(beta) * d / m)
        return w / w.sum()


def blend(W, T):
    """sum_i w_i T_i for one weight row W (P,) and a table T (P, ...), in long double."""
    return np.tensordot(ld(W), ld(T), axes=1)


def blend_abs(W, T):
    """sum_i |w_i T_i|: the scale of the blend's rounding error."""
    return np.tensordot(np.abs(ld(W)), np.abs(ld(T)), axes=1)


def rollout(model, Ad, Bd, dd, x0, u):
    """x_{k+1} = A_d[i_k] x_k + B_d[i_k] u_k + d_d[i_k], i_k = first_min(d(x_k)): the states (N + 1, n) and the indices (N,)."""
    Ad, Bd, dd, u = ld(Ad), ld(Bd), ld(dd), ld(u)
    x = np.zeros((u.shape[0] + 1, len(x0)), dtype=LD)
    x[0] = ld(x0)
    idx = np.zeros(u.shape[0], dtype=np.int32)
    for k in range(u.shape[0]):
        i = idx[k] = first_min(distances(model, x[k]))
        x[k + 1] = Ad[i] @ x[k] + Bd[i] @ u[k] + dd[i]
    return x, idx
