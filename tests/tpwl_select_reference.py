"""Extended-precision statement of the TPWL point selection behind csrc/tpwl_select.hip (test infrastructure only): the reference's
distance rule, sofacontrol/tpwl/tpwl_utils.py:156-196, as the sequential scan over recorded reduced states that INTEGRATION.md ("TPWL
model identification") defines.  Plain numpy in np.longdouble with tests/tpwl_table_reference.py's _norms and its RANGE rule; nothing here
imports the package under test or the oracle.

  candidates: all kept rows 0, s, 2s, .. of every episode of X (E, T, 2 r), x = [v; q], episode by episode in row order
  table:      starts as the seed (q0, v0); an empty table takes the first candidate unconditionally
  distances:  dq = w_q ||q_p - q_c||, dv = w_v ||v_p - v_c||; with w_v == 0 the velocity is not read and dv = 0
  decision:   separate False: taken iff min_p (dq + dv) >= threshold; True: iff min_p dq >= threshold or min_p dv >= threshold
              (the minimum over an empty table is +inf)
  cap:        the candidate that would be point max_points + 1 stops the scan (complete False, stopped_at = its episode and row)

scan_f64 is the float64 numpy restatement of tpwl_utils.py:171-196 (np.linalg.norm, np.min), one distance row per candidate.

THE CERTIFICATE.  A comparison d >= threshold of the scan (d = a minimum over the table) is decided when
  |d - threshold| / threshold > 32 (r + 4) eps -- the a-priori bound of tpwl_table_reference.decided for a computed distance -- or
  d is exact by construction: the case declares integer coordinates and unit (or zero) weights, and d is an integer.  Every difference
  and every partial sum of squares is then an integer below 2^53, the square root of a perfect square is exact and the weighted sum adds
  integers: float64 computes d without any rounding, so the comparison with ANY threshold is the exact one.  That covers d == threshold
  (3-4-5 offsets, threshold 5: `>=`, not `>`) and a threshold one ulp above d.
One undecided comparison can change every later decision, so a case is certified only when ALL comparisons of its scan are decided."""
import numpy as np

from lq_reference import LD
import tpwl_table_reference as tr

EPS = tr.EPS


def bound(r):
    return 32 * (r + 4) * EPS


def decided(d, threshold, r, exact=False):
    d = LD(d)
    if d != d:
        return False
    if abs(d - LD(threshold)) / LD(threshold) > bound(r):
        return True
    return bool(exact and d == np.floor(d))


def records(X):
    X = np.asarray(X, dtype=np.float64)
    return X[None] if X.ndim == 2 else X


def _seed(q0, v0, r):
    if q0 is None:
        return [], []
    return [np.asarray(p, dtype=np.float64) for p in np.reshape(q0, (-1, r))], [np.asarray(p, dtype=np.float64) for p in np.reshape(v0, (-1, r))]


def minima(qt, vt, x, r, w_q, w_v):
    """(min dq + dv, min dq, min dv) of the state x = [v; q] over the table (P, r arrays), in long double; +inf over an empty table."""
    if not len(qt):
        return LD(np.inf), LD(np.inf), LD(np.inf)
    with np.errstate(all='ignore'):
        dq = LD(w_q) * tr._norms(qt, x[r:])
        dv = LD(w_v) * tr._norms(vt, x[:r]) if w_v != 0 else np.zeros(len(qt), dtype=LD)
        return np.min(dq + dv), np.min(dq), np.min(dv)


def minima_f64(qt, vt, x, r, w_q, w_v):
    """tpwl_utils.py:179-184 in float64."""
    if not len(qt):
        return np.inf, np.inf, np.inf
    with np.errstate(all='ignore'):
        dq = w_q * np.linalg.norm(x[r:] - np.asarray(qt), axis=1)
        dv = w_v * np.linalg.norm(x[:r] - np.asarray(vt), axis=1)
        return np.min(dq + dv), np.min(dq), np.min(dv)


def scan(X, w_q, w_v, threshold, separate=False, stride=1, q0=None, v0=None, max_points=1024, minima=minima):
    """The sequential scan.  {'q', 'v' (P, r: seed first), 'index' (P_taken, 2), 'dmin' (P_taken,) or (P_taken, 2), 'complete',
    'stopped_at', 'candidates', 'comparisons': the minimum d of every comparison d >= threshold made, 'P0'}."""
    X = records(X)
    E, T, nx = X.shape
    r = nx // 2
    qt, vt = _seed(q0, v0, r)
    P0 = len(qt)
    qa, va = np.zeros((max(max_points, P0, 1), r)), np.zeros((max(max_points, P0, 1), r))      # the table as arrays, for the distances
    qa[:P0], va[:P0] = np.reshape(qt, (P0, r)), np.reshape(vt, (P0, r))
    index, dmin, comps = [], [], []
    stopped = None
    for ep in range(E):
        for row in range(0, T, stride):
            x = X[ep, row]
            d, dq, dv = minima(qa[:len(qt)], va[:len(qt)], x, r, w_q, w_v)
            if separate:
                comps += [dq, dv]
                take = bool(dq >= threshold) or bool(dv >= threshold)
            else:
                comps.append(d)
                take = bool(d >= threshold)
            if take:
                if len(qt) == max_points:
                    stopped = (ep, row)
                    break
                qa[len(qt)], va[len(vt)] = x[r:], x[:r]
                qt.append(x[r:].copy())
                vt.append(x[:r].copy())
                index.append((ep, row))
                dmin.append((dq, dv) if separate else d)
        if stopped:
            break
    return {'q': np.array(qt, dtype=np.float64).reshape(-1, r), 'v': np.array(vt, dtype=np.float64).reshape(-1, r),
            'index': np.array(index, dtype=np.int64).reshape(-1, 2), 'dmin': np.array(dmin, dtype=LD).reshape((-1, 2) if separate else (-1,)),
            'complete': stopped is None, 'stopped_at': stopped, 'candidates': E * ((T - 1) // stride + 1), 'comparisons': comps, 'P0': P0}


def scan_f64(X, w_q, w_v, threshold, **kw):
    return scan(X, w_q, w_v, threshold, minima=minima_f64, **kw)


def certified(res, threshold, r, exact=False):
    """(all comparisons decided, the undecided ones)."""
    bad = [float(d) for d in res['comparisons'] if not decided(d, threshold, r, exact)]
    return not bad, bad


def coverage(res, X, w_q, w_v, stride=1):
    """The largest distance (dq + dv, long double) of a kept row to its nearest point of the finished table."""
    X = records(X)
    r = X.shape[2] // 2
    qt, vt = res['q'], res['v']
    return max(minima(qt, vt, x, r, w_q, w_v)[0] for ep in range(X.shape[0]) for x in X[ep, ::stride])
