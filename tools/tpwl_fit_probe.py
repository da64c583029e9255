"""TPWL fit probe (csrc/tpwl_fit.hip) at the Diamond shape: n_x = 60, m = 4 (n = 65), the P = 64 points of the synthetic Diamond model
(workloads.diamond_c2), records of E episodes x T = 401 rows (stride 1: 400 samples per episode) for E in {64, 1024}.  Every row of the
records is a point of the table plus seeded noise, the point drawn per row (the content does not change the work).

Two sides, alternated in one process:
  (a) fit_tpwl from records resident on the device before the clock starts: assign, order, accumulate, reduce and solve on the device,
      the tables come back, the TPWLATV is built and the residuals are read from the sums (a clock between the steps gives the split
      add / solve / model and result);
  (b) what a user could do before, from the same records in host memory: TPWL.calc_nearest_point on the batch of samples (the states
      go up, the indices come back), then per point numpy.linalg.lstsq of g on [x - x_p, u, 1] with the columns scaled by their norms,
      on the granted threads.
Between the sides an untimed settle step (garbage collection, one small device allocation, a device wait).  The two sets of tables are
compared on the points both solve (the figure is reported).  Host clock around work that ends in a device wait or a host result;
warm-up runs first; median, min, max.  --kernel-stats <csv>: merges the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of
`--only-fit` (a run of its own) into the JSON.

    python tools/tpwl_fit_probe.py [--out profiles/tpwl_fit_probe.json] [--episodes 64,1024] [--only-fit] [--kernel-stats csv]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import contextlib
import csv
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

T, TS = 401, 0.01
KERNELS = ('tf_assign_kernel', 'tf_scan_kernel', 'tf_scatter_kernel', 'tf_accum_kernel', 'tf_reduce_kernel', 'tf_solve_kernel')
W = {'q': 1.0, 'v': 0.0}


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def plant():
    import workloads as wl
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    w = wl.diamond_c2()
    rom = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    tp = TPWLATV(data=dict(w['tab'], rom_info=rom), params=dict(tpwl_method='nn', dist_weights=dict(W)), discr_method='fe')
    return tp, np.asarray(w['tab']['q']), np.asarray(w['tab']['v']), np.asarray(w['tab']['u']), rom


def records(q, v, u, E, rng):
    """X (E, T, n_x), U (E, T, m): every row x_p + noise, u_p + noise with p drawn per row (the content does not change the work of
    either side, and every point receives samples)."""
    P, m = q.shape[0], u.shape[1]
    p = rng.integers(0, P, (E, T))
    X = np.concatenate([v[p], q[p]], axis=2) + 0.5 * rng.standard_normal((E, T, 2 * q.shape[1]))
    U = u[p] + 50.0 * rng.standard_normal((E, T, m))
    return np.ascontiguousarray(X), np.ascontiguousarray(U)


def side_a(dX, dU, E, q, v, rom):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import TPWLSysID
    t0 = time.perf_counter()
    sid = TPWLSysID(q, v, W, 4, TS)
    sid.add(dX, dU, shape=(E, T))
    _lib.sync()
    t1 = time.perf_counter()
    tab = sid.solve_tables(1e-9)
    t2 = time.perf_counter()
    model, kept = sid.model(tab, rom, on_fail='drop')
    res = sid.result(tab, 1e-9, kept)
    t3 = time.perf_counter()
    return t3 - t0, tab, res, (t1 - t0, t2 - t1, t3 - t2)


def settle():
    """Between the sides, outside every clock: what the last side left to the allocator and the driver is paid here."""
    import gc
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def side_b(tp, X, U, q, v):
    """calc_nearest_point on the batch, then per point lstsq on the host."""
    t0 = time.perf_counter()
    nx, m, P = X.shape[2], U.shape[2], q.shape[0]
    x0 = np.ascontiguousarray(X[:, :-1].reshape(-1, nx))
    g = ((X[:, 1:] - X[:, :-1]) / TS).reshape(-1, nx)
    u0 = U[:, :-1].reshape(-1, m)
    idx = tp.calc_nearest_point(x0)
    xp = np.hstack([v, q])
    A, B, d = np.zeros((P, nx, nx)), np.zeros((P, nx, m)), np.zeros((P, nx))
    solved = np.zeros(P, dtype=bool)
    for p in range(P):
        sel = idx == p
        if sel.sum() < nx + m + 2:
            continue
        Phi = np.hstack([x0[sel] - xp[p], u0[sel], np.ones((int(sel.sum()), 1))])
        s = np.sqrt(np.einsum('ij,ij->j', Phi, Phi))
        s[s == 0.0] = 1.0
        sol = (np.linalg.lstsq(Phi / s, g[sel], rcond=None)[0] / s[:, None]).T
        A[p], B[p], d[p] = sol[:, :nx], sol[:, nx:nx + m], sol[:, nx + m] - sol[:, :nx] @ xp[p]
        solved[p] = True
    return time.perf_counter() - t0, dict(A_c=A, B_c=B, d_c=d, solved=solved)


def kernel_split(path):
    """{kernel: total ns, calls} of the fit's kernels from a rocprofv3 kernel stats csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            for key in KERNELS:
                if key in name:
                    tot = float(row.get('TotalDurationNs') or row.get('TotalDuration') or 0)
                    calls = int(float(row.get('Calls') or row.get('Count') or 0))
                    prev = out.get(key, dict(total_ns=0.0, calls=0))
                    out[key] = dict(total_ns=prev['total_ns'] + tot, calls=prev['calls'] + calls)
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tpwl_fit_probe.json'))
    ap.add_argument('--episodes', default='64,1024')
    ap.add_argument('--only-fit', action='store_true', help='side (a) alone, a few runs: the run to trace')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        doc['kernel_split'] = kernel_split(args.kernel_stats)
        json.dump(doc, open(args.out, 'w'), indent=1)
        print(json.dumps(doc['kernel_split']))
        return
    from sofacontrol_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    with contextlib.redirect_stdout(io.StringIO()):
        tp, q, v, u, rom = plant()
    doc = dict(shape=dict(n_x=2 * q.shape[1], m=u.shape[1], n=2 * q.shape[1] + u.shape[1] + 1, P=q.shape[0], T=T, stride=1, ridge=1e-9),
               threads=os.environ.get('OMP_NUM_THREADS'), sizes={})
    for E in [int(s) for s in args.episodes.split(',')]:
        X, U = records(q, v, u, E, np.random.default_rng(E))
        dX, dU = _lib.DeviceBuffer.from_array(X), _lib.DeviceBuffer.from_array(U)
        warm, timed = (2, 7) if E <= 128 else (1, 3)
        if args.only_fit:
            for _ in range(3):
                side_a(dX, dU, E, q, v, rom)
                settle()
            continue
        ta, tb, phases = [], [], []
        for it in range(warm + timed):
            a, tab, res, ph = side_a(dX, dU, E, q, v, rom)
            settle()
            b, hb = side_b(tp, X, U, q, v)
            settle()
            if it >= warm:
                ta.append(a); tb.append(b); phases.append(ph)
        both = (tab['status'] == 0) & hb['solved']
        diff = {k: float(np.abs(tab[k][both] - hb[k][both]).max() / max(1.0, np.abs(hb[k][both]).max())) if both.any() else None
                for k in ('A_c', 'B_c', 'd_c')}
        sa, sb = stat(ta), stat(tb)
        doc['sizes'][str(E)] = dict(
            samples=res.samples, counts=dict(min=int(res.counts.min()), max=int(res.counts.max())),
            status=dict(solved=int((tab['status'] == 0).sum()), too_few_samples=int((tab['status'] == 1).sum()), failing_pivot=int((tab['status'] == 2).sum())),
            host_solved=int(hb['solved'].sum()), fit_seconds=sa,
            fit_phase_seconds=dict(zip(('add', 'solve', 'model_and_result'), (stat(x) for x in zip(*phases)))), host_seconds=sb,
            speedup_of_medians=sb['median'] / sa['median'], fit_median_within_host_spread=bool(sa['median'] <= sb['median'] + (sb['max'] - sb['min'])),
            largest_relative_difference_of_the_tables=diff)
        print('E = %d: %d samples, %d of %d points solved; fit %.2f ms (%.2f .. %.2f), host route %.1f ms (%.1f .. %.1f), tables differ by %s'
              % (E, res.samples, int((tab['status'] == 0).sum()), q.shape[0], 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'],
                 1e3 * sb['median'], 1e3 * sb['min'], 1e3 * sb['max'], diff))
    if not args.only_fit:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
