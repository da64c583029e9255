"""TPWL horizon-error probe (csrc/tpwl_horizon.hip) at the Diamond shape: n_x = 60, m = 4, P = 64, records of E episodes x T = 1001 rows
resident on the device, H = 50, every = 10, E in {256, 4096}.  The model is the synthetic Diamond plant of workloads.diamond_c2() at
dt = 0.01 (zoh); the records are its own open-loop episodes under seeded random held inputs plus a seeded measurement noise, so the
k-step error is small and not zero.  The work does not depend on which model is judged.

Two sides, alternated in one process:
  (a) horizon_error on the device-resident records (two launches, one host wait; 4 (H + 1) doubles and a few counts come back);
  (b) the host route a user has today: the same windows gathered on the host (x0 (W, n_x), U (W, H, m)), TPWL.rollout (stpwl_rollout:
      upload, one workgroup per window, X and Z downloaded) in chunks of --chunk windows, the errors and their norms in numpy on the
      host's granted threads.  Run at the sizes of --host-episodes.
The curves of the two routes are compared to twice the bound (n_x W + 3) 2^-53 sse of tests/tpwl_horizon_reference.py (each side
lies within it of the exact sums of the same predictions: the predictions are the same bits).
Between the sides an untimed settle step.  Host clock around work that ends in a device wait or a host result; warm-up first; median,
min, max.  The bytes across PCIe are those of the calls' copies (computed, not measured).  --kernel-stats <csv> merges the per-kernel
times of a `rocprofv3 --kernel-trace --stats` run of `--only-unit` (a run of its own) into the JSON.

    python tools/tpwl_horizon_probe.py [--out profiles/tpwl_horizon_probe.json] [--episodes 256,4096] [--host-episodes 256] [--only-unit]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import contextlib
import csv
import gc
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

T, H, EVERY, DT, HOLD, U_HI = 1001, 50, 10, 0.01, 5, 1500.0
KERNELS = ('th_window_kernel', 'th_join_kernel')
EPS = 2.0 ** -53


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def settle():
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def plant():
    import workloads as wl
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    w = wl.diamond_c2()
    Hf = linearModel(nodes=[1354], num_nodes=w['U'].shape[0] // 3).C.tocsr()
    rom_info = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    tp = TPWLATV(data=dict(w['tab'], rom_info=rom_info), params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(DT)
    return tp


def records(tp, E, seed):
    """(X (E, T, n_x), U (E, T, m)): open-loop episodes of the plant in blocks of 256, inputs held for five steps, noise 1e-3 on the states."""
    rng = np.random.default_rng(seed)
    n, m = tp.get_state_dim(), tp.get_input_dim()
    X, U = np.empty((E, T, n)), np.empty((E, T, m))
    for e0 in range(0, E, 256):
        k = min(256, E - e0)
        held = rng.uniform(0.0, U_HI, (k, (T - 1) // HOLD, m))
        u = np.repeat(held, HOLD, axis=1)
        x, _ = tp.rollout(0.5 * rng.standard_normal((k, n)), u, DT)
        X[e0:e0 + k] = x + 1e-3 * rng.standard_normal(x.shape)
        U[e0:e0 + k] = np.concatenate([u, u[:, -1:]], axis=1)
    assert np.isfinite(X).all()
    return X, U


def side_a(tp, dX, dU, E):
    from sofacontrol_amd.tpwl.sysid import horizon_error
    t0 = time.perf_counter()
    res = horizon_error(tp, dX, dU, H, dt=DT, every=EVERY, shape=(E, T))
    return time.perf_counter() - t0, res


def side_b(tp, X, U, chunk):
    """The host route: (seconds, sse_x (H + 1), sse_z (H + 1), bytes across PCIe)."""
    t0 = time.perf_counter()
    E = X.shape[0]
    j0 = np.arange(0, T - H, EVERY)
    rows = j0[:, None] + np.arange(H + 1)[None]
    sse_x, sse_z, h2d, d2h = np.zeros(H + 1), np.zeros(H + 1), 0, 0
    per = max(1, chunk // len(j0))                               # whole episodes per chunk
    for e0 in range(0, E, per):
        Xw = X[e0:e0 + per][:, rows].reshape(-1, H + 1, X.shape[2])
        Uw = U[e0:e0 + per][:, rows[:, :H]].reshape(-1, H, U.shape[2])
        xp, zp = tp.rollout(np.ascontiguousarray(Xw[:, 0]), np.ascontiguousarray(Uw), DT)
        e = xp - Xw
        ez = e @ tp.H.T
        sse_x += np.einsum('wkj,wkj->k', e, e)
        sse_z += np.einsum('wkj,wkj->k', ez, ez)
        h2d += Xw[:, 0].nbytes + Uw.nbytes
        d2h += xp.nbytes + zp.nbytes
    return time.perf_counter() - t0, sse_x, sse_z, dict(host_to_device=int(h2d), device_to_host=int(d2h))


def kernel_split(path):
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tpwl_horizon_probe.json'))
    ap.add_argument('--episodes', default='256,4096')
    ap.add_argument('--host-episodes', default='256', help='the sizes at which the host route runs too')
    ap.add_argument('--chunk', type=int, default=8192, help='windows of a chunk of the host route')
    ap.add_argument('--only-unit', action='store_true', help='side (a) alone, a few runs: the run to trace')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        doc['kernel_split'] = dict(kernel_split(args.kernel_stats), source='rocprofv3 --kernel-trace --stats of --only-unit, a run of its own')
        json.dump(doc, open(args.out, 'w'), indent=1)
        print(json.dumps(doc['kernel_split']))
        return
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    assert _lib.device_count() >= 1, 'no GPU visible'
    tp = plant()
    n, m, nz = tp.get_state_dim(), tp.get_input_dim(), tp.get_output_dim()
    sizes = [int(s) for s in args.episodes.split(',')]
    host_sizes = [int(s) for s in args.host_episodes.split(',') if s]
    doc = dict(shape=dict(n_x=n, m=m, P=tp.num_points, n_z=nz, T=T, H=H, every=EVERY, stride=1, dt=DT), threads=os.environ.get('OMP_NUM_THREADS'),
               host_chunk_windows=args.chunk, sizes={},
               not_measured=['other shapes (n_x, P, H, stride)', 'every = 1', 'host records on side (a) (the upload of the records is outside every clock)',
                             'hardware counters', 'records of a real robot (the records are the synthetic plant\'s)',
                             'the bytes across PCIe are computed from the copies of a call, not counted',
                             'the host route at the sizes not listed in host_episodes'])
    for E in sizes:
        X, U = records(tp, E, seed=E)
        dX, dU = _lib.DeviceBuffer.from_array(X), _lib.DeviceBuffer.from_array(U)
        plan = sysid.horizon_plan(tp, E, T, H, every=EVERY)
        if args.only_unit:
            for _ in range(3):
                side_a(tp, dX, dU, E)
                settle()
            dX.free(); dU.free()
            continue
        host = E in host_sizes
        warm, timed = (1, 7) if E <= 512 else (1, 5)
        ta, tb, hb = [], [], None
        for it in range(warm + timed):
            a, res = side_a(tp, dX, dU, E)
            settle()
            if host and it < warm + 3:                            # the host route takes seconds: a few runs
                b, hx, hz, pcie_b = side_b(tp, X, U, args.chunk)
                settle()
                if it >= warm:
                    tb.append(b)
                hb = (hx, hz)
            if it >= warm:
                ta.append(a)
        W = res.windows
        sa = stat(ta)
        entry = dict(windows=W, diverged=res.diverged, bad_rows=res.bad_rows, plan=plan, unit_seconds=sa, unit_seconds_per_window_step=sa['median'] / (W * H),
                     rms_x=[float(res.rms_x[k]) for k in (1, H // 2, H)], rms_z=[float(res.rms_z[k]) for k in (1, H // 2, H)],
                     pcie_bytes_unit=dict(host_to_device=0, device_to_host=8 * 4 * (H + 1) + 8 * 2 * (H + 1) + 16))
        line = 'E = %d: %d windows, plan %r; unit %.2f ms (%.2f .. %.2f)' % (E, W, plan, 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'])
        if host:
            sb = stat(tb)
            bx = 2 * (n * W + 3) * EPS * res.sse_x
            dx, dz = np.abs(res.sse_x - hb[0]), np.abs(res.sse_z - hb[1])
            entry.update(host_seconds=sb, pcie_bytes_host=pcie_b, sse_x_within_twice_the_bound=bool((dx <= bx).all()),
                         sse_x_largest_share=float(np.max(dx[1:] / bx[1:])), sse_z_largest_relative_difference=float(np.max(dz[1:] / res.sse_z[1:])))
            line += '; host route %.2f s (%.2f .. %.2f), %d bytes up, %d down; sse_x within twice the bound: %s (share %.3f), sse_z rel. diff %.2e' % (
                sb['median'], sb['min'], sb['max'], pcie_b['host_to_device'], pcie_b['device_to_host'], entry['sse_x_within_twice_the_bound'],
                entry['sse_x_largest_share'], entry['sse_z_largest_relative_difference'])
        print(line)
        doc['sizes'][str(E)] = entry
        dX.free(); dU.free()
        del X, U
    if not args.only_unit:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
