"""TPWL point-selection probe (csrc/tpwl_select.hip) at the Diamond size: r = 30 (n_x = 60), records of E episodes x T = 1001 rows resident
on the device, E in {256, 4096}.  The records are synthetic and smooth: per episode a three-dimensional latent motion a sin(2 pi f t / T +
phi) mapped to the 60 coordinates by one fixed matrix, plus seeded noise -- the point count then follows the threshold as it does on a
robot's records (few intrinsic dimensions), which changes the work: the count is reported with every time.

Thresholds: a geometric sweep on the device at the first size picks one threshold that yields a few tens of points and one that yields a
few hundred; the sweep is reported.

Two sides, alternated in one process:
  (a) points_by_distance on the device-resident records (one call: the finite check, two launches per chunk, one host wait);
  (b) the float64 numpy restatement of the reference's scan (tpwl_utils.py:171-196) on the host's granted threads: one distance row per
      candidate against the table taken so far.  At the large size side (b) scans only the first --host-episodes episodes (the scan of
      a prefix of the records is the prefix of the scan), and the device result is compared on that prefix; the JSON says so.
Between the sides an untimed settle step.  Host clock around work that ends in a device wait or a host result; warm-up first; median,
min, max.  The bytes across PCIe are those of the call's copies (computed, not measured).  --kernel-stats <csv> merges the per-kernel
times of a `rocprofv3 --kernel-trace --stats` run of `--only-select` (a run of its own) into the JSON.

    python tools/tpwl_select_probe.py [--out profiles/tpwl_select_probe.json] [--episodes 256,4096] [--only-select] [--kernel-stats csv]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import csv
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

R, T, LATENT = 30, 1001, 3
W = {'q': 1.0, 'v': 0.05}
KERNELS = ('ts_finite_kernel', 'ts_dmin_kernel', 'ts_scan_kernel')


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def records(E, seed=0):
    rng = np.random.default_rng(seed)
    M = np.random.default_rng(1234).standard_normal((LATENT, 2 * R)) / np.sqrt(LATENT)
    t = np.arange(T) / T
    X = np.empty((E, T, 2 * R))
    for e0 in range(0, E, 256):                                   # in blocks: the latent motion, the map, the noise
        n = min(256, E - e0)
        a, f, ph = rng.uniform(0.2, 1.0, (n, 1, LATENT)), rng.uniform(0.5, 2.0, (n, 1, LATENT)), rng.uniform(0, 2 * np.pi, (n, 1, LATENT))
        z = a * np.sin(2 * np.pi * f * t[None, :, None] + ph)
        X[e0:e0 + n] = z @ M + 0.01 * rng.standard_normal((n, T, 2 * R))
    return X


def settle():
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def side_a(dX, E, thr):
    from sofacontrol_amd.tpwl.sysid import points_by_distance
    t0 = time.perf_counter()
    sel = points_by_distance(dX, W, thr, shape=(E, T, 2 * R))
    return time.perf_counter() - t0, sel


def side_b(X, thr, max_points=1024):
    """tpwl_utils.py:171-196 on records: (seconds, index (P, 2), complete)."""
    t0 = time.perf_counter()
    E = X.shape[0]
    q, v, n, index, complete = np.zeros((max_points, R)), np.zeros((max_points, R)), 0, [], True
    for ep in range(E):
        for row in range(T):
            x = X[ep, row]
            if n:
                d = W['q'] * np.linalg.norm(x[R:] - q[:n], axis=1) + W['v'] * np.linalg.norm(x[:R] - v[:n], axis=1)
                if not np.min(d) >= thr:
                    continue
            if n == max_points:
                complete = False
                break
            q[n], v[n] = x[R:], x[:R]
            n += 1
            index.append((ep, row))
        if not complete:
            break
    return time.perf_counter() - t0, np.array(index, dtype=np.int64).reshape(-1, 2), complete


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tpwl_select_probe.json'))
    ap.add_argument('--episodes', default='256,4096')
    ap.add_argument('--host-episodes', type=int, default=256)
    ap.add_argument('--only-select', action='store_true', help='side (a) alone, a few runs at fixed thresholds: the run to trace')
    ap.add_argument('--thresholds', default=None, help='two thresholds (few tens, few hundred points) instead of the sweep')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        doc['kernel_split'] = dict(kernel_split(args.kernel_stats), source='rocprofv3 --kernel-trace --stats of --only-select, a run of its own')
        json.dump(doc, open(args.out, 'w'), indent=1)
        print(json.dumps(doc['kernel_split']))
        return
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    assert _lib.device_count() >= 1, 'no GPU visible'
    sizes = [int(s) for s in args.episodes.split(',')]
    doc = dict(shape=dict(r=R, n_x=2 * R, T=T, stride=1, dist_weights=W, max_points=1024, latent_dimensions=LATENT),
               threads=os.environ.get('OMP_NUM_THREADS'), sizes={},
               not_measured=['records of a real robot (the records are synthetic)', 'host records (the upload of the records is outside every clock)',
                             'separate=True', 'stride > 1', 'the bytes across PCIe are computed from the copies of a call, not counted',
                             'the host side at the large size beyond its first episodes'])
    thr = [float(s) for s in args.thresholds.split(',')] if args.thresholds else None
    for E in sizes:
        X = records(E, seed=E)
        dX = _lib.DeviceBuffer.from_array(X)
        plan = sysid.select_plan(R, E * T)
        if thr is None:                                            # the sweep, on the device
            scale = float(np.linalg.norm(X[0, :, R:].max(axis=0) - X[0, :, R:].min(axis=0)))
            sweep, thr = [], [None, None]
            for k in range(28):
                th = scale * 0.85 ** k
                _, sel = side_a(dX, E, th)
                sweep.append(dict(threshold=th, points=len(sel.q), complete=bool(sel.complete)))
                if thr[0] is None and 20 <= len(sel.q) < 100:
                    thr[0] = th
                if thr[1] is None and 200 <= len(sel.q) < 1000 and sel.complete:
                    thr[1] = th
                if not sel.complete:
                    break
            doc['sweep'] = dict(episodes=E, scale=scale, steps=sweep)
            print('sweep at E = %d: %s' % (E, [(round(s['threshold'], 4), s['points']) for s in sweep]))
            assert thr[0] is not None and thr[1] is not None, 'the sweep found no threshold for a few tens / a few hundred points'
        if args.only_select:
            for th in thr:
                for _ in range(3):
                    side_a(dX, E, th)
                    settle()
            dX.free()
            continue
        Eh = min(E, args.host_episodes)
        entry = dict(candidates=E * T, chunk=plan['chunk'], launches=plan['launches'], host_episodes=Eh, thresholds={})
        for th in thr:
            warm, timed = (1, 5) if E <= 512 else (1, 3)
            ta, tb = [], []
            for it in range(warm + timed):
                a, sel = side_a(dX, E, th)
                settle()
                if it < 3:                                         # the host side: a few runs (it takes seconds to minutes)
                    b, hidx, hcomplete = side_b(X[:Eh], th)
                    settle()
                    tb.append(b)
                if it >= warm:
                    ta.append(a)
            on_prefix = sel.index[sel.index[:, 0] < Eh]
            same = bool(np.array_equal(on_prefix, hidx)) if (hcomplete and (sel.complete or Eh == E)) else None
            sa, sb = stat(ta), stat(tb)
            pcie = dict(host_to_device=24, device_to_host=24 + 1024 * (8 + 2 * R * 8 + 16))
            entry['thresholds']['%.6g' % th] = dict(
                points=len(sel.q), complete=bool(sel.complete), select_seconds=sa, host_seconds=sb, host_candidates=Eh * T,
                host_points=int(len(hidx)), host_seconds_per_candidate=sb['median'] / (Eh * T),
                select_seconds_per_candidate=sa['median'] / (E * T), index_equal_on_the_host_prefix=same, pcie_bytes_per_call=pcie)
            print('E = %d, threshold %.4g: %d points (complete %s); device %.2f ms (%.2f .. %.2f) for %d candidates; host scan of %d '
                  'candidates %.2f s (%.2f .. %.2f), %d points; index equal on the prefix: %s'
                  % (E, th, len(sel.q), sel.complete, 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'], E * T, Eh * T, sb['median'],
                     sb['min'], sb['max'], len(hidx), same))
        doc['sizes'][str(E)] = entry
        dX.free()
    if not args.only_select:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
