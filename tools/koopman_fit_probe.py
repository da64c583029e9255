"""Koopman fit probe (csrc/koopman_fit.hip) at the Diamond shape: n_y = 3, m = 4, one delay, degree 2 (P = 66 observables with the
constant, n = 70), records of E episodes x T = 1001 samples (stride 1: 999 pairs per episode) for E in {256, 4096}, iid uniform in [-1, 1]
(the content does not change the work), resident on the device before the clock starts.

Two sides, alternated in one process:
  (a) fit_koopman's steps from the device-resident records: min/max, accumulate, reduce and solve on the device; A, B and the sums come
      back (a clock between the steps gives the split add / solve / sums);
  (b) what the library offered before for the same arithmetic: KoopmanLift.embed_lift_dev per episode on the device (psi of every row),
      one copy of psi and of u back, then Phi^T Phi, Psi1^T Phi in numpy and scipy.linalg.cho_factor / cho_solve on the granted threads.
      The scaling of (b) is given (the min/max of (a) has no counterpart there).  (b) runs twice (b, b2): the difference of the two medians
      is the spread of the host figure.
Between the sides an untimed settle step (garbage collection, one small device allocation, a device wait) keeps what one side leaves
to the allocator and the driver out of the other's clock; (b) releases its host arrays inside its own clock.  The two models are
compared (the figure is reported).  Host clock around work that ends in a device wait or a host result; warm-up runs first; median,
min, max.  Bytes across PCIe are computed from the shapes.  The flop count of the accumulate kernel is that of the MFMA
instructions it issues (tiles x k steps x 2048), for the share of the f64 MFMA rate (73 TFLOP/s sustained).
--kernel-stats <csv>: merges the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of `--only-fit` (a run of its own) into
the JSON.

    python tools/koopman_fit_probe.py [--out profiles/koopman_fit_probe.json] [--episodes 256,4096] [--only-fit] [--kernel-stats csv]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

NY, M, D, DEG, T, TS = 3, 4, 1, 2, 1001, 0.05
P, N = 66, 70
MFMA_F64_TFLOPS = 73.0


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def accumulate_flop(E):
    """MFMA flop the accumulate kernel issues: per chunk ceil(pairs / 4) k steps of every tile (15 of G, 25 of R at n = 70)."""
    from sofacontrol_amd.baselines.koopman.sysid import fit_plan
    TR = fit_plan(NY * (D + 1) + M * D, DEG, False, M)['rows_per_chunk']
    ppe = T - 1 - D
    T16, PT = (N + 15) // 16, (P + 15) // 16
    ntile = T16 * (T16 + 1) // 2 + PT * T16
    ksteps = sum((min(TR, ppe - c * TR) + 3) // 4 for c in range((ppe + TR - 1) // TR))
    useful = 2.0 * E * ppe * (N * (N + 1) / 2 + P * N)
    return 2048.0 * ntile * ksteps * E, useful


def side_a(dy, du, E):
    """fit_koopman's own steps with a clock between them: (seconds, model, result, (add, solve, sums and model) seconds).  `add` holds
    the min/max, the creation of the lift and fit handles, accumulate and reduce, and ends in a device wait."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.baselines.koopman.sysid import KoopmanSysID, KoopmanFitResult, residual_rms
    t0 = time.perf_counter()
    sid = KoopmanSysID(NY, M, TS, obs_degree=DEG, delays=D)
    sid.add(dy, du, shape=(E, T))
    _lib.sync()
    t1 = time.perf_counter()
    A, B = sid.solve_AB(0.0)
    t2 = time.perf_counter()
    res = KoopmanFitResult(sid.pairs, 0.0, residual_rms(sid.sums(), A, B))
    model = sid._model(A, B)
    t3 = time.perf_counter()
    return t3 - t0, model, res, (t1 - t0, t2 - t1, t3 - t2)


def settle():
    """Between the sides, outside every clock: what the last side left to the allocator and the driver is paid here."""
    import gc
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def side_b(lift, dy, du, dpsi, E, scale):
    """embed_lift on the device per episode, the copy back, the normal equations and the Cholesky solve on the host."""
    import scipy.linalg
    from sofacontrol_amd import _lib
    t0 = time.perf_counter()
    rows = T - D
    for e in range(E):
        lift.embed_lift_dev(C.c_void_p(dy.ptr.value + 8 * e * T * NY), C.c_void_p(du.ptr.value + 8 * e * T * M), T,
                            C.c_void_p(dpsi.ptr.value + 8 * e * rows * P))
    _lib.sync()
    psi = dpsi.to_array((E, rows, P))
    u = du.to_array((E, T, M))
    v = (u[:, D:T - 1] - scale['u_offset']) / scale['u_factor']
    G, R = np.zeros((N, N)), np.zeros((P, N))
    for e0 in range(0, E, 64):                                   # blocks of episodes: the host never holds Phi of the whole record
        Phi = np.concatenate([psi[e0:e0 + 64, :-1], v[e0:e0 + 64]], axis=2).reshape(-1, N)
        G += Phi.T @ Phi
        R += psi[e0:e0 + 64, 1:].reshape(-1, P).T @ Phi
    X = scipy.linalg.cho_solve(scipy.linalg.cho_factor(G), R.T).T
    del psi, u, v, Phi                                           # the side's own 2 GB of host arrays are released inside its clock
    return time.perf_counter() - t0, X


def kernel_split(path):
    """{kernel: total ns, calls} of the fit's kernels from a rocprofv3 kernel stats csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            for key in ('kf_accum_kernel', 'kf_reduce_kernel', 'kf_solve_kernel', 'kf_minmax_kernel', 'kf_minmax_final_kernel'):
                if key + '<' in name or key + '(' in name or name.endswith(key) or key + 'E' in name or key + 'I' in name:
                    tot = float(row.get('TotalDurationNs') or row.get('TotalDuration') or 0)
                    calls = int(float(row.get('Calls') or row.get('Count') or 0))
                    prev = out.get(key, dict(total_ns=0.0, calls=0))
                    out[key] = dict(total_ns=prev['total_ns'] + tot, calls=prev['calls'] + calls)
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'koopman_fit_probe.json'))
    ap.add_argument('--episodes', default='256,4096')
    ap.add_argument('--only-fit', action='store_true', help='side (a) alone, a few runs: the run to trace')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    from sofacontrol_amd import _lib
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanLift
    assert _lib.device_count() >= 1, 'no GPU visible'
    if args.kernel_stats:
        doc = json.load(open(args.out))
        doc['kernel_split'] = kernel_split(args.kernel_stats)
        json.dump(doc, open(args.out, 'w'), indent=1)
        print(json.dumps(doc['kernel_split']))
        return
    doc = dict(shape=dict(n_y=NY, m=M, delays=D, degree=DEG, n_psi=P, n=N, T=T, stride=1), threads=os.environ.get('OMP_NUM_THREADS'), sizes={})
    for E in [int(s) for s in args.episodes.split(',')]:
        rng = np.random.default_rng(E)
        Y, U = rng.uniform(-1.0, 1.0, (E, T, NY)), rng.uniform(-1.0, 1.0, (E, T, M))
        dy, du = _lib.DeviceBuffer.from_array(Y), _lib.DeviceBuffer.from_array(U)
        warm, timed = (2, 7) if E <= 512 else (1, 5)
        if args.only_fit:
            for _ in range(3):
                side_a(dy, du, E)
                settle()
            continue
        dpsi = _lib.DeviceBuffer(8 * E * (T - D) * P)
        _, model, res, _ = side_a(dy, du, E)
        scale = {k: np.ravel(v) for k, v in model.scale.items()}
        lift = KoopmanLift(NY, M, D, DEG, DMD=False, **scale)
        ta, tb, tb2, phases = [], [], [], []
        for it in range(warm + timed):
            a, model, res, ph = side_a(dy, du, E)
            settle()
            b, X = side_b(lift, dy, du, dpsi, E, scale)
            settle()
            b2, _ = side_b(lift, dy, du, dpsi, E, scale)
            settle()
            if it >= warm:
                ta.append(a); tb.append(b); tb2.append(b2); phases.append(ph)
        diff = float(np.abs(np.hstack([model.A_d, model.B_d]) - X).max())
        flop, useful = accumulate_flop(E)
        sa, sb, sb2 = stat(ta), stat(tb), stat(tb2)
        doc['sizes'][str(E)] = dict(
            pairs=res.pairs, residual_rms=res.residual_rms, fit_seconds=sa,
            fit_phase_seconds=dict(zip(('add', 'solve', 'sums_and_model'), (stat(v) for v in zip(*phases)))), host_seconds=sb, host_seconds_second_run=sb2,
            host_spread_seconds=abs(sb['median'] - sb2['median']), speedup_of_medians=sb['median'] / sa['median'],
            largest_difference_of_the_models=diff,
            pcie_bytes=dict(fit=dict(d2h=8 * (P * P + P * M + N * N + P * N + 1 + 2 * (NY + M)), h2d=0),
                            host=dict(d2h=8 * (E * (T - D) * P + E * T * M), h2d=0)),
            accumulate_mfma_flop=flop, accumulate_useful_flop=useful)
        print('E = %d: %d pairs; fit %.2f ms (%.2f .. %.2f), host side %.1f ms (%.1f .. %.1f; second run %.1f), models differ by %.2e'
              % (E, res.pairs, 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'], 1e3 * sb['median'], 1e3 * sb['min'], 1e3 * sb['max'],
                 1e3 * sb2['median'], diff))
        del dpsi
    if not args.only_fit:
        doc['mfma_f64_tflops_reference'] = MFMA_F64_TFLOPS
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
