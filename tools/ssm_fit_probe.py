"""SSM fit probe (csrc/ssm_fit.hip) at the shipped shape: n_x = n_y = 6, m = 4, cubic (83 monomials, n = 87), records of E episodes x
T = 1001 samples (stride 1: 999 samples per episode) for E in {256, 4096}, iid uniform in [-1, 1] (the content does not change the
work), V a fixed orthogonal matrix.

Two sides, alternated in one process:
  (a) SSMSysID's steps from records resident on the device before the clock starts: accumulate, reduce and the two solves on the
      device; the coefficients and the sums come back (a clock between the steps gives the split add / solve / sums and dictionaries);
  (b) the host route the library offered before for the same arithmetic, from the same records in host memory: sssm_reduce per episode
      (x = V^T (y - y_ref) through the model handle: y goes up, x comes back), then the monomials by the parent recurrence, the columns
      scaled by their norms, and numpy.linalg.lstsq for the three fits, on the granted threads.
Between the sides an untimed settle step (garbage collection, one small device allocation, a device wait).  The two sets of
coefficients are compared (the figure is reported).  Host clock around work that ends in a device wait or a host result; warm-up runs
first; median, min, max.  Bytes across PCIe are computed from the shapes.  The flop count of the accumulate kernel is that of the
MFMA instructions it issues (tiles x k steps x 2048), for the share of the f64 MFMA rate (73 TFLOP/s sustained).
--kernel-stats <csv>: merges the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of `--only-fit` (a run of its own) into
the JSON.

    python tools/ssm_fit_probe.py [--out profiles/ssm_fit_probe.json] [--episodes 256,4096] [--only-fit] [--kernel-stats csv]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

NX, NY, M, RO, SO, T, TS = 6, 6, 4, 3, 3, 1001, 0.01
NMON, N = 83, 87
MFMA_F64_TFLOPS = 73.0
KERNELS = ('sf_accum_kernel', 'sf_reduce_kernel', 'sf_solve_kernel', 'sf_cov_kernel')


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def accumulate_flop(E):
    """MFMA flop the accumulate kernel issues: per chunk ceil(samples / 4) k steps of every tile (21 of G, 12 of the stacked R at
    n = 87, 2 n_x + n_y = 18), and the flop of the sums themselves."""
    from sofacontrol_amd.SSM.sysid import fit_plan
    TR = fit_plan(NX, NY, M, RO, SO)['rows_per_chunk']
    spe = T - 2
    T16, TT = (N + 15) // 16, (2 * NX + NY + 15) // 16
    ntile = T16 * (T16 + 1) // 2 + TT * T16
    ksteps = sum((min(TR, spe - c * TR) + 3) // 4 for c in range((spe + TR - 1) // TR))
    useful = 2.0 * E * spe * (N * (N + 1) / 2 + 2 * NX * N + NY * NMON)
    return 2048.0 * ntile * ksteps * E, useful


def side_a(dy, du, E, V):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.SSM.sysid import SSMSysID
    t0 = time.perf_counter()
    sid = SSMSysID(NY, M, TS, NX, RO, SO, V=V)
    sid.add(dy, du, shape=(E, T))
    _lib.sync()
    t1 = time.perf_counter()
    co = sid.solve_coeffs(0.0)
    t2 = time.perf_counter()
    model, params = sid.dictionaries(co)
    res = sid.result(co, 0.0)
    t3 = time.perf_counter()
    return t3 - t0, co, res, (t1 - t0, t2 - t1, t3 - t2)


def settle():
    """Between the sides, outside every clock: what the last side left to the allocator and the driver is paid here."""
    import gc
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def side_b(ssm, Y, U, E, tables):
    """sssm_reduce per episode, the monomials, the scaled columns and lstsq on the host."""
    par, var = tables
    t0 = time.perf_counter()
    X = np.empty((E, T, NX))
    for e in range(E):
        X[e] = ssm.compute_RO_state(Y[e])
    xi = X[:, 1:-1].reshape(-1, NX)
    Phi = np.empty((xi.shape[0], N))
    for k in range(NMON):
        Phi[:, k] = xi[:, var[k]] if par[k] < 0 else Phi[:, par[k]] * xi[:, var[k]]
    Phi[:, NMON:] = U[:, 1:-1].reshape(-1, M)
    d = 1.0 / np.sqrt(np.einsum('ij,ij->j', Phi, Phi))
    Phi *= d
    rhs = np.hstack([X[:, 2:].reshape(-1, NX), ((X[:, 2:] - X[:, :-2]) / (2 * TS)).reshape(-1, NX), Y[:, 1:-1].reshape(-1, NY)])
    sol = np.linalg.lstsq(Phi, rhs, rcond=None)[0] * d[:, None]
    co = dict(rd_coeff=sol[:NMON, :NX].T, Bd=sol[NMON:, :NX].T, r_coeff=sol[:NMON, NX:2 * NX].T, B=sol[NMON:, NX:2 * NX].T,
              w_coeff=np.linalg.lstsq(Phi[:, :NMON], rhs[:, 2 * NX:], rcond=None)[0].T * d[None, :NMON])
    del X, xi, Phi, rhs
    return time.perf_counter() - t0, co


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


def host_model(V):
    """An SSMDynamics whose v_coeff is [V^T | 0] (the other coefficients are not used by sssm_reduce), and the basis tables."""
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    from sofacontrol_amd.SSM.sysid import SSMSysID, exponents
    sid = SSMSysID(NY, M, TS, NX, RO, SO, V=V)
    zero = dict(rd_coeff=np.zeros((NX, NMON)), Bd=np.zeros((NX, M)), r_coeff=np.zeros((NX, NMON)), B=np.zeros((NX, M)), w_coeff=np.zeros((NY, NMON)))
    model, params = sid.dictionaries(zero)
    Ex = exponents(NX, max(RO, SO))
    index = {tuple(e): k for k, e in enumerate(Ex)}
    par, var = [], []
    for e in Ex:
        last = int(np.flatnonzero(e)[-1])
        p = e.copy(); p[last] -= 1
        var.append(last); par.append(index[tuple(p)] if p.any() else -1)
    return SSMDynamics(np.zeros(NY), model=model, params=params), (par, var)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssm_fit_probe.json'))
    ap.add_argument('--episodes', default='256,4096')
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
    V, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((NY, NX)))
    V = np.ascontiguousarray(V)
    doc = dict(shape=dict(n_x=NX, n_y=NY, m=M, ROM_order=RO, SSM_order=SO, n_mon=NMON, n=N, T=T, stride=1),
               threads=os.environ.get('OMP_NUM_THREADS'), sizes={})
    for E in [int(s) for s in args.episodes.split(',')]:
        rng = np.random.default_rng(E)
        Y, U = rng.uniform(-1.0, 1.0, (E, T, NY)), rng.uniform(-1.0, 1.0, (E, T, M))
        dy, du = _lib.DeviceBuffer.from_array(Y), _lib.DeviceBuffer.from_array(U)
        warm, timed = (2, 7) if E <= 512 else (1, 3)
        if args.only_fit:
            for _ in range(3):
                side_a(dy, du, E, V)
                settle()
            continue
        ssm, tables = host_model(V)
        ta, tb, phases = [], [], []
        for it in range(warm + timed):
            a, co, res, ph = side_a(dy, du, E, V)
            settle()
            b, cb = side_b(ssm, Y, U, E, tables)
            settle()
            if it >= warm:
                ta.append(a); tb.append(b); phases.append(ph)
        diff = {k: float(np.abs(co[k] - cb[k]).max() / max(1.0, np.abs(cb[k]).max())) for k in co}
        flop, useful = accumulate_flop(E)
        sa, sb = stat(ta), stat(tb)
        nd = NMON + M
        doc['sizes'][str(E)] = dict(
            samples=res.samples, residual_rms=dict(d=res.residual_rms_d, c=res.residual_rms_c, w=res.residual_rms_w), fit_seconds=sa,
            fit_phase_seconds=dict(zip(('add', 'solve', 'sums_and_dictionaries'), (stat(v) for v in zip(*phases)))), host_seconds=sb,
            speedup_of_medians=sb['median'] / sa['median'], largest_relative_difference_of_the_coefficients=diff,
            pcie_bytes=dict(fit=dict(d2h=8 * (2 * NX * nd + NY * NMON + N * N + 2 * NX * N + NY * NMON + 3) + 8, h2d=8 * (NY * NX + NY) + 4 * (nd + NMON)),
                            host=dict(d2h=8 * E * T * NX, h2d=8 * E * T * NY)),
            accumulate_mfma_flop=flop, accumulate_useful_flop=useful)
        print('E = %d: %d samples; fit %.2f ms (%.2f .. %.2f), host route %.1f ms (%.1f .. %.1f), coefficients differ by %s'
              % (E, res.samples, 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'], 1e3 * sb['median'], 1e3 * sb['min'], 1e3 * sb['max'], diff))
    if not args.only_fit:
        doc['mfma_f64_tflops_reference'] = MFMA_F64_TFLOPS
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
