"""SSM horizon-error probe (csrc/ssm_horizon.hip) at the shipped Diamond shape: n_x = n_y = 6, m = 4, cubic (the reference's SSM_model.mat
as golden g17 holds it), records of E episodes x T = 1001 rows resident on the device, H = 20, every = 10, E in {256, 4096}, modes `be`
and the discrete map.  The records are the model's own open-loop episodes under the reference's recorded inputs (g17 u_interp, shifted
and scaled per episode) plus a seeded measurement noise, so the k-step error is small and not zero.  The work does not depend on
which model is judged.

Two sides, alternated in one process:
  (a) horizon_error on the device-resident records (three launches, one host wait; 4 (H + 1) doubles and a few counts come back);
  (b) the host route a user has today, all of it code that existed before the unit: the observed states of every kept row by
      compute_RO_state (W_map(y - z_ref)), the windows gathered on the host, SSM.rollout (upload, one workgroup per window, X and Z
      downloaded; Z is already C_map(x) + z_ref, so x_to_zfyf is not called again) in chunks of --chunk windows, the errors and their
      norms in numpy on the host's granted threads.  Run at the sizes of --host-episodes.
The two routes do not give the same bits (SSM.rollout's kernel sums in another order than the staged evaluator): the curves are
compared by their largest relative difference.
Between the sides an untimed settle step.  Host clock around work that ends in a device wait or a host result; warm-up first; median,
min, max.  The bytes across PCIe are those of the calls' copies (computed, not measured).  --kernel-stats <csv> merges the per-kernel
times of a `rocprofv3 --kernel-trace --stats` run of `--only-unit` (a run of its own) into the JSON.

    python tools/ssm_horizon_probe.py [--out profiles/ssm_horizon_probe.json] [--episodes 256,4096] [--host-episodes 256] [--only-unit]

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

T, H, EVERY, NOISE = 1001, 20, 10, 1e-3
KERNELS = ('sh_observe_kernel', 'sh_window_kernel', 'sh_join_kernel')
MODES = ('be', 'map')


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def settle():
    from sofacontrol_amd import _lib
    gc.collect()
    _lib.DeviceBuffer(4096).free()
    _lib.sync()


def _mat(v):
    a = np.empty((1, 1), dtype=object)
    a[0, 0] = np.asarray(v)
    return a


def shipped(mode):
    """(the shipped model in a mode, the golden's arrays)."""
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g17_ssm_hardware.npz'))
    mdl = {k[len('model_'):]: _mat(g[k]) for k in g.files if k.startswith('model_')}
    prm = {k[len('params_'):]: _mat(g[k]) for k in g.files if k.startswith('params_')}
    kw = dict(discrete=True, discr_method='be') if mode == 'map' else dict(discrete=False, discr_method=mode)
    return SSMDynamics(g['z_eq'].copy(), model=mdl, params=prm, **kw), g


def records(gen, g, E, seed):
    """(Y (E, T, 6), U (E, T, 4)): open-loop episodes of the model's discrete map in blocks of 256 under the recorded inputs, rolled by 7 rows
    and scaled by 0.5 .. 1 per episode, noise 1e-3 on the outputs."""
    rng = np.random.default_rng(seed)
    u0 = np.asarray(g['u_interp'], dtype=np.float64)[:T]
    Y, U = np.empty((E, T, 6)), np.empty((E, T, 4))
    for e0 in range(0, E, 256):
        k = min(256, E - e0)
        u = np.stack([rng.uniform(0.5, 1.0) * np.roll(u0, 7 * (e0 + i), axis=0) for i in range(k)])
        _, z = gen.rollout(np.zeros((k, 6)), np.ascontiguousarray(u[:, :T - 1]), float(g['dt']))
        Y[e0:e0 + k] = z + NOISE * rng.standard_normal(z.shape)
        U[e0:e0 + k] = u
    assert np.isfinite(Y).all()
    return Y, U


def side_a(model, dY, dU, E, dt):
    from sofacontrol_amd.SSM.sysid import horizon_error
    t0 = time.perf_counter()
    res = horizon_error(model, dY, dU, H, dt=dt, every=EVERY, shape=(E, T))
    return time.perf_counter() - t0, res


def side_b(model, Y, U, chunk, dt):
    """The host route: (seconds, sse_x (H + 1), sse_z (H + 1), bytes across PCIe)."""
    t0 = time.perf_counter()
    E, n = Y.shape[0], Y.shape[2]
    Xo = model.compute_RO_state(Y.reshape(-1, n)).reshape(E, T, n)
    h2d, d2h = Y.nbytes, Xo.nbytes
    j0 = np.arange(0, T - H, EVERY)
    rows = j0[:, None] + np.arange(H + 1)[None]
    sse_x, sse_z = np.zeros(H + 1), np.zeros(H + 1)
    per = max(1, chunk // len(j0))                               # whole episodes per chunk
    for e0 in range(0, E, per):
        Yw = Y[e0:e0 + per][:, rows].reshape(-1, H + 1, n)
        Xw = Xo[e0:e0 + per][:, rows].reshape(-1, H + 1, n)
        Uw = U[e0:e0 + per][:, rows[:, :H]].reshape(-1, H, U.shape[2])
        xp, zp = model.rollout(np.ascontiguousarray(Xw[:, 0]), np.ascontiguousarray(Uw), dt)
        ex, ez = xp - Xw, zp - Yw
        sse_x += np.einsum('wkj,wkj->k', ex, ex)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssm_horizon_probe.json'))
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
    from sofacontrol_amd.SSM import sysid
    assert _lib.device_count() >= 1, 'no GPU visible'
    models = {mode: shipped(mode)[0] for mode in MODES}
    g = shipped('map')[1]
    dt = float(g['dt'])
    sizes = [int(s) for s in args.episodes.split(',')]
    host_sizes = [int(s) for s in args.host_episodes.split(',') if s]
    doc = dict(shape=dict(n_x=6, n_y=6, m=4, ROM_order=3, SSM_order=3, T=T, H=H, every=EVERY, stride=1, dt=dt), threads=os.environ.get('OMP_NUM_THREADS'),
               host_chunk_windows=args.chunk, sizes={},
               not_measured=['other shapes (n_x, orders, H, stride)', 'every = 1 at 4096 episodes', 'the modes fe and bil',
                             'host records on side (a) (the upload of the records is outside every clock)', 'hardware counters',
                             'records of a real robot (the records are the model\'s own episodes under the recorded inputs)',
                             'the bytes across PCIe are computed from the copies of a call, not counted',
                             'the host route at the sizes not listed in host_episodes'])
    for E in sizes:
        Y, U = records(models['map'], g, E, seed=E)
        dY, dU = _lib.DeviceBuffer.from_array(Y), _lib.DeviceBuffer.from_array(U)
        for mode in MODES:
            model = models[mode]
            plan = sysid.horizon_plan(model, E, T, H, every=EVERY)
            if args.only_unit:
                for _ in range(3):
                    side_a(model, dY, dU, E, dt)
                    settle()
                continue
            host = E in host_sizes
            warm, timed = (1, 7) if E <= 512 else (1, 5)
            ta, tb, hb = [], [], None
            for it in range(warm + timed):
                a, res = side_a(model, dY, dU, E, dt)
                settle()
                if host and it < warm + 3:                        # the host route takes long: a few runs
                    b, hx, hz, pcie_b = side_b(model, Y, U, args.chunk, dt)
                    settle()
                    if it >= warm:
                        tb.append(b)
                    hb = (hx, hz)
                if it >= warm:
                    ta.append(a)
            W = res.windows
            sa = stat(ta)
            ks = (0, 1, H // 2, H)
            entry = dict(windows=W, diverged=res.diverged, bad_rows=res.bad_rows, plan=plan, unit_seconds=sa,
                         unit_seconds_per_window_step=sa['median'] / (W * H), rms_x=[float(res.rms_x[k]) for k in ks],
                         rms_z=[float(res.rms_z[k]) for k in ks],
                         pcie_bytes_unit=dict(host_to_device=0, device_to_host=8 * 4 * (H + 1) + 8 * 2 * (H + 1) + 16))
            line = 'E = %d %s: %d windows, plan %r; unit %.2f ms (%.2f .. %.2f)' % (E, mode, W, plan, 1e3 * sa['median'], 1e3 * sa['min'], 1e3 * sa['max'])
            if host:
                sb = stat(tb)
                dx, dz = np.abs(res.sse_x - hb[0])[1:] / res.sse_x[1:], np.abs(res.sse_z - hb[1]) / res.sse_z
                entry.update(host_seconds=sb, host_seconds_spread_of_two_runs=float(abs(tb[0] - tb[1])), pcie_bytes_host=pcie_b,
                             sse_x_largest_relative_difference=float(dx.max()), sse_z_largest_relative_difference=float(dz.max()))
                line += '; host route %.3f s (%.3f .. %.3f), %d bytes up, %d down; sse rel. diff x %.2e z %.2e' % (
                    sb['median'], sb['min'], sb['max'], pcie_b['host_to_device'], pcie_b['device_to_host'], dx.max(), dz.max())
            print(line)
            doc['sizes']['%d/%s' % (E, mode)] = entry
        dY.free(); dU.free()
        del Y, U
    if not args.only_unit:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
