"""Batched closed-loop iLQR probe (csrc/ilqr_loop.hip, the resident plan of csrc/lqr.hip): B loops on the Diamond shape of
examples/diamond_ilqr_closed_loop_batch.py (n_x = 60, n_u = 4, n_z = 6, n_y = 30, a synthetic TPWL plant, dt = dt_sim = 0.01, horizon N)
for B in {1, 256, 4096}.

Two ways to close the same loops from the same states, alternated run by run in one process:
  (a) ILQRClosedLoopBatch: reset, plan() (the solve on the device, K stays there) and run(N) (one launch sequence, one wait);
  (b) what the library offered before: one batched iLQR.ilqr_computation (x, u and K come down over PCIe), then per step the law in
      numpy, one batched plant step (linearize_batch and the affine update in numpy) and, with --observer, one batched filter step.
      (b) runs twice (b, b2): the difference of the two medians is the spread of the host figure.
The solve and the tracking are timed separately on both sides (host clock; (a)'s solve is timed to a wait of its own that the loop does
not need, so (a) is also timed whole: plan + run with the single wait).  Inputs of the two sides are compared; the figure is reported,
not judged.  Bytes across PCIe are computed from the shapes.  The split of a step between point search, gain product and plant product
needs a kernel trace of its own and is not measured here.

    python tools/ilqr_loop_probe.py [--out profiles/ilqr_loop_probe.json] [--batches 1,256,4096] [--N 100] [--observer]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

DT = 0.01


def runs_for(B):
    """(warm-up, timed) runs."""
    return (2, 7) if B <= 16 else ((2, 5) if B <= 512 else (1, 3))


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def problem(B, N, observer, seed=0):
    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import QuadraticCost
    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()
    Cf = linearModel(nodes=[1354, 200, 600, 1000, 1500], num_nodes=n_f // 3).C.tocsr() if observer else None
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, Cf=Cf, discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        model.pre_discretize(DT)
    rng = np.random.default_rng(seed)
    x0 = 0.5 * rng.standard_normal((B, 2 * r))
    phase = rng.uniform(0.0, float(w['t'][-1]) / 2, B)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    z = zi(phase[:, None] + DT * np.arange(N + 1)) + np.asarray(model.z_ref)
    policy = iLQR(DT, model, QuadraticCost(Q=w['Qz'], R=w['R'], Qf=10.0 * w['Qz']), N)
    x_hat0 = x0 + 0.1 * rng.standard_normal(x0.shape) if observer else None
    return model, policy, x0, x_hat0, z


def host_run(model, policy, obs, rows, x0, x_hat0, z, N):
    """Loop (b): returns (solve ms, tracking ms, U (B, N, m), x (B, n))."""
    t0 = time.perf_counter()
    policy.set_target(z)
    belief = x0 if obs is None else x_hat0
    xb, ub, K = policy.ilqr_computation(belief)
    t1 = time.perf_counter()
    x, xh = x0.copy(), None if obs is None else x_hat0.copy()
    if obs is not None:
        obs.initialize(xh)
        obs.Sigma = np.broadcast_to(obs._Sigma0, (x0.shape[0],) + obs._Sigma0.shape)
    C, y_ref = (None, None) if obs is None else (np.asarray(model.C), np.asarray(model.y_ref))
    U = np.empty((x0.shape[0], N, ub.shape[2]))
    for s in range(N):
        row = int(rows[s])
        xl = x if obs is None else xh
        u = ub[:, row] + np.einsum('bij,bj->bi', K[:, row], xl - xb[:, row]) if row >= 0 else np.zeros_like(U[:, 0])
        A, Bm, d, _ = model.linearize_batch(x, DT)
        x = np.einsum('bij,bj->bi', A, x) + np.einsum('bij,bj->bi', Bm, u) + d
        if obs is not None:
            obs.update(u, x @ C.T + y_ref, DT)
            xh = obs.x
        U[:, s] = u
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), U, x


def pcie_bytes(B, N, n, m, nz, ny, observer):
    D = 8
    res_up = B * n * D * (2 if observer else 1)                                     # reset: x0 (and x_hat0); the target is counted apart
    res_down = B * ((N + 1) * nz + N * m) * D + (B * ((N + 1) * n + N * ny) * D + B * 4 if observer else 0) + B * (D + 4)
    host_up = B * (n + (N + 1) * nz + m) * D + N * B * n * D + (N * B * (m + ny) * D if observer else 0)
    host_down = B * ((N + 1) * n + N * m + N * m * n + 1) * D + B * 4 + N * B * (n * n + n * m + n) * D + N * B * 4 + (N * B * n * D if observer else 0)
    return dict(resident=dict(up=res_up, down=res_down, target_up=B * (N + 1) * nz * D),
                host_driven=dict(up=host_up, down=host_down, of_which_K_down=B * N * m * n * D))


def probe(B, N, observer):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    model, policy, x0, x_hat0, z = problem(B, N, observer)
    n, m = x0.shape[1], policy.input_dim
    mk = lambda: DiscreteEKFObserverBatch(model, B, W=100.0 * np.eye(n), V=np.eye(30)) if observer else None
    loop = ILQRClosedLoopBatch(policy, model, DT, B, z=z, observer=mk(), max_steps_per_run=N)
    hobs, hobs2 = mk(), mk()
    warm, timed = runs_for(B)
    t = dict(a_solve=[], a_run=[], a_whole=[], b_solve=[], b_track=[], b2_solve=[], b2_track=[])
    agree = dict(u_rel_diff=0.0, x_rel_diff=0.0)
    quiet = contextlib.redirect_stdout(io.StringIO())
    for k in range(warm + timed):
        loop.reset(x0, x_hat0)
        t0 = time.perf_counter()
        loop.plan()
        _lib.sync()
        t1 = time.perf_counter()
        ra = loop.run(N, record_x=True)
        t2 = time.perf_counter()
        loop.reset(x0, x_hat0)
        t3 = time.perf_counter()
        loop.plan()
        loop.run(N, record_x=observer)
        t4 = time.perf_counter()
        with quiet:
            bs, bt, Ub, xb_ = host_run(model, policy, hobs, loop.rows, x0, x_hat0, z, N)
            b2s, b2t, _, _ = host_run(model, policy, hobs2, loop.rows, x0, x_hat0, z, N)
        if k >= warm:
            for key, v in (('a_solve', 1e3 * (t1 - t0)), ('a_run', 1e3 * (t2 - t1)), ('a_whole', 1e3 * (t4 - t3)), ('b_solve', bs), ('b_track', bt),
                           ('b2_solve', b2s), ('b2_track', b2t)):
                t[key].append(v)
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(ra.u - Ub).max() / max(1.0, np.abs(Ub).max())))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(ra.x[:, -1] - xb_).max() / max(1.0, np.abs(xb_).max())))
    s = {k: stat(v) for k, v in t.items()}
    host = s['b_solve']['median'] + s['b_track']['median']
    host2 = s['b2_solve']['median'] + s['b2_track']['median']
    info = loop.plan_info()
    return dict(batch=B, N=N, observer=bool(observer), warm_up_runs=warm, timed_runs=timed, agreement=agree,
                resident_solve_ms=s['a_solve'], resident_tracking_ms=s['a_run'], resident_plan_plus_run_ms=s['a_whole'],
                host_solve_ms=s['b_solve'], host_tracking_ms=s['b_track'], host_repeat_solve_ms=s['b2_solve'], host_repeat_tracking_ms=s['b2_track'],
                host_whole_ms_median=host, host_spread_ms=abs(host - host2), host_over_resident=host / s['a_whole']['median'],
                waits_last_run=loop.stats()['waits_last_run'], ilqr_iterations_median=float(np.median(info['iters'])),
                pcie_bytes_per_run=pcie_bytes(B, N, n, m, loop.n_z, 30, observer))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ilqr_loop_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    ap.add_argument('--N', type=int, default=100)
    ap.add_argument('--observer', action='store_true')
    args = ap.parse_args()
    res = dict(shape=dict(n_x=60, n_u=4, n_z=6, n_y=30, dt=DT, dt_sim=DT, r=1, plant='a synthetic TPWL model of n_x = 60, P = 64 points'),
               note='ms per run of N steps: host clock; resident_plan_plus_run is reset-free plan() + run(N) with the loop\'s single wait; '
                    'resident_solve is timed to a wait of its own; the sides alternate run by run; the split of a step between point search, '
                    'gain product and plant product is not measured here: it needs a kernel trace of its own',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(probe(B, args.N, args.observer))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
