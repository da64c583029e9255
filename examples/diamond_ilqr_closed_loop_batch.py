"""The iLQR controller of the reference's run_ilqr (examples/diamond/diamond.py:318-389) as B closed loops at once: the C2 Diamond shape
(synthetic TPWL model, the model itself as the plant), controller and simulation step 0.01 s, a horizon of --steps steps, seeded initial
states and target phases -- a Monte-Carlo validation of the iLQR policy.  Every loop plans once from its belief (one batched iLQR solve;
the gains K, B x N x n_u x n_x doubles, never leave the device) and then tracks its per-step policy; plan and run stay on the device
(lqr.closed_loop.ILQRClosedLoopBatch): one launch sequence and one host wait for the whole run.  Without --observer state feedback is
perfect; with it every loop carries its own extended Kalman filter (tpwl.observer.DiscreteEKFObserverBatch) on five measured nodes
(n_y = 30) with measurement noise and a wrong initial estimate, plans from the estimate and controls from it.

    python examples/diamond_ilqr_closed_loop_batch.py [--loops 256] [--steps 100] [--seed 0] [--observer]

Needs an MI355X (no CPU fallback)."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loops', type=int, default=256)
    ap.add_argument('--steps', type=int, default=100, help='controller = simulation steps of 0.01 s: the horizon of the plan and the length of the run')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--observer', action='store_true', help='output feedback: one EKF per loop on five measured nodes, noise, wrong initial estimate')
    args = ap.parse_args()

    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import QuadraticCost

    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    m, dt, B, N = w['m'], 0.01, args.loops, args.steps
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()              # tip velocity + position (diamond.py:269)
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    Cf = linearModel(nodes=[1354, 200, 600, 1000, 1500], num_nodes=n_f // 3).C.tocsr() if args.observer else None
    model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, Cf=Cf, discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        model.pre_discretize(dt)

    rng = np.random.default_rng(args.seed)
    x0 = 0.5 * rng.standard_normal((B, 2 * r))
    phase = rng.uniform(0.0, float(w['t'][-1]) / 2, B)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    z_rel = zi(phase[:, None] + dt * np.arange(N + 1))                        # (B, N + 1, 6) around the rest tip, as the loop records z = H x
    z = z_rel + np.asarray(model.z_ref)                                       # absolute, as iLQR.set_target's
    policy = iLQR(dt, model, QuadraticCost(Q=w['Qz'], R=w['R'], Qf=10.0 * w['Qz']), N)
    observer = DiscreteEKFObserverBatch(model, B, W=100.0 * np.eye(2 * r), V=np.eye(30)) if args.observer else None
    loop = ILQRClosedLoopBatch(policy, model, dt, B, z=z, observer=observer, max_steps_per_run=N)
    noise = None
    if args.observer:
        x_hat0 = x0 + 0.1 * rng.standard_normal(x0.shape)                     # where a first update at t = 0 would have left the filters
        noise = 0.05 * rng.standard_normal((N, B, 30))
        loop.reset(x0, x_hat0)
    else:
        loop.reset(x0)
    t0 = time.perf_counter()
    loop.plan()
    res = loop.run(N, V=noise, record_x=args.observer)
    wall = time.perf_counter() - t0
    info = loop.plan_info()

    err = np.linalg.norm((res.z - z_rel)[:, 1:, 3:5], axis=2)
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    print('%d loops x %d steps of %.2f s, plan + run %.1f ms, waits_last_run %d' % (B, N, dt, 1e3 * wall, loop.stats()['waits_last_run']))
    print('tip error rms (x, y) per loop: median %.3f, best %.3f, worst %.3f   (target amplitude %.1f)' %
          (np.median(rms), rms.min(), rms.max(), np.abs(w['z'][:, 3:5]).max()))
    print('iLQR iterations per loop: median %d, max %d; diverged: %d' % (np.median(info['iters']), info['iters'].max(), int((info['iters'] < 0).sum())))
    for b in range(min(B, 8)):
        print('  loop %d: phase %.2f s, tip error rms %.3f, plan cost %.4g in %d iterations' % (b, phase[b], rms[b], info['cost'][b], info['iters'][b]))
    if args.observer:
        H = np.asarray(model.H)
        e = np.linalg.norm(res.x_hat - res.x, axis=2)
        ez = np.linalg.norm((res.x_hat - res.x) @ H.T, axis=2)
        print('estimate error over the loops, start -> end (median): state |x_hat - x| %.3f -> %.3f, tip output |H (x_hat - x)| %.3f -> %.3f; '
              'filters that reported a failure: %d' % (np.median(e[:, 0]), np.median(e[:, -1]), np.median(ez[:, 0]), np.median(ez[:, -1]),
                                                       int((res.ekf_status != 0).sum())))


if __name__ == '__main__':
    main()
