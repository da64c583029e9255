"""Monte-Carlo closed loops on an SSM reduced model, resident on the device: `--batch` receding-horizon loops of the reference's SSM
driver (examples/hardware/diamond_SSM.py: SSMGuSTO, u = u_bar(t), x_hat = W_map(y - z_ref)) on the synthetic polynomial model of
examples/ssm_closed_loop.py, every loop with its own start, target phase, disturbance and measurement noise, and -- with `--mismatch` --
a plant that differs from the planner's model.  One launch sequence and one host wait for the whole run (scp.closed_loop_ssm).

    python examples/ssm_closed_loop_batch.py [--batch 256] [--periods 25] [--mismatch 0.02]

Needs an MI355X (no CPU fallback)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256, help='loops')
    ap.add_argument('--periods', type=int, default=25, help='replanning periods of 2 x 0.02 s')
    ap.add_argument('--mismatch', type=float, default=0.0, help='the plant\'s nonlinear coefficients moved this far towards another model')
    args = ap.parse_args()

    from oracle import ssm as ossm                      # only the synthetic model generator
    from test_ssm_gpu import product_ssm
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.utils import HyperRectangle

    n, m, N, dt, n_keep, B = 4, 2, 8, 0.02, 2, args.batch
    model = ossm.synthetic(n, m, 3, 2, seed=81)
    model['W'][:] = 0.0; model['W'][:, :n] = np.eye(n)          # consistent observation / reduction maps: z = x + z_ref
    model['V'][:] = 0.0; model['V'][:, :n] = np.eye(n)
    planner = product_ssm(model, discr='fe')
    plant = planner
    if args.mismatch > 0:
        other = ossm.synthetic(n, m, 3, 2, seed=181)
        pm = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in model.items()}
        pm['R'][:, n:] += args.mismatch * (other['R'][:, n:] - model['R'][:, n:])
        plant = product_ssm(pm, discr='be')
    rng = np.random.default_rng(0)
    x0 = 0.02 * rng.standard_normal((B, n))
    t = np.linspace(0.0, 4.0, 201)                              # a slow circle of the first two outputs, in the solver's coordinates
    z = np.zeros((201, n)); z[:, 0] = 0.08 * np.sin(0.5 * np.pi * t); z[:, 1] = 0.04 * (1.0 - np.cos(0.5 * np.pi * t))
    phase = rng.uniform(0.0, 2.0, B)
    u_init = np.zeros((B, N, m))
    x_init, _ = planner.rollout(x0, u_init, dt)
    Qz, R = np.diag([10., 10., 0.1, 0.1]), 1e-2 * np.eye(m)
    gu = GuSTO(SSMGuSTO(planner), N, dt, Qz, R, x0, u_init, x_init, z=np.tile(z[0], (B, N + 1, 1)), U=HyperRectangle([2.0] * m, [-2.0] * m),
               verbose=0, max_gusto_iters=4, convg_thresh=1e-4, batch=B, first_solve_cap=1, max_trace=0)
    S = args.periods * n_keep
    cl = SSMClosedLoopBatch(gu, plant, dt, n_keep, t=t, z=z, phase=phase, max_steps_per_run=S)
    cl.reset(x0, 0.0, v0=1e-4 * rng.standard_normal((B, n)))
    W = 1e-4 * rng.standard_normal((args.periods, n_keep, B, n)); V = 1e-4 * rng.standard_normal((args.periods, n_keep, B, n))
    t0 = time.perf_counter()
    r = cl.run(args.periods, W=W, V=V)
    wall = time.perf_counter() - t0
    target = np.stack([np.stack([np.interp(r.t + ph, t, z[:, c]) for c in range(2)], axis=1) for ph in phase])
    e = np.linalg.norm(r.z[:, :, :2] - target, axis=2)
    print('%d loops x %d periods (%d plant steps) in %.1f ms, %d host wait(s); SCP iterations per solve: mean %.2f, max %d; status != 0: %d'
          % (B, args.periods, S, 1e3 * wall, cl.stats()['waits_last_run'], r.iters.mean(), r.iters.max(), int((r.status != 0).sum())))
    print('tracked-output error over the loops: start median %.4f, end median %.4f, end worst %.4f; estimate error |x_hat - x| end worst %.2e'
          % (np.median(e[:, 0]), np.median(e[:, -1]), e[:, -1].max(), np.abs(r.x_hat[:, -1] - r.x[:, -1]).max()))


if __name__ == '__main__':
    main()
