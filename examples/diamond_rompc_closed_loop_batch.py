"""The set-up of examples/diamond_rompc_closed_loop.py as B closed loops at once: the linear ROMPC baseline on the Diamond shape
(synthetic TPWL model linearised at its first point, five measured nodes, tip output model, N = 5 at 0.05 s, N_replan = 10 at 0.01 s,
the TPWL model as the plant) with seeded disturbed starts, wrong initial estimates, measurement noise and target phases -- the
Monte-Carlo run to set beside examples/diamond_closed_loop_batch.py.  All loops stay on the device
(baselines.rompc.closed_loop.ROMPCClosedLoopBatch): one launch sequence and one host wait for the whole run.

    python examples/diamond_rompc_closed_loop_batch.py [--loops 256] [--periods 20] [--seed 0]

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


def diamond_rompc(B, max_steps_per_run, phase=None, plant=True):
    """(loop, model, plant, w) of the example's Diamond set-up with B members: shared with tools/rompc_loop_probe.py."""
    import workloads as wl
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
    from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
    from sofacontrol_amd.lqr.lqr import dare
    from sofacontrol_amd.measurement_models import linearModel, MeasurementModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import QuadraticCost, HyperRectangle, Polyhedron

    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    m, dt_sim, dt_mpc = w['m'], 0.01, 0.05
    num_nodes = n_f // 3
    nodes = [1354, 726, 139, 1445, 729]                                      # diamond_rompc.py:13
    Hf = linearModel(nodes=[nodes[0]], num_nodes=num_nodes).C.tocsr()
    Cf = MeasurementModel(nodes, num_nodes).C.tocsr()                        # 30 measurements
    rom_info = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    lin = dict(A_c=w['tab']['A_c'][0], B_c=w['tab']['B_c'][0], d_c=w['tab']['d_c'][0], rom_info=rom_info)
    model = LinearROM(lin, dt_sim, Cf=Cf, Hf=Hf)
    mpc_model = LinearROM(lin, dt_mpc, Hf=Hf)
    tp = TPWLATV(data=dict(w['tab'], rom_info=rom_info), params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf,
                 discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(dt_sim)
    # controller side (diamond_rompc.py:67-80): the gains ROMPC computes
    cost = QuadraticCost(Q=model.H.T @ w['Qz'] @ model.H, R=1e-4 * np.eye(m))
    costL = QuadraticCost(Q=cost.Q, R=1e-3 * np.eye(model.meas_dim))
    observer = DiscreteLuenbergerObserver(model, costL.Q, costL.R, batch=B)
    observer.K, _ = dare(model.A_d, model.B_d, cost.Q, cost.R)
    # solver side (diamond_rompc.py:108-145): output cost, U box, tip polyhedron
    loop = ROMPCClosedLoopBatch(observer, mpc_model, 5, dt_mpc, QuadraticCost(Q=w['Qz'], R=1e-5 * np.eye(m)), tp if plant else None, dt_sim, 10,
                                t=w['t'], z=w['z'], phase=phase, U=HyperRectangle([1500.] * m, [0.] * m), X=Polyhedron(w['XA'], w['Xb']),
                                max_steps_per_run=max_steps_per_run)
    return loop, model, tp, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loops', type=int, default=256)
    ap.add_argument('--periods', type=int, default=20, help='re-planning periods of 10 steps of 0.01 s')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    B, P, nk = args.loops, args.periods, 10

    rng = np.random.default_rng(args.seed)
    phase = rng.uniform(0.0, 1.0, B)
    loop, model, tp, w = diamond_rompc(B, P * nk, phase=phase)
    n, ny = loop.n_x, loop.n_y
    x0 = 0.5 * rng.standard_normal((B, n))                                   # disturbed starts
    x_hat0 = x0 + 0.1 * rng.standard_normal((B, n))                          # the observers start off the plant
    V = 0.05 * rng.standard_normal((P, nk, B, ny))
    loop.reset(x0, x_hat0)
    t0 = time.perf_counter()
    res = loop.run(P, V=V)
    wall = time.perf_counter() - t0

    target = np.stack([np.stack([np.interp(phase[b] + res.t, w['t'], w['z'][:, j]) for j in (3, 4)], axis=1) for b in range(B)])
    err = np.linalg.norm(res.z[:, 1:, 3:5] - target[:, 1:], axis=2)
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    e = np.linalg.norm(res.x_hat - res.x, axis=2)
    print('rompc closed loop batch: %d loops x %d periods (%.2f s each), waits_last_run %d, %.2f ms per period'
          % (B, P, P * nk * 0.01, loop.stats()['waits_last_run'], 1e3 * wall / P))
    print('tip error (x, y) rms per loop: median %.3f, best %.3f, worst %.3f   (target amplitude %.1f)'
          % (np.median(rms), rms.min(), rms.max(), np.abs(w['z'][:, 3:5]).max()))
    print('observer error |x_hat - x| start -> end (median): %.3f -> %.3f' % (np.median(e[:, 0]), np.median(e[:, -1])))
    codes, counts = np.unique(res.status, return_counts=True)
    print('solve status over %d solves: ' % res.status.size + ', '.join('%d: %d' % (int(c), k) for c, k in zip(codes, counts)))
    assert np.isfinite(res.x).all() and np.isfinite(res.u).all()


if __name__ == '__main__':
    main()
