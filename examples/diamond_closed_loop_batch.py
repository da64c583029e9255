"""The problem of examples/diamond_closed_loop.py as B closed loops at once: the C2 Diamond shape (synthetic TPWL model, the model
itself as the plant at dt_sim = 0.01), seeded initial states and target phases, the scp controller's per-point DARE gains -- a
Monte-Carlo validation of the controller.  All loops stay on the device (scp.closed_loop.ClosedLoopBatch): one launch sequence and
one host wait for the whole run.  Without --observer state feedback is perfect; with it every loop carries its own extended Kalman
filter (tpwl.observer.DiscreteEKFObserverBatch) on five measured nodes (n_y = 30) with measurement noise and a wrong initial
estimate, plans from the estimate and controls from it -- the loop the reference's drivers close.

    python examples/diamond_closed_loop_batch.py [--batch 256] [--periods 20] [--seed 0] [--observer] [--chained]

--chained runs the reference's default policy, mpc=False (tpwl/controllers.py:236; what examples/diamond/diamond.py:249 runs): plan
k + 1 starts from the end of the followed part of plan k, not from the plant state or the estimate, so only the law and the filter
close the loop.  It then runs mpc=True -- every period re-plans from the plant -- on the same seeds, and prints the tip error of both.

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
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--periods', type=int, default=20, help='re-planning periods of 10 steps of 0.01 s')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--observer', action='store_true', help='output feedback: one EKF per loop on five measured nodes, noise, wrong initial estimate')
    ap.add_argument('--chained', action='store_true', help="the reference's default policy mpc=False, then mpc=True on the same seeds")
    args = ap.parse_args()

    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.lqr.lqr import dare_batch
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import HyperRectangle, Polyhedron

    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    m, N, dt, dt_sim, n_keep, B = w['m'], w['N'], w['dt'], 0.01, 10, args.batch
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()              # tip velocity + position (diamond.py:269)
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    Cf = linearModel(nodes=[1354, 200, 600, 1000, 1500], num_nodes=n_f // 3).C.tocsr() if args.observer else None
    model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, Cf=Cf, discr_method='zoh')
    gm = TPWLGuSTO(model)
    with contextlib.redirect_stdout(io.StringIO()):
        gm.pre_discretize(dt)
    H = np.asarray(model.H)
    # the gains of the scp controller (tpwl/controllers.py: _point_gains): DARE at every table point, discretised at dt_sim
    tab = model.tpwl_dict
    Ad, Bd, dd = model.discretize_batch(np.stack(tab['A_c']), np.stack(tab['B_c']), np.stack(tab['d_c']), dt_sim)
    model.handle_for(dt_sim, tables=(Ad, Bd, dd))                            # the plant: the same model stepped at dt_sim
    K, _ = dare_batch(Ad, Bd, H.T @ w['Qz'] @ H + 1e-3 * np.eye(2 * r), 1e-4 * np.eye(m))

    rng = np.random.default_rng(args.seed)
    x0 = 0.5 * rng.standard_normal((B, 2 * r))
    phase = rng.uniform(0.0, float(w['t'][-1]) / 2, B)
    u_init = np.zeros((B, N, m))
    x_init, _ = gm.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    xc, fc = gm.get_characteristic_vals()
    gusto = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=zi(phase[:, None] + dt * np.arange(N + 1)),
                  U=HyperRectangle([1500.] * m, [0.] * m), X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3,
                  max_gusto_iters=3, batch=B, first_solve_cap=1, max_trace=0)
    observer = DiscreteEKFObserverBatch(model, B, W=100.0 * np.eye(2 * r), V=np.eye(30)) if args.observer else None
    if args.observer:
        x_hat0 = x0 + 0.1 * rng.standard_normal(x0.shape)                     # where a first update at t = 0 would have left the filters
        noise = 0.05 * rng.standard_normal((args.periods, n_keep, B, 30))

    def run_policy(mpc):
        """(loop, records, seconds) of one policy on the seeded states, estimates and noise."""
        loop = ClosedLoopBatch(gusto, model, dt_sim, n_keep, t=w['t'], z=w['z'], phase=phase, K=K, max_steps_per_run=args.periods * n_keep,
                               observer=observer, mpc=mpc, record_tape=not mpc)
        if args.observer:
            loop.reset_observed(x0, x_hat0)
            t0 = time.perf_counter()
            res = loop.run_observed(args.periods, V=noise)
        else:
            loop.reset(x0)
            t0 = time.perf_counter()
            res = loop.run(args.periods, record_x=False)
        return loop, res, time.perf_counter() - t0

    def tip_rms(res):
        target = zi(phase[:, None] + res.t[None, :])                          # (B, S + 1, 6)
        err = np.linalg.norm((res.z - target)[:, 1:, 3:5], axis=2)
        return np.sqrt(np.mean(err ** 2, axis=1))

    loop, res, wall = run_policy(not args.chained)
    rms = tip_rms(res)
    if args.chained:
        _, res_mpc, wall_mpc = run_policy(True)
        rms_mpc = tip_rms(res_mpc)
        # the nominal tape the loops follow (the reference's x_opt of save_controller_info), as outputs: how far the PLAN is from the target
        tape = np.linalg.norm((res.x_bar @ H.T - zi(phase[:, None] + res.t[None, :]))[:, 1:, 3:5], axis=2)
        print('policy mpc=False (chained, the reference\'s default): tip rms median %.3f, worst %.3f; its nominal tape alone: median %.3f; '
              '%.1f ms per period' % (np.median(rms), rms.max(), np.median(np.sqrt(np.mean(tape ** 2, axis=1))), 1e3 * wall / args.periods))
        print('policy mpc=True  (re-plan from the %s):           tip rms median %.3f, worst %.3f; %.1f ms per period'
              % ('estimate' if args.observer else 'plant', np.median(rms_mpc), rms_mpc.max(), 1e3 * wall_mpc / args.periods))
        print('loops where the chained policy tracks better: %d of %d (the records below are the chained policy\'s)' % (int((rms < rms_mpc).sum()), B))
    print('%d loops x %d periods (%.2f s each), %d host wait(s), %.1f ms per period' %
          (B, args.periods, args.periods * n_keep * dt_sim, loop.stats()['waits_last_run'], 1e3 * wall / args.periods))
    print('tip tracking rms (x, y) per loop: median %.3f, best %.3f, worst %.3f   (target amplitude %.1f)' %
          (np.median(rms), rms.min(), rms.max(), np.abs(w['z'][:, 3:5]).max()))
    for b in range(min(B, 8)):
        print('  loop %d: phase %.2f s, rms %.3f, SCP iterations per period %.1f' % (b, phase[b], rms[b], res.iters[:, b].mean()))
    if args.observer:
        # W = 100 I trusts the measurements: their noise reaches the weakly observed directions of the state amplified, the outputs hardly
        e = np.linalg.norm(res.x_hat - res.x, axis=2)                         # (B, S + 1)
        ez = np.linalg.norm((res.x_hat - res.x) @ H.T, axis=2)
        print('estimate error over the loops, start -> end (median): state |x_hat - x| %.3f -> %.3f, tip output |H (x_hat - x)| %.3f -> %.3f; '
              'filters that reported a failure: %d' % (np.median(e[:, 0]), np.median(e[:, -1]), np.median(ez[:, 0]), np.median(ez[:, -1]),
                                                       int(res.ekf_status.any(axis=0).sum())))
    names = {0: 'converged', 1: 'QP failed', 2: 'omega > omega_max', 3: 'max iterations'}
    codes, counts = np.unique(res.status, return_counts=True)
    print('solve status over %d solves: ' % res.status.size + ', '.join('%s %d' % (names.get(int(c), str(int(c))), n) for c, n in zip(codes, counts)))
    sat = (res.u <= 1e-6) | (res.u >= 1500.0 - 1e-6)
    print('input outside (0, 1500) on %.1f%% of the steps (the loop does not clip: the reference does not)' % (100 * sat.any(axis=2).mean()))


if __name__ == '__main__':
    main()
