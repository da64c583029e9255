"""The set-up of examples/diamond_koopman_closed_loop.py as B closed loops at once: the Koopman baseline on the Diamond -- the shipped
66-observable model (stored as plain arrays in tests/golden/g22_koopman.npz), the reference driver's cost, U box and figure-8 target
(examples/diamond/diamond_koopman.py:128-185, here with N = 5), Ts = 0.05 s on a simulation step of 0.01 s -- on a synthetic TPWL plant
of the Diamond shape (n_x = 60, four cables) whose tip position is the measurement, with seeded disturbed starts, measurement noise and
target phases: the Monte-Carlo run to set beside examples/diamond_rompc_closed_loop_batch.py.  The plant is not the robot the model was
identified on, so the tracking error printed is that of a mismatched model; the loop's mechanics are what the example shows.  All loops
stay on the device (baselines.koopman.closed_loop.KoopmanClosedLoopBatch): one launch sequence and one host wait for the whole run.

    python examples/diamond_koopman_closed_loop_batch.py [--batch 256] [--periods 40] [--rollout-horizon 1] [--seed 0] [--Y 20]

--Y H re-projects every measurement onto the box |y - y_ref|_inf <= H around the tip's rest position before the controller reads it (the
reference driver's Y, examples/diamond/diamond_koopman.py:117), inside the resident loop, and runs the same seeds without Y beside it: the
share of projected samples and the tip error of both runs are printed.

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

N, DT_SIM, U0 = 5, 0.01, 300.0


def diamond_problem():
    """(model, scaling, cost, target, U, zf) of examples/diamond_koopman_closed_loop.py: shared with tools/koopman_loop_probe.py."""
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanModel, KoopmanScaling
    from sofacontrol_amd.tpwl.tpwl_utils import Target
    from sofacontrol_amd.utils import QuadraticCost, HyperRectangle
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g22_koopman.npz'))
    model = KoopmanModel({k: g['model_' + k] for k in ('A', 'B', 'C', 'M', 'K')},
                         {'n': 3, 'm': 4, 'N': 66, 'nzeta': 10, 'delays': 1, 'obs_degree': 2, 'obs_type': 'poly', 'Ts': 0.05,
                          'scale': {k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}})
    scaling = KoopmanScaling(scale=model.scale)
    # diamond_koopman.py:146-185
    target = Target()
    target.t = np.linspace(0, 10, 1000)
    th = np.linspace(0, 2 * np.pi, 1000)
    zf = np.zeros((1000, model.n))
    zf[:, 0] = -15. * np.sin(th)
    zf[:, 1] = 15. * np.sin(2 * th)
    zf[:, 2] -= 114
    target.z = scaling.scale_down(y=zf)
    target.u = scaling.scale_down(u=np.zeros(model.m)).reshape(-1)
    cost = QuadraticCost()
    cost.R = .00001 * np.eye(model.m) * np.diag(scaling.u_factor[0])
    cost.Q = np.zeros((model.n, model.n))
    cost.Q[0, 0] = cost.Q[1, 1] = 100
    cost.Q *= np.diag(scaling.y_factor[0])
    U = HyperRectangle(ub=scaling.scale_down(u=1500. * np.ones(model.m)).reshape(-1),
                       lb=scaling.scale_down(u=200. * np.ones(model.m)).reshape(-1))
    return model, scaling, cost, target, U, zf


def diamond_plant():
    """(TPWL plant pre-discretised at DT_SIM, C (3, 60), y_ref (3)): the synthetic Diamond of workloads.diamond_c2, measured at its tip."""
    import workloads as wl
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    w = wl.diamond_c2()
    n_f = w['U'].shape[0]
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()
    rom_info = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    tp = TPWLATV(data=dict(w['tab'], rom_info=rom_info), params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf,
                 discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        tp.pre_discretize(DT_SIM)
    return tp, np.ascontiguousarray(w['H'][3:6]), np.array([0.0, 0.0, -114.0])


def tip_box(half, y_ref=(0.0, 0.0, -114.0)):
    """The admissible set of the tip measurement: the box of half-width `half` around y_ref, as a Polyhedron that may be projected onto."""
    from sofacontrol_amd.utils import Polyhedron
    y_ref = np.asarray(y_ref, dtype=np.float64)
    A = np.kron(np.eye(3), np.array([[1.0], [-1.0]]))
    b = np.ravel(np.stack([y_ref + half, -(y_ref - half)], axis=1))
    return Polyhedron(A, b, with_reproject=True)


def diamond_koopman(B, max_steps_per_run, rollout_horizon=1, phase=None, Y=None):
    """(loop, model, scaling, plant, C, y_ref, zf, target) of the example's set-up with B members."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    model, scaling, cost, target, U, zf = diamond_problem()
    tp, Cm, y_ref = diamond_plant()
    loop = KoopmanClosedLoopBatch(model, N, cost, tp, Cm, y_ref, DT_SIM, rollout_horizon, t=target.t, z=target.z, u=target.u, phase=phase, U=U,
                                  u0=np.full(model.m, U0), batch=B, max_steps_per_run=max_steps_per_run)
    if Y is not None:
        loop.set_reproject(Y)
    return loop, model, scaling, tp, Cm, y_ref, zf, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--periods', type=int, default=40, help='periods of rollout_horizon controller steps of 0.05 s')
    ap.add_argument('--rollout-horizon', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--Y', type=float, default=None, metavar='H', help='re-project the measurements onto the box of half-width H around the tip at rest')
    args = ap.parse_args()
    B, P, rh = args.batch, args.periods, args.rollout_horizon

    rng = np.random.default_rng(args.seed)
    phase = rng.uniform(0.0, 1.0, B)
    nk = 5 * rh
    loop, model, scaling, tp, Cm, y_ref, zf, target = diamond_koopman(B, P * nk, rollout_horizon=rh, phase=phase)
    x0 = 0.5 * rng.standard_normal((B, loop.n_plant))                        # disturbed starts around the rest configuration
    y_rest = x0 @ Cm.T + y_ref
    V = 0.05 * rng.standard_normal((P, nk, B, loop.n_y))
    # the history in front of the first solve: the plant at rest under the idle input
    loop.reset(x0=x0, y_hist=y_rest[:, None, :], u_hist=np.full((B, 1, model.m), U0), u_prev0=np.full((B, model.m), U0))
    t0 = time.perf_counter()
    res = loop.run(P, V=V)
    wall = time.perf_counter() - t0

    want = np.stack([np.stack([np.interp(phase[b] + res.t, target.t, zf[:, j]) for j in (0, 1)], axis=1) for b in range(B)])
    err = np.linalg.norm(res.y[:, 1:, :2] - want[:, 1:], axis=2)
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    print('koopman closed loop batch: %d loops x %d periods (%.2f s each), waits_last_run %d, %.2f ms per period'
          % (B, P, P * nk * DT_SIM, loop.stats()['waits_last_run'], 1e3 * wall / P))
    print('tip error (x, y) rms per loop: median %.3f, best %.3f, worst %.3f   (target amplitude 15.0; the plant is not the model\'s robot)'
          % (np.median(rms), rms.min(), rms.max()))
    print('inputs applied: min %.1f, max %.1f (box 200 .. 1500)' % (res.u.min(), res.u.max()))
    codes, counts = np.unique(res.status, return_counts=True)
    print('solve status over %d solves: ' % res.status.size + ', '.join('%d: %d' % (int(c), k) for c, k in zip(codes, counts)))
    assert np.isfinite(res.x).all() and np.isfinite(res.y).all() and np.isfinite(res.u).all()

    if args.Y is not None:
        loop_y = diamond_koopman(B, P * nk, rollout_horizon=rh, phase=phase, Y=tip_box(args.Y))[0]
        loop_y.reset(x0=x0, y_hist=y_rest[:, None, :], u_hist=np.full((B, 1, model.m), U0), u_prev0=np.full((B, model.m), U0))
        ry = loop_y.run(P, V=V)
        err_y = np.linalg.norm(ry.y[:, 1:, :2] - want[:, 1:], axis=2)
        rms_y = np.sqrt(np.mean(err_y ** 2, axis=1))
        words, counts = np.unique(ry.proj, return_counts=True)
        print('with Y = tip box of half-width %g: %.1f %% of the %d samples projected (status words ' % (args.Y, 100.0 * np.mean(ry.proj == 1), ry.proj.size)
              + ', '.join('%d: %d' % (int(c), k) for c, k in zip(words, counts)) + ')')
        print('tip error (x, y) rms per loop with Y: median %.3f, best %.3f, worst %.3f   (without Y: median %.3f, best %.3f, worst %.3f)'
              % (np.median(rms_y), rms_y.min(), rms_y.max(), np.median(rms), rms.min(), rms.max()))
        assert np.isfinite(ry.y_used).all() and (ry.proj >= 0).all()


if __name__ == '__main__':
    main()
