"""Closed loop of the Koopman baseline on the Diamond without SOFA: the reference's driver (examples/diamond/diamond_koopman.py:
128-185 -- cost, U box and figure-8 target, here with N = 5) on the shipped 66-observable model (stored as plain arrays in
tests/golden/g22_koopman.npz), with the lifted model itself as the plant.  Every simulation step goes through
`controller.evaluate(sim_time, y, x, u_prev)`: the sample goes into the device ring; every Ts the resident step lifts it
into the QP's x0 and solves (KoopmanSolverNode), one synchronisation.

    python examples/diamond_koopman_closed_loop.py [--steps 400]

Needs an MI355X (no CPU fallback)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400, help='simulation steps of 0.01 s')
    args = ap.parse_args()

    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanModel, KoopmanScaling
    from sofacontrol_amd.baselines.koopman.koopman import KoopmanMPC
    from sofacontrol_amd.baselines.mpc import KoopmanSolverNode
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
    node = KoopmanSolverNode(model, 5, model.Ts, cost, target, U=U)
    ctrl = KoopmanMPC(model, delay=1.0, u0=np.full(model.m, 300.), solver_node=node, rollout_horizon=1)
    sim_dt = 0.01
    ctrl.set_sim_timestep(sim_dt)

    # plant: the lifted model, advanced once per Ts with the input held (zero-order hold on the controller's grid)
    x = np.zeros(model.N)
    x[-1] = 1.0
    u = np.full(model.m, 300.)
    per_ts = int(round(model.Ts / sim_dt))
    err, t_eval = [], []
    for k in range(args.steps):
        y = scaling.scale_up(y=model.H @ x)[0]
        t0 = time.perf_counter()
        u = ctrl.evaluate(k * sim_dt, y, None, u)
        t_eval.append(time.perf_counter() - t0)
        if k % per_ts == per_ts - 1:
            x = model.A_d @ x + model.B_d @ scaling.scale_down(u=u)[0]
        if k * sim_dt >= ctrl.t_delay + 1.0:
            t_rel = k * sim_dt - ctrl.t_delay
            zt = np.array([np.interp(t_rel, target.t, zf[:, j]) for j in range(2)])
            err.append(np.abs(y[:2] - zt).max())
    info = ctrl.save_controller_info()
    print('koopman closed loop: %d steps, %d solves, evaluate median %.3f ms / max %.3f ms, tracking error (x, y) median %.2f mm'
          % (args.steps, len(info['solve_times']), 1e3 * np.median(t_eval), 1e3 * np.max(t_eval),
             np.median(err) if err else float('nan')))


if __name__ == '__main__':
    main()
