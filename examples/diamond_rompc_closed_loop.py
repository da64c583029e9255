"""Closed loop of the linear ROMPC baseline on the Diamond shape without SOFA: the reference's driver
(examples/diamond/diamond_rompc.py:32-145 -- MeasurementModel over five nodes, tip output model, costs, N_replan = 10; the
solver side with N = 5, the U box and the tip polyhedron of run_rompc_solver) on the synthetic TPWL model of
examples/diamond_closed_loop.py, linearised at its first point (TPWL2LinearROM's choice), with the TPWL model as the plant.
Every simulation step goes through `controller.evaluate(sim_time, y, x, u_prev)`: one resident step on the device
(feedback on the estimate + Luenberger update); every N_replan steps the reduced OCP is solved by the in-process MPC node.

    python examples/diamond_rompc_closed_loop.py [--steps 300]

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
    ap.add_argument('--steps', type=int, default=300, help='simulation steps of 0.01 s')
    args = ap.parse_args()

    import workloads as wl
    from sofacontrol_amd.measurement_models import linearModel, MeasurementModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.tpwl.tpwl_utils import Target
    from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
    from sofacontrol_amd.baselines.rompc.rompc import ROMPC
    from sofacontrol_amd.baselines.mpc import MPCSolverNode
    from sofacontrol_amd.utils import QuadraticCost, HyperRectangle, Polyhedron

    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    m, dt_sim, dt_mpc = w['m'], 0.01, 0.05
    num_nodes = n_f // 3
    nodes = [1354, 726, 139, 1445, 729]                                      # diamond_rompc.py:13
    Hf = linearModel(nodes=[nodes[0]], num_nodes=num_nodes).C.tocsr()
    Cf = MeasurementModel(nodes, num_nodes).C.tocsr()                        # 30 measurements: the wide observer DARE
    rom_info = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    lin = dict(A_c=w['tab']['A_c'][0], B_c=w['tab']['B_c'][0], d_c=w['tab']['d_c'][0], rom_info=rom_info)
    model = LinearROM(lin, dt_sim, Cf=Cf, Hf=Hf)
    mpc_model = LinearROM(lin, dt_mpc, Hf=Hf)
    plant = TPWLATV(data=dict(w['tab'], rom_info=rom_info), params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}),
                    Hf=Hf, discr_method='zoh')
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        plant.pre_discretize(dt_sim)
    # controller side (diamond_rompc.py:67-80)
    cost = QuadraticCost(Q=model.H.T @ w['Qz'] @ model.H, R=1e-4 * np.eye(m))
    costL = QuadraticCost(Q=cost.Q, R=1e-3 * np.eye(model.meas_dim))
    # solver side (diamond_rompc.py:108-145): output cost, U box, tip polyhedron
    target = Target()
    target.t, target.z = w['t'], w['z']
    node = MPCSolverNode(mpc_model, 5, dt_mpc, QuadraticCost(Q=w['Qz'], R=1e-5 * np.eye(m)), target,
                         U=HyperRectangle([1500.] * m, [0.] * m), X=Polyhedron(w['XA'], w['Xb']))
    ctrl = ROMPC(model, cost, costL, dt_sim, N_replan=10, delay=0.05, solver_node=node)
    ctrl.set_sim_timestep(dt_sim)

    xr = np.zeros(2 * r)
    u = np.zeros(m)
    err, t_eval = [], []
    for k in range(args.steps):
        t = k * dt_sim
        x_full = model.rom.compute_FO_state(x=xr)                            # what SOFA hands to the controller
        y = np.asarray(Cf @ x_full).ravel()
        t0 = time.perf_counter()
        with quiet:
            u = ctrl.evaluate(t, y, x_full, u)
        t_eval.append(time.perf_counter() - t0)
        xr = plant.update_state(xr, u, dt_sim)
        if t >= ctrl.t_delay:
            z_tgt = np.array([np.interp(t - ctrl.t_delay + dt_sim, w['t'], w['z'][:, j]) for j in (3, 4)])
            err.append(np.abs((model.H @ xr)[3:5] - z_tgt).max())
    info = ctrl.save_controller_info()
    t_eval = 1e3 * np.array(t_eval)
    print('rompc closed loop: %d steps, %d solves, %d requests, evaluate median %.3f ms / max %.3f ms, tip error (x, y) median %.3f '
          '(target amplitude %.1f), observer error %.2e'
          % (args.steps, len(info['solve_times']), len(ctrl.requests), np.median(t_eval), t_eval.max(),
             np.median(err) if err else float('nan'), np.abs(w['z'][:, 3:5]).max(), np.abs(ctrl.observer.x - xr).max()))


if __name__ == '__main__':
    main()
