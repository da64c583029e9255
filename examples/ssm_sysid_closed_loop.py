"""Identify an SSM model of the plant at hand on the device, then close the batched SSM loop with it.

The plant is the reference's shipped Diamond SSM model (examples/hardware/SSMmodels/SSM_model.mat as kept in tests/golden/g17_ssm_hardware.npz:
n_x = 6, four cables, cubic), stepped in backward Euler at 0.01 s.  It is excited first: E open-loop episodes from seeded starts under
seeded random pressures, each held for `--hold` steps, rolled out by the batched model rollout (SSMDynamics.rollout).  SSM.sysid.fit_ssm
fits a model of the same shape from the records (y = the plant's six outputs, y_ref = the shipped equilibrium, chart = 'pca': with
n_y = n_x the chart is a rotation of the outputs).  Row i of the records holds the input applied after y_i.

The loop (SSMClosedLoopBatch: N = 3, n_keep = 2, the hardware driver's shape) then runs twice on the same seeds (starts, target phases):
with the fitted model as the planner and with the shipped one, the plant being the shipped model both times, and the errors of the two
tracked outputs are printed side by side.

    python examples/ssm_sysid_closed_loop.py [--episodes 64] [--steps 400] [--hold 20] [--batch 64] [--periods 100] [--ridge 0] [--seed 0]

Needs an MI355X (no CPU fallback)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))

DT, N, N_KEEP, U_LO, U_HI = 0.01, 3, 2, 0.0, 800.0


def _mat(v):
    a = np.empty((1, 1), dtype=object)
    a[0, 0] = np.asarray(v)
    return a


def shipped():
    """(model, params, z_eq) of the shipped Diamond SSM model in the loadmat layout."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g17_ssm_hardware.npz'))
    model = {k[len('model_'):]: _mat(g[k]) for k in g.files if k.startswith('model_')}
    params = {k[len('params_'):]: _mat(g[k]) for k in g.files if k.startswith('params_')}
    return model, params, g['z_eq'].copy()


def excite(plant, E, S, hold, rng):
    """Records of E open-loop episodes of S steps: Y (E, S + 1, n_y) with z_ref, U (E, S + 1, m); the last row's input is never used."""
    n, m = plant.get_state_dim(), plant.get_input_dim()
    held = rng.uniform(U_LO, U_HI, (E, -(-S // hold), m))
    u = np.repeat(held, hold, axis=1)[:, :S]
    x, z = plant.rollout(10.0 * rng.standard_normal((E, n)), u, DT)
    return np.asarray(z), np.concatenate([u, u[:, -1:]], axis=1)


def closed_loop(planner, plant, B, P, x0, t, zt, phase):
    """rms error of the two tracked outputs per loop, and the result, of P periods of the batched loop planned on `planner`."""
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.utils import HyperRectangle
    n, m = planner.get_state_dim(), planner.get_input_dim()
    # the planner's own coordinates of the plant's starts: x = W_map(y - z_ref) of the plant's output at rest
    z0 = plant.x_to_zfyf(x0)
    xp0 = planner.compute_RO_state(z0)
    u_init = np.zeros((B, N, m))
    x_init, _ = planner.rollout(xp0, u_init, DT)
    Qz = np.zeros((n, n)); Qz[0, 0] = Qz[1, 1] = 100.0
    gu = GuSTO(SSMGuSTO(planner), N, DT, Qz, 1e-5 * np.eye(m), xp0, u_init, x_init, z=np.tile(zt[0], (B, N + 1, 1)),
               U=HyperRectangle([U_HI] * m, [U_LO] * m), verbose=0, max_gusto_iters=0, convg_thresh=1e-5, batch=B, first_solve_cap=1, max_trace=0)
    cl = SSMClosedLoopBatch(gu, plant, DT, N_KEEP, t=t, z=zt, phase=phase, max_steps_per_run=P * N_KEEP)
    cl.reset(x0, 0.0)
    r = cl.run(P)
    want = np.stack([np.stack([np.interp(r.t + ph, t, zt[:, c]) for c in range(2)], axis=1) for ph in phase])
    err = np.linalg.norm(r.z[:, :, :2] - want, axis=2)
    return np.sqrt(np.mean(err[:, err.shape[1] // 2:] ** 2, axis=1)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--steps', type=int, default=400, help='steps of 0.01 s per episode')
    ap.add_argument('--hold', type=int, default=20, help='steps an excitation input is held')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--periods', type=int, default=100, help='replanning periods of 2 x 0.01 s')
    ap.add_argument('--ridge', type=float, default=0.0)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    from sofacontrol_amd.SSM.sysid import fit_ssm, one_step_error
    E, S, B, P = args.episodes, args.steps, args.batch, args.periods
    rng = np.random.default_rng(args.seed)
    smodel, sparams, z_eq = shipped()
    plant = SSMDynamics(z_eq.copy(), discrete=False, discr_method='be', model=smodel, params=sparams)
    n, m = plant.get_state_dim(), plant.get_input_dim()

    Y, U = excite(plant, E, S, args.hold, rng)
    assert np.isfinite(Y).all(), 'the open-loop episodes left the plant\'s range'
    Yv, Uv = excite(plant, max(2, E // 8), S, args.hold, rng)                # held-out episodes
    t0 = time.perf_counter()
    model, params, fit = fit_ssm(Y, U, DT, n, 3, 3, y_ref=z_eq, chart='pca', ridge=args.ridge)
    wall = time.perf_counter() - t0
    print('fit: %d episodes x %d rows, %d samples, n = %d regressors, ridge %g, %.1f ms (records from the host)'
          % (E, S + 1, fit.samples, model['rd_coeff'][0, 0].shape[1] + m, fit.ridge, 1e3 * wall))
    print('residual rms from the sums: discrete map %.3e, central difference %.3e, observation %.3e; one-step error of the discrete map '
          '(one_step_error): %.3e on the fit\'s records, %.3e on %d held-out episodes (output amplitude %.1f)'
          % (fit.residual_rms_d, fit.residual_rms_c, fit.residual_rms_w, one_step_error(model, Y, U, y_ref=z_eq),
             one_step_error(model, Yv, Uv, y_ref=z_eq), Yv.shape[0], np.abs(Y - z_eq).max()))

    fitted = SSMDynamics(z_eq.copy(), discrete=False, discr_method='be', model=model, params=params)
    # the planner never uses the model for one step: its open-loop output error over the planner's own horizon, started from the observer
    # map as the planner starts, from every kept row of the held-out episodes (SSM.sysid.horizon_error: the records are read on the device)
    from sofacontrol_amd.SSM.sysid import horizon_error
    for name, mdl in (('fitted', fitted), ('shipped', plant)):
        hz = horizon_error(mdl, Yv, Uv, N, dt=DT)
        print('%-7s model: k-step output error rms_z on the held-out episodes: %s; %d windows, %d diverged'
              % (name, ', '.join('k = %d: %.3e' % (k, hz.rms_z[k]) for k in sorted({0, 1, max(1, N // 2), N})), hz.windows, hz.diverged))
    t = np.linspace(0.0, 4.0, 201)                              # a slow circle of the first two outputs around the equilibrium
    zt = np.zeros((201, n)); zt[:, 0] = 5.0 * np.sin(0.5 * np.pi * t); zt[:, 1] = 5.0 * (1.0 - np.cos(0.5 * np.pi * t))
    phase = rng.uniform(0.0, 2.0, B)
    x0 = 1.0 * rng.standard_normal((B, n))
    for name, planner in (('fitted', fitted), ('shipped', plant)):
        rms, r = closed_loop(planner, plant, B, P, x0, t, zt, phase)
        print('%-7s model: error of the two tracked outputs, rms over the second half, per loop: median %.3f, best %.3f, worst %.3f (target '
              'amplitude 5.0); inputs %.1f .. %.1f; status != 0: %d' % (name, np.median(rms), rms.min(), rms.max(), r.u.min(), r.u.max(),
                                                                         int((r.status != 0).sum())))
        assert np.isfinite(r.z).all() and np.isfinite(r.u).all()


if __name__ == '__main__':
    main()
