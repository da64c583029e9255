"""The SSM controller and the TPWL controller side by side on ONE plant: the synthetic TPWL plant of the Diamond shape (n_x = 60, four
cables; the plant of the other diamond_* examples), which has ten times the states of the 6-state SSM model.

The SSM controller sees only the measured tip, y = C x + y_ref (velocity and position, n_y = 6).  The plant is excited first: E open-loop
episodes from seeded disturbed starts under seeded random inputs inside the U box, each held for five steps of 0.01 s, rolled out by the
batched plant rollout (TPWLATV.rollout).  SSM.sysid.fit_ssm fits a cubic SSM model with n_x = n_y = 6 from the tip records (y_ref = their
mean, chart = 'pca'; row i of the records holds the input applied after y_i).  Then both loops run on the same plant, the same seeds
(starts, target phases) and the same figure-8 target of the tip position:
  - SSMClosedLoopBatch.on_plant: plans on the fitted SSM model (N = 3, dt = 0.02, n_keep = 2: the hardware driver's shape), steps the
    TPWL plant, measures the tip and estimates x_hat = W_map(y - z_ref);
  - ClosedLoopBatch: plans on the plant's own TPWL model with perfect state feedback (N, dt, cost of workloads.diamond_c2, no gains).
Each controller's tracking error of the tip position (x, y) is printed: rms per loop, median over the loops.  No figure is promised.

    python examples/diamond_ssm_on_tpwl_closed_loop.py [--episodes 64] [--steps 400] [--batch 64] [--time 1.2] [--ridge 1e-8] [--seed 0]

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
sys.path.insert(0, os.path.join(ROOT, 'examples'))

from diamond_koopman_closed_loop_batch import DT_SIM, U0, diamond_plant   # noqa: E402

HOLD, U_LO, U_HI = 5, 200.0, 1500.0
N_SSM, DT_SSM, KEEP_SSM = 3, 0.02, 2
AMP, PERIOD = 15.0, 10.0


def excite(tp, Cm, y_ref, E, S, rng):
    """Records of E open-loop episodes of S simulation steps: Y (E, S + 1, 6), U (E, S + 1, m); row i holds the input applied after y_i
    (the last row's input is never used)."""
    m = tp.get_input_dim()
    held = rng.uniform(U_LO, U_HI, (E, -(-S // HOLD), m))
    u = np.repeat(held, HOLD, axis=1)[:, :S]
    x, _ = tp.rollout(0.5 * rng.standard_normal((E, tp.get_state_dim())), u, DT_SIM)
    return np.asarray(x) @ Cm.T + y_ref, np.concatenate([u, u[:, -1:]], axis=1)


def target_table():
    """t (T,), the figure-8 of the tip position (T, 2) around (0, 0), amplitude AMP (diamond_koopman.py:146-185)."""
    t = np.linspace(0.0, PERIOD, 1000)
    th = np.linspace(0.0, 2 * np.pi, 1000)
    return t, np.stack([-AMP * np.sin(th), AMP * np.sin(2 * th)], axis=1)


def tip_rms(tip, t_rows, phase, t, fig8):
    """rms over the rows (the first excluded) of |tip (x, y) - target| per loop."""
    want = np.stack([np.stack([np.interp(t_rows + ph, t, fig8[:, c]) for c in range(2)], axis=1) for ph in phase])
    err = np.linalg.norm(tip[:, 1:] - want[:, 1:], axis=2)
    return np.sqrt(np.mean(err ** 2, axis=1))


def ssm_loop(planner, tp, Cm, y_ref, x0, phase, t, fig8, periods):
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.utils import HyperRectangle
    B, n, m = x0.shape[0], planner.get_state_dim(), planner.get_input_dim()
    # the target in the shifted coordinates the solver takes: the output minus the planner's z_ref; the height is left where it rests
    zt = np.zeros((len(t), n))
    zt[:, 3:5] = fig8 - planner.z_ref[3:5]
    xp0 = planner.compute_RO_state(x0 @ Cm.T + y_ref)
    u_init = np.zeros((B, N_SSM, m))
    x_init, _ = planner.rollout(xp0, u_init, DT_SSM)
    Qz = np.zeros((n, n)); Qz[3, 3] = Qz[4, 4] = 100.0
    gu = GuSTO(SSMGuSTO(planner), N_SSM, DT_SSM, Qz, 1e-5 * np.eye(m), xp0, u_init, x_init, z=np.tile(zt[0], (B, N_SSM + 1, 1)),
               U=HyperRectangle([U_HI] * m, [U_LO] * m), verbose=0, max_gusto_iters=0, convg_thresh=1e-5, batch=B, first_solve_cap=1, max_trace=0)
    cl = SSMClosedLoopBatch.on_plant(gu, tp, DT_SIM, KEEP_SSM, t=t, z=zt, phase=phase, max_steps_per_run=periods * KEEP_SSM, C=Cm, y_ref=y_ref)
    cl.reset(x0, 0.0)
    t0 = time.perf_counter()
    r = cl.run(periods)
    return tip_rms(r.y[:, :, 3:5], r.t, phase, t, fig8), r, time.perf_counter() - t0, cl.stats()['waits_last_run']


def tpwl_loop(tp, w, y_ref, x0, phase, t, fig8, periods, n_keep):
    from scipy.interpolate import interp1d
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    from sofacontrol_amd.utils import HyperRectangle, Polyhedron
    B, m, N, dt = x0.shape[0], w['m'], w['N'], w['dt']
    gm = TPWLGuSTO(tp)
    with contextlib.redirect_stdout(io.StringIO()):
        gm.pre_discretize(dt)
    # the same target for z = H x: the tip position without y_ref
    zt = np.zeros((len(t), 6))
    zt[:, 3:5] = fig8 - y_ref[3:5]
    zi = interp1d(t, zt, axis=0, bounds_error=False, fill_value=(zt[0], zt[-1]))
    u_init = np.zeros((B, N, m))
    x_init, _ = gm.rollout(x0, u_init, dt)
    xc, fc = gm.get_characteristic_vals()
    gu = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=zi(phase[:, None] + dt * np.arange(N + 1)),
               U=HyperRectangle([U_HI] * m, [U_LO] * m), X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, max_gusto_iters=3,
               batch=B, first_solve_cap=1, max_trace=0)
    cl = ClosedLoopBatch(gu, tp, DT_SIM, n_keep, t=t, z=zt, phase=phase, max_steps_per_run=periods * n_keep)
    cl.reset(x0)
    t0 = time.perf_counter()
    r = cl.run(periods, record_x=False)
    return tip_rms(r.z[:, :, 3:5] + y_ref[3:5], r.t, phase, t, fig8), r, time.perf_counter() - t0, cl.stats()['waits_last_run']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--steps', type=int, default=400, help='simulation steps of 0.01 s per episode')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--time', type=float, default=1.2, help='seconds of closed loop')
    ap.add_argument('--ridge', type=float, default=1e-8)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    import workloads as wl
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    from sofacontrol_amd.SSM.sysid import fit_ssm, one_step_error
    E, S, B = args.episodes, args.steps, args.batch
    rng = np.random.default_rng(args.seed)
    w = wl.diamond_c2()
    tp, C3, y3 = diamond_plant()
    Cm = np.ascontiguousarray(w['H'])                                        # (6, 60): tip velocity and position
    y_ref = np.concatenate([np.zeros(3), y3])
    assert Cm.shape == (6, tp.get_state_dim()) and np.array_equal(Cm[3:6], C3)

    Y, U = excite(tp, Cm, y_ref, E, S, rng)
    assert np.isfinite(Y).all(), 'the open-loop episodes left the plant\'s range'
    Yv, Uv = excite(tp, Cm, y_ref, max(2, E // 8), S, rng)                   # held-out episodes
    y_eq = Y.reshape(-1, 6).mean(axis=0)
    t0 = time.perf_counter()
    model, params, fit = fit_ssm(Y, U, DT_SIM, 6, 3, 3, y_ref=y_eq, chart='pca', ridge=args.ridge)
    wall = time.perf_counter() - t0
    print('fit: %d episodes x %d rows, %d samples, ridge %g, %.1f ms (records from the host); one-step error of the discrete map: %.3e on the '
          'fit\'s records, %.3e on %d held-out episodes (output amplitude %.1f)'
          % (E, S + 1, fit.samples, fit.ridge, 1e3 * wall, one_step_error(model, Y, U, y_ref=y_eq), one_step_error(model, Yv, Uv, y_ref=y_eq),
             Yv.shape[0], np.abs(Y - y_eq).max()))
    planner = SSMDynamics(y_eq.copy(), discrete=False, discr_method='be', model=model, params=params)
    # what the one-step figure does not show: the open-loop output error over the planner's own horizon (N_SSM stages of DT_SSM), started
    # from the observer map as the planner starts, from every kept row of the held-out episodes (SSM.sysid.horizon_error)
    from sofacontrol_amd.SSM.sysid import horizon_error
    hz = horizon_error(planner, Yv, Uv, N_SSM, dt=DT_SSM, stride=int(round(DT_SSM / DT_SIM)))
    print('k-step output error rms_z of the planner at dt = %.2f on the held-out episodes: %s; %d windows, %d diverged'
          % (DT_SSM, ', '.join('k = %d: %.3e' % (k, hz.rms_z[k]) for k in sorted({0, 1, max(1, N_SSM // 2), N_SSM})), hz.windows, hz.diverged))

    t, fig8 = target_table()
    phase = rng.uniform(0.0, PERIOD / 2, B)
    x0 = 0.5 * rng.standard_normal((B, tp.get_state_dim()))
    p_ssm = max(1, int(round(args.time / (KEEP_SSM * DT_SIM))))
    n_keep = 10
    p_tpwl = max(1, int(round(args.time / (n_keep * DT_SIM))))
    for name, (rms, r, wall, waits), periods in (
            ('SSM controller (measured tip)', ssm_loop(planner, tp, Cm, y_ref, x0, phase, t, fig8, p_ssm), p_ssm),
            ('TPWL controller (full state)', tpwl_loop(tp, w, y_ref, x0, phase, t, fig8, p_tpwl, n_keep), p_tpwl)):
        print('%-30s %d loops x %d periods, %d host wait(s), %.2f ms per period: tip error (x, y) rms per loop: median %.3f, best %.3f, worst '
              '%.3f (target amplitude %.1f); inputs %.1f .. %.1f; solve status != 0: %d of %d'
              % (name, B, periods, waits, 1e3 * wall / periods, np.median(rms), rms.min(), rms.max(), AMP, r.u.min(), r.u.max(),
                 int((r.status != 0).sum()), r.status.size))
        if not (np.isfinite(r.u).all() and np.isfinite(rms).all()):
            print('  (this loop left the finite range: the figures above are what came out)')


if __name__ == '__main__':
    main()
