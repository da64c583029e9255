"""Identify a TPWL model of the plant at hand on the device, then close the batched GuSTO loop with it on the true plant.

The set-up is examples/diamond_closed_loop_batch.py's: the synthetic TPWL plant of the Diamond shape (n_x = 60, four cables, P = 64
points), stepped at dt_sim = 0.01 s, the reference driver's cost, input box and figure-8 target, planning at dt = 0.05 s.  There the
planner is the plant's own model.  Here the plant is excited first: E open-loop episodes from seeded disturbed starts under seeded
random inputs inside the input box, each held for one planner step (five simulation steps), rolled out by the batched plant rollout
(TPWLATV.rollout).  tpwl.sysid.fit_tpwl fits the tables at Ts = 0.05 from the dt_sim = 0.01 records with stride = 5, so the fitted
model's forward-Euler step at Ts is the plant's five-step map.  The linearisation points come from --points: `plant`, the plant's own
(the default: a user knows where the robot was linearised); `kmeans`, the --kmeans K centroids of the kept states (points_from_records;
--kmeans K alone selects it too); `distance`, the reference's distance rule on the kept states (points_by_distance) with --threshold
(default: half the largest distance of a kept position from the mean kept position) -- every point is then a visited state, and their
number follows the spread of the records.  Points that received too few samples are dropped (on_fail='drop'): the open-loop episodes do
not visit every region.  For the chosen source the points, the points dropped, the one-step error and the tip error are printed; no
source is promised to beat another.

The one-step error of the fitted model is printed on the fit's records and on held-out episodes, and next to it the k-step output error
(tpwl.sysid.horizon_error: rms_z at k = 1, N / 2 and N of the planner's horizon, open loop from every kept row of the held-out episodes),
which is what the planner's rollouts meet; then B loops run on the true plant with the fitted planner, and the tip error is printed.

    python examples/diamond_tpwl_sysid_closed_loop.py [--episodes 128] [--steps 500] [--batch 16] [--periods 10] [--ridge 1e-8] [--points plant|kmeans|distance] [--kmeans 0] [--threshold T] [--seed 0]

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

STRIDE, DT_SIM, U_LO, U_HI = 5, 0.01, 0.0, 1500.0


def excite(tp, E, S, rng):
    """Records of E open-loop episodes of S simulation steps: X (E, S + 1, n_x), U (E, S + 1, m); row k holds the input applied after x_k
    (the last row's is never used)."""
    m = tp.get_input_dim()
    held = rng.uniform(U_LO, U_HI, (E, S // STRIDE, m))
    u_sim = np.repeat(held, STRIDE, axis=1)                                  # (E, S, m): u_k applied over [k, k + 1) dt_sim
    x0 = 0.5 * rng.standard_normal((E, tp.get_state_dim()))
    x, _ = tp.rollout(x0, u_sim, DT_SIM)                                     # (E, S + 1, n_x)
    return np.ascontiguousarray(x), np.concatenate([u_sim, u_sim[:, -1:]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=128)
    ap.add_argument('--steps', type=int, default=500, help='simulation steps of 0.01 s per episode (a multiple of 5)')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--periods', type=int, default=10, help='re-planning periods of 10 steps of 0.01 s')
    ap.add_argument('--ridge', type=float, default=1e-8)
    ap.add_argument('--kmeans', type=int, default=0, help='take K points from the records by k-means instead of the plant\'s own')
    ap.add_argument('--points', choices=('plant', 'kmeans', 'distance'), default=None, help='the source of the linearisation points (default: plant)')
    ap.add_argument('--threshold', type=float, default=None, help='--points distance: the threshold of the distance rule')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    source = args.points or ('kmeans' if args.kmeans else 'plant')
    if source == 'kmeans' and not args.kmeans:
        args.kmeans = 32

    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    from sofacontrol_amd.tpwl.sysid import fit_tpwl, horizon_error, one_step_error, points_by_distance, points_from_records
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import HyperRectangle

    w = wl.diamond_c2()
    n_f, r = w['U'].shape
    m, N, dt, n_keep, B = w['m'], w['N'], w['dt'], 10, args.batch
    E, S = args.episodes, args.steps // STRIDE * STRIDE
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()              # tip velocity + position
    rom_info = dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref'])
    weights = {'q': 1.0, 'v': 0.0}
    plant = TPWLATV(data=dict(w['tab'], rom_info=rom_info), params=dict(tpwl_method='nn', dist_weights=dict(weights)), Hf=Hf, discr_method='zoh')
    with contextlib.redirect_stdout(io.StringIO()):
        plant.pre_discretize(DT_SIM)

    rng = np.random.default_rng(args.seed)
    X, U = excite(plant, E, S, rng)
    assert np.isfinite(X).all(), 'the open-loop episodes left the plant\'s range'
    Xv, Uv = excite(plant, max(2, E // 8), S, rng)                           # held-out episodes
    if source == 'kmeans':
        with contextlib.redirect_stdout(io.StringIO()):
            q, v = points_from_records(X, args.kmeans, stride=STRIDE)
        print('points: %d k-means centroids of the kept states' % len(q))
    elif source == 'distance':
        thr = args.threshold
        if thr is None:
            qk = X[:, ::STRIDE, r:].reshape(-1, r)
            thr = 0.5 * float(np.linalg.norm(qk - qk.mean(axis=0), axis=1).max())
        t0 = time.perf_counter()
        sel = points_by_distance(X, weights, thr, stride=STRIDE)
        print('points: %r by the distance rule, threshold %.4g, %.1f ms (records from the host)%s'
              % (sel, thr, 1e3 * (time.perf_counter() - t0), '' if sel.complete else '; the cap of 1024 points was met: raise the threshold'))
        q, v = sel.q, sel.v
    else:
        q, v = np.asarray(w['tab']['q']), np.asarray(w['tab']['v'])
        print('points: the %d points of the plant\'s own table' % len(q))
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        model, fit = fit_tpwl(X, U, q, v, weights, STRIDE * DT_SIM, rom_info, stride=STRIDE, ridge=args.ridge, on_fail='drop', Hf=Hf)
    wall = time.perf_counter() - t0
    print('fit: %d episodes x %d rows kept, %d samples over %d points, %d points solved (%d with too few samples, %d with a failing pivot), '
          'ridge %g, %.1f ms (records from the host)' % (E, S // STRIDE + 1, fit.samples, len(fit.counts), int((fit.status == 0).sum()),
                                                         int((fit.status == 1).sum()), int((fit.status == 2).sum()), fit.ridge, 1e3 * wall))
    print('one-step residual rms per coordinate at Ts = %.2f: %.3e on the fit\'s records, %.3e on %d held-out episodes (worst sample %.3e)'
          % (STRIDE * DT_SIM, one_step_error(model, X, U, stride=STRIDE), one_step_error(model, Xv, Uv, stride=STRIDE), Xv.shape[0],
             one_step_error(model, Xv, Uv, stride=STRIDE, worst=True)))
    # the planner never uses the model for one step: its open-loop error over the planner's own horizon, from every kept row of the
    # held-out episodes (tpwl.sysid.horizon_error: the records are read on the device, the curve over k = 0 .. N comes back)
    t0 = time.perf_counter()
    hz = horizon_error(model, Xv, Uv, N, stride=STRIDE)
    ks = sorted({1, max(1, N // 2), N})
    print('k-step output error rms_z at Ts = %.2f on the held-out episodes, --points %s: %s; worst window at k = %d: %.3e (episode %d, row %d); '
          '%d windows, %d diverged, %.1f ms (records from the host)'
          % (STRIDE * DT_SIM, source, ', '.join('k = %d: %.3e' % (k, hz.rms_z[k]) for k in ks), N, hz.worst_z[N], hz.worst_z_at[N, 0],
             hz.worst_z_at[N, 1], hz.windows, hz.diverged, 1e3 * (time.perf_counter() - t0)))

    # the loop of examples/diamond_closed_loop_batch.py with the fitted planner on the true plant (no feedback gains: u = u_bar)
    gm = TPWLGuSTO(model)
    with contextlib.redirect_stdout(io.StringIO()):
        gm.pre_discretize(dt)
    x0 = 0.5 * rng.standard_normal((B, 2 * r))
    phase = rng.uniform(0.0, float(w['t'][-1]) / 2, B)
    u_init = np.zeros((B, N, m))
    x_init, _ = gm.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    xc, fc = gm.get_characteristic_vals()
    gusto = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=zi(phase[:, None] + dt * np.arange(N + 1)),
                  U=HyperRectangle([U_HI] * m, [U_LO] * m), x_char=xc, f_char=fc, convg_thresh=1e-3, max_gusto_iters=3, batch=B,
                  first_solve_cap=1, max_trace=0)
    loop = ClosedLoopBatch(gusto, plant, DT_SIM, n_keep, t=w['t'], z=w['z'], phase=phase, max_steps_per_run=args.periods * n_keep)
    loop.reset(x0)
    t0 = time.perf_counter()
    res = loop.run(args.periods, record_x=False)
    wall = time.perf_counter() - t0
    target = zi(phase[:, None] + res.t[None, :])
    err = np.linalg.norm((res.z - target)[:, 1:, 3:5], axis=2)
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    print('%d loops x %d periods on the true plant with the fitted planner, %.1f ms per period' % (B, args.periods, 1e3 * wall / args.periods))
    print('tip tracking rms (x, y) per loop: median %.3f, best %.3f, worst %.3f   (target amplitude %.1f)'
          % (np.median(rms), rms.min(), rms.max(), np.abs(w['z'][:, 3:5]).max()))
    names = {0: 'converged', 1: 'QP failed', 2: 'omega > omega_max', 3: 'max iterations'}
    codes, counts = np.unique(res.status, return_counts=True)
    print('solve status over %d solves: ' % res.status.size + ', '.join('%s %d' % (names.get(int(c), str(int(c))), k) for c, k in zip(codes, counts)))
    assert np.isfinite(res.z).all() and np.isfinite(res.u).all()


if __name__ == '__main__':
    main()
