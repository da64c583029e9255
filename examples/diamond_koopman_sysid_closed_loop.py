"""Identify a Koopman model of the plant at hand on the device, then close the batched Koopman MPC loop with it.

The set-up is examples/diamond_koopman_closed_loop_batch.py's: the synthetic TPWL plant of the Diamond shape (n_x = 60, four cables, the
tip position measured), the reference driver's cost, U box and figure-8 target, Ts = 0.05 s on a simulation step of 0.01 s.  There the
loop runs on the shipped 66-observable model, which was identified on another robot.  Here the plant is excited first: E open-loop
episodes from seeded disturbed starts under seeded random inputs inside the U box, each held for one controller step (five simulation
steps), rolled out by the batched plant rollout (TPWLATV.rollout).  baselines.koopman.sysid.fit_koopman fits the model (66 observables of
degree 2, one delay) at Ts = 0.05 from the dt_sim = 0.01 records with stride = 5.

HOW THE ROWS ARE ARRANGED.  The loop's ring holds (y_k, the input applied BEFORE y_k), so the model is fitted on that layout, u_lag = 1:
row k of the records is (y_k, u_{k-1}) with y_k = C x_k + y_ref and x_{k+1} = f(x_k, u_k); row 0 carries the idle input that held the
plant before the episode.  With stride 5 the kept row 5 i holds y at t = i Ts and the input held over [(i - 1) Ts, i Ts).

The loop then runs twice on the same seeds (starts, noise, target phases): with the fitted model and with the shipped one, and the tip
errors are printed side by side.

    python examples/diamond_koopman_sysid_closed_loop.py [--episodes 64] [--steps 1000] [--batch 64] [--periods 40] [--ridge 1e-6] [--seed 0]

Needs an MI355X (no CPU fallback)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

from diamond_koopman_closed_loop_batch import N, DT_SIM, U0, diamond_problem, diamond_plant   # noqa: E402

STRIDE, U_LO, U_HI = 5, 200.0, 1500.0


def excite(tp, Cm, y_ref, E, S, rng):
    """Records of E open-loop episodes of S simulation steps in the u_lag = 1 layout: Y (E, S + 1, n_y), U (E, S + 1, m)."""
    m = tp.get_input_dim()
    held = rng.uniform(U_LO, U_HI, (E, S // STRIDE, m))
    u_sim = np.repeat(held, STRIDE, axis=1)                                  # (E, S, m): u_k applied over [k, k + 1) dt_sim
    x0 = 0.5 * rng.standard_normal((E, tp.get_state_dim()))
    x, _ = tp.rollout(x0, u_sim, DT_SIM)                                     # (E, S + 1, n_x)
    Y = np.asarray(x) @ Cm.T + y_ref
    U = np.concatenate([np.full((E, 1, m), U0), u_sim], axis=1)              # row k: the input applied before y_k
    return Y, U


def loop_problem(model):
    """Cost, U box and target of diamond_problem in the scaling of `model` (diamond_koopman.py:146-185)."""
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanScaling
    from sofacontrol_amd.tpwl.tpwl_utils import Target
    from sofacontrol_amd.utils import QuadraticCost, HyperRectangle
    scaling = KoopmanScaling(scale=model.scale)
    _, _, _, shipped_target, _, zf = diamond_problem()
    target = Target()
    target.t = shipped_target.t
    target.z = scaling.scale_down(y=zf)
    target.u = scaling.scale_down(u=np.zeros(model.m)).reshape(-1)
    cost = QuadraticCost()
    cost.R = .00001 * np.eye(model.m) * np.diag(scaling.u_factor[0])
    cost.Q = np.zeros((model.n, model.n))
    cost.Q[0, 0] = cost.Q[1, 1] = 100
    cost.Q *= np.diag(scaling.y_factor[0])
    U = HyperRectangle(ub=scaling.scale_down(u=U_HI * np.ones(model.m)).reshape(-1), lb=scaling.scale_down(u=U_LO * np.ones(model.m)).reshape(-1))
    return cost, target, U, zf


def closed_loop(model, tp, Cm, y_ref, B, P, phase, x0, V):
    """rms tip error (x, y) per loop, and the result, of P periods of the batched loop on `model`."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    cost, target, U, zf = loop_problem(model)
    loop = KoopmanClosedLoopBatch(model, N, cost, tp, Cm, y_ref, DT_SIM, 1, t=target.t, z=target.z, u=target.u, phase=phase, U=U,
                                  u0=np.full(model.m, U0), batch=B, max_steps_per_run=P * STRIDE)
    y_rest = x0 @ Cm.T + y_ref
    loop.reset(x0=x0, y_hist=y_rest[:, None, :], u_hist=np.full((B, 1, model.m), U0), u_prev0=np.full((B, model.m), U0))
    res = loop.run(P, V=V)
    want = np.stack([np.stack([np.interp(phase[b] + res.t, target.t, zf[:, j]) for j in (0, 1)], axis=1) for b in range(B)])
    err = np.linalg.norm(res.y[:, 1:, :2] - want[:, 1:], axis=2)
    return np.sqrt(np.mean(err ** 2, axis=1)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--steps', type=int, default=1000, help='simulation steps of 0.01 s per episode (a multiple of 5)')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--periods', type=int, default=40, help='controller steps of 0.05 s')
    ap.add_argument('--ridge', type=float, default=1e-6)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    from sofacontrol_amd.baselines.koopman.sysid import fit_koopman, one_step_error
    E, S, B, P = args.episodes, args.steps // STRIDE * STRIDE, args.batch, args.periods
    rng = np.random.default_rng(args.seed)
    shipped = diamond_problem()[0]
    tp, Cm, y_ref = diamond_plant()

    Y, U = excite(tp, Cm, y_ref, E, S, rng)
    assert np.isfinite(Y).all(), 'the open-loop episodes left the plant\'s range'
    Yv, Uv = excite(tp, Cm, y_ref, max(2, E // 8), S, rng)                   # held-out episodes
    t0 = time.perf_counter()
    model, fit = fit_koopman(Y, U, STRIDE * DT_SIM, obs_degree=2, delays=1, stride=STRIDE, u_lag=1, ridge=args.ridge)
    wall = time.perf_counter() - t0
    print('fit: %d episodes x %d rows kept, %d pairs, %d observables, ridge %g, %.1f ms (records from the host)'
          % (E, S // STRIDE + 1, fit.pairs, model.N, fit.ridge, 1e3 * wall))
    print('one-step residual rms per observable: %.3e on the fit\'s records (from the sums), %.3e on them and %.3e on %d held-out episodes '
          '(one_step_error)' % (fit.residual_rms, one_step_error(model, Y, U, stride=STRIDE, u_lag=1),
                                one_step_error(model, Yv, Uv, stride=STRIDE, u_lag=1), Yv.shape[0]))
    print('spectral radius of A: %.4f' % np.abs(np.linalg.eigvals(model.A_d)).max())

    phase = rng.uniform(0.0, 1.0, B)
    x0 = 0.5 * rng.standard_normal((B, tp.get_state_dim()))
    V = 0.05 * rng.standard_normal((P, STRIDE, B, 3))
    for name, mdl in (('fitted', model), ('shipped', shipped)):
        rms, res = closed_loop(mdl, tp, Cm, y_ref, B, P, phase, x0, V)
        codes, counts = np.unique(res.status, return_counts=True)
        print('%-7s model: tip error (x, y) rms per loop: median %.3f, best %.3f, worst %.3f (target amplitude 15.0); inputs %.1f .. %.1f; '
              'solve status %s' % (name, np.median(rms), rms.min(), rms.max(), res.u.min(), res.u.max(),
                                   ', '.join('%d: %d' % (int(c), k) for c, k in zip(codes, counts))))
        assert np.isfinite(res.y).all() and np.isfinite(res.u).all()


if __name__ == '__main__':
    main()
