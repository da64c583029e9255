"""Batched closed-loop Koopman MPC probe (csrc/koopman_loop.hip): B loops on the Diamond shape of
examples/diamond_koopman_closed_loop_batch.py (n_lift = 66, n_u = 4, n_y = 3, N = 5 at Ts = 0.05, r = 5 simulation steps of 0.01 per
controller step, rollout_horizon = 1, a TPWL plant of n_x = 60) for B in {1, 256, 4096}.

Two kinds of loop over the same seeds, alternated period by period in one process:
  (a) KoopmanClosedLoopBatch.run(1): prepare -> lift -> solve -> fix-up -> advance on the device, the period's records copied back, one wait;
  (b) the same policy driven from the host with what the library offered before: one KoopmanSolverNode(batch=B).step per period (lift and
      QP on the device, the plan copied back), and per simulation step one batched plant step (linearize_batch and the affine update in
      numpy), the measurement in numpy and one push into the node's device ring.  (b) runs twice (b, b2): the difference of the two
      medians is the spread of the host figure.
The loops are compared as they run (applied inputs, plant states); the figure is reported, not judged.  Per period: host clock around
work that ends in the loop's own wait (the step of (b) ends in its wait; its pushes are asynchronous and are waited for by the next
step, inside the timed interval of the next period); warm-up periods first; median, min, max.  Bytes across PCIe per period are computed
from the shapes.  The split of a period between lift, solve, fix-up and advance needs a kernel trace of its own and is not measured here.

    python tools/koopman_loop_probe.py [--out profiles/koopman_loop_probe.json] [--batches 1,256,4096]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'examples')):
    sys.path.insert(0, p)

N, TS, R, RH, DT_SIM = 5, 0.05, 5, 1, 0.01
NK = R * RH


def periods_for(B):
    """(warm-up, timed) periods: the host-driven side steps a batched plant in numpy five times per period."""
    return (3, 30) if B <= 16 else ((3, 20) if B <= 512 else (2, 8))


class HostLoop:
    """Loop (b): the policy of the resident loop written against KoopmanSolverNode(batch=B) and the TPWL model."""

    def __init__(self, B, x0, y_hist, u_hist, u_prev0):
        from diamond_koopman_closed_loop_batch import diamond_problem, diamond_plant
        from sofacontrol_amd.baselines.mpc import KoopmanSolverNode
        model, self.scaling, cost, target, U, _ = diamond_problem()
        self.tp, self.C, self.y_ref = diamond_plant()
        self.node = KoopmanSolverNode(model, N, TS, cost, target, U=U, batch=B)
        self.x, self.k = x0.copy(), 0
        self.xo = self.uo = None
        self.node.push(y_hist[:, 0], u_hist[:, 0])
        self.node.push(x0 @ self.C.T + self.y_ref, u_prev0)

    def period(self):
        B = self.x.shape[0]
        _, xo, uo, _, st = self.node.step(self.k * NK * DT_SIM)
        bad = st != 0
        if bad.any() and self.xo is not None:             # baselines/ros.py:223-227
            xo[bad] = np.concatenate((self.xo[bad, 1:], self.xo[bad, -1:]), axis=1)
            uo[bad] = np.concatenate((self.uo[bad, 1:], self.uo[bad, -1:]), axis=1)
        self.xo, self.uo = xo, uo
        U = np.empty((B, NK, uo.shape[2]))
        x = self.x
        for s in range(NK):
            u = self.scaling.scale_up(u=uo[:, s // R])
            A, Bm, d, _ = self.tp.linearize_batch(x, DT_SIM)
            x = np.einsum('bij,bj->bi', A, x) + np.einsum('bij,bj->bi', Bm, u) + d
            self.node.push(x @ self.C.T + self.y_ref, u)
            U[:, s] = u
        self.x = x
        self.k += 1
        return U, x, int(np.count_nonzero(bad))


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def bytes_per_period(B, n, m, ny, npl):
    D = 8
    resident = dict(up=0, down=B * (NK * (npl + ny + m) + n) * D + B * (4 + 4 + D))
    step_up = B * ((N + 1) * ny + N * m) * D                       # skoop_mpc_step: the target window and u_des of every member
    step_down = B * (n + (N + 1) * n + N * m + 1) * D + B * 4
    sub_up = B * (ny + m) * D + B * npl * D                        # skoop_push (y, u), linearize_batch (x)
    sub_down = B * (npl * npl + npl * m + npl) * D + B * 4         # (A, B, d, idx)
    return dict(resident=resident, host_driven=dict(up=step_up + NK * sub_up, down=step_down + NK * sub_down))


def probe(B, seed=0):
    from diamond_koopman_closed_loop_batch import diamond_koopman, U0
    rng = np.random.default_rng(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        loop, model, scaling, tp, Cm, y_ref, zf, target = diamond_koopman(B, NK, rollout_horizon=RH)
    x0 = 0.5 * rng.standard_normal((B, loop.n_plant))
    y_hist = (x0 @ Cm.T + y_ref)[:, None, :]
    u_hist, u_prev0 = np.full((B, 1, model.m), U0), np.full((B, model.m), U0)
    loop.reset(x0=x0, y_hist=y_hist, u_hist=u_hist, u_prev0=u_prev0)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        hb, hb2 = HostLoop(B, x0, y_hist, u_hist, u_prev0), HostLoop(B, x0, y_hist, u_hist, u_prev0)
    warm, timed = periods_for(B)
    ta, tb, tb2 = [], [], []
    agree = dict(u_rel_diff=0.0, x_rel_diff=0.0, status_nonzero=0, host_status_nonzero=0)
    for k in range(warm + timed):
        t0 = time.perf_counter()
        r = loop.run(1)
        t1 = time.perf_counter()
        with quiet:
            Ub, xb, nb = hb.period()
        t2 = time.perf_counter()
        with quiet:
            hb2.period()
        t3 = time.perf_counter()
        if k >= warm:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tb2.append(1e3 * (t3 - t2))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Ub).max() / np.abs(Ub).max()))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(r.x[:, -1] - xb).max() / np.abs(xb).max()))
        agree['status_nonzero'] += int(np.count_nonzero(r.status)); agree['host_status_nonzero'] += nb
    a, b, b2 = stat(ta), stat(tb), stat(tb2)
    return dict(batch=B, warm_up_periods=warm, timed_periods=timed, agreement=agree, resident_ms_per_period=a, host_driven_ms_per_period=b,
                host_driven_repeat_ms_per_period=b2, host_driven_spread_ms=abs(b['median'] - b2['median']),
                host_over_resident=b['median'] / a['median'], waits_per_run=loop.stats()['waits_last_run'],
                pcie_bytes_per_period=bytes_per_period(B, loop.n_x, loop.n_u, loop.n_y, loop.n_plant))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'koopman_loop_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    args = ap.parse_args()
    res = dict(shape=dict(n_lift=66, n_u=4, n_y=3, N=N, Ts=TS, dt_sim=DT_SIM, r=R, rollout_horizon=RH, plant='a synthetic TPWL model of n_x = 60 at dt_sim'),
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the three loops alternate period by period; '
                    'the split of a period between lift, solve, fix-up and advance is not measured here: it needs a kernel trace of its own',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(probe(B))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
