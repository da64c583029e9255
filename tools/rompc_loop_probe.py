"""Batched closed-loop ROMPC probe (csrc/rompc_loop.hip): B loops on the Diamond shape of examples/diamond_rompc_closed_loop_batch.py
(n_x = 60, n_u = 4, n_y = 30, N = 5 at dt_mpc = 0.05, n_replan = 10 at dt_sim = 0.01, the TPWL model as the plant) for B in {1, 256, 4096}.

Two kinds of loop over the same seeds, alternated period by period in one process:
  (a) ROMPCClosedLoopBatch.run(1): prepare -> solve -> chain -> advance on the device, the period's records copied back, one wait;
  (b) the same policy driven from the host with what the library offered before: one MPCSolverNode.mpc_callback per member per period,
      the chain in numpy, and per simulation step one batched observer.step (srompc_step) and one batched plant step (linearize_batch
      and the affine update in numpy).  (b) runs twice (b, b2): the difference of the two medians is the spread of the host figure.
The loops are compared as they run (applied inputs, plant states); the figure is reported, not judged.  Per period: host clock around
work that ends in the loop's own wait (every call of (b) is synchronous); warm-up periods first; median, min, max.  The host-driven side of
large batches takes seconds per period, so its period count shrinks with B (recorded).  Bytes across PCIe per period are computed from the
shapes.  The split of a period between solve, chain and advance needs a kernel trace of its own and is not measured here
(profiles/rompc_loop_kernel_stats_b256.csv: rocprofv3 --kernel-trace --stats of the example at 256 loops x 20 periods).

    python tools/rompc_loop_probe.py [--out profiles/rompc_loop_probe.json] [--batches 1,256,4096]

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

N, DT, NK, DT_SIM = 5, 0.05, 10, 0.01


def periods_for(B):
    """(warm-up, timed) periods: the host-driven side costs about B solves per period."""
    return (3, 20) if B <= 16 else ((2, 8) if B <= 512 else (1, 3))


class HostLoop:
    """Loop (b): the policy of the resident loop written against MPCSolverNode, DiscreteLuenbergerObserver.step and the TPWL model."""

    def __init__(self, loop, model, tp, w, x0, x_hat0, phase):
        from sofacontrol_amd.baselines.mpc import MPCSolverNode
        from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver
        from sofacontrol_amd.tpwl.tpwl_utils import Target
        from sofacontrol_amd.utils import QuadraticCost, HyperRectangle, Polyhedron
        from sofacontrol_amd.scp.closed_loop import schedule
        m = loop.n_u
        target = Target()
        target.t, target.z = w['t'], w['z']
        self.node = MPCSolverNode(loop.mpc_model, N, DT, QuadraticCost(Q=w['Qz'], R=1e-5 * np.eye(m)), target,
                                  U=HyperRectangle([1500.] * m, [0.] * m), X=Polyhedron(w['XA'], w['Xb']))
        self.ob = DiscreteLuenbergerObserver(model, None, None, batch=loop.B, L=loop.observer.L)
        self.ob.K = loop.observer.K
        self.ob.set_state(x_hat0)
        self.C, self.y_ref = np.asarray(model.C), np.ravel(model.y_ref)
        self.tp, self.phase = tp, phase
        self.x, self.x_req, self.k = x0.copy(), x_hat0.copy(), 0
        self.sc = schedule(N, DT, DT_SIM, NK, 0.0, 0)
        tau = NK * DT_SIM
        self.j_end = min(int(tau / DT), N - 1)
        self.th_end = (tau - self.j_end * DT) / DT

    def period(self):
        B = self.x.shape[0]
        t_p = self.k * NK * DT_SIM
        xo, uo = np.empty((B, N + 1, self.x.shape[1])), np.empty((B, N, self.node.model.B_d.shape[1]))
        for b in range(B):
            _, xo[b], uo[b], _, _ = self.node.mpc_callback(t_p + self.phase[b], self.x_req[b])
        xo[:, 0] = self.x_req
        self.x_req = xo[:, self.j_end] + self.th_end * (xo[:, self.j_end + 1] - xo[:, self.j_end])
        uext = np.concatenate((uo, uo[:, -1:]), axis=1)
        U = np.empty((B, NK, uo.shape[2]))
        x = self.x
        for s in range(NK):
            j, th = int(self.sc.j[s]), self.sc.theta[s]
            xbar = xo[:, j] + th * (xo[:, j + 1] - xo[:, j])
            ubar = uext[:, j] + th * (uext[:, j + 1] - uext[:, j])
            y = x @ self.C.T + self.y_ref
            u = np.reshape(self.ob.step(y, ubar=ubar, xbar=xbar), (B, -1))
            A, Bm, d, _ = self.tp.linearize_batch(x, DT_SIM)
            x = np.einsum('bij,bj->bi', A, x) + np.einsum('bij,bj->bi', Bm, u) + d
            U[:, s] = u
        self.x = x
        self.k += 1
        return U, x


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def bytes_per_period(B, n, m, ny, nz, nzq):
    D = 8
    resident = dict(up=0, down=B * (NK * (3 * n + nz + ny + 2 * m) + (3 * n + nz)) * D + B * (4 + 4 + D))
    solve_up = B * (N * (n * n + n * m + n) + n + 2 + (N + 1) * nzq) * D          # LOCP.update(full=True): the horizon goes up with every request
    solve_down = B * ((N + 1) * n + N * m + (N + 1) + 1) * D + B * 8
    step_up = B * ((ny + m + n) + n) * D                  # srompc_step (y, ubar, xbar), linearize_batch (x)
    step_down = B * ((m + n + nz) + (n * n + n * m + n)) * D + B * 4        # (u, x_hat, z), (A, B, d, idx)
    return dict(resident=resident, host_driven=dict(up=solve_up + NK * step_up, down=solve_down + NK * step_down))


def probe(B, seed=0):
    from diamond_rompc_closed_loop_batch import diamond_rompc
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0.0, 1.0, B)
    with contextlib.redirect_stdout(io.StringIO()):
        loop, model, tp, w = diamond_rompc(B, NK, phase=phase)
    n = loop.n_x
    x0 = 0.5 * rng.standard_normal((B, n))
    x_hat0 = x0 + 0.1 * rng.standard_normal((B, n))
    loop.reset(x0, x_hat0)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        hb, hb2 = HostLoop(loop, model, tp, w, x0, x_hat0, phase), HostLoop(loop, model, tp, w, x0, x_hat0, phase)
    warm, timed = periods_for(B)
    ta, tb, tb2 = [], [], []
    agree = dict(u_rel_diff=0.0, x_rel_diff=0.0, status_nonzero=0)
    for k in range(warm + timed):
        t0 = time.perf_counter()
        r = loop.run(1)
        t1 = time.perf_counter()
        with quiet:
            Ub, xb = hb.period()
        t2 = time.perf_counter()
        with quiet:
            hb2.period()
        t3 = time.perf_counter()
        if k >= warm:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tb2.append(1e3 * (t3 - t2))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Ub).max() / np.abs(Ub).max()))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(r.x[:, -1] - xb).max() / np.abs(xb).max()))
        agree['status_nonzero'] += int(np.count_nonzero(r.status))
    a, b, b2 = stat(ta), stat(tb), stat(tb2)
    return dict(batch=B, warm_up_periods=warm, timed_periods=timed, agreement=agree, resident_ms_per_period=a, host_driven_ms_per_period=b,
                host_driven_repeat_ms_per_period=b2, host_driven_spread_ms=abs(b['median'] - b2['median']),
                host_over_resident=b['median'] / a['median'], waits_per_run=loop.stats()['waits_last_run'],
                pcie_bytes_per_period=bytes_per_period(B, n, loop.n_u, loop.n_y, loop.n_zc, loop.n_z))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rompc_loop_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    args = ap.parse_args()
    res = dict(shape=dict(n_x=60, n_u=4, n_y=30, N=N, dt_mpc=DT, dt_sim=DT_SIM, n_replan=NK, plant='the TPWL model at dt_sim'),
               constants='read from global memory through L2 (no LDS variant was built)',
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the three loops alternate period by period; '
                    'the split of a period between solve, chain and advance is not measured here: it comes from a kernel trace of its own (profiles/rompc_loop_kernel_stats_b256.csv)',
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
