"""What the measurement re-projection (Y=) costs inside the resident Koopman loop, and what it saves over driving the loop from the host:
B loops on the Diamond shape of tools/koopman_loop_probe.py (n_lift = 66, n_u = 4, n_y = 3, N = 5 at Ts = 0.05, r = 5 simulation steps of
0.01, rollout_horizon = 1, a TPWL plant of n_x = 60) for B in {1, 256, 4096}, Y the box of half-width --half around the tip at rest and a
measurement noise of --sigma, so that the reported share of the samples leaves Y.

Three loops over the same seeds, alternated period by period in one process:
  (1) KoopmanClosedLoopBatch(...).set_reproject(Y).run(1): the projection inside the advance kernel (csrc/koopman_loop.hip, <true> instantiation);
  (2) KoopmanClosedLoopBatch().run(1): the same loop without Y (the samples enter the ring as measured);
  (3) the route a user had before: one KoopmanSolverNode(batch=B).step per period and, per simulation step, one batched plant step in numpy,
      the noisy measurement, one batched `contains` and one `Polyhedron.project_to_polyhedron` of the samples outside, one push.
Per period: host clock around work that ends in the loop's own wait; warm-up periods first; median, min, max.  (1) over (2) is the cost of
the projection, (3) over (1) what the resident loop saves.  (1) and (3) see the same noise: their applied inputs are compared as they run.

    python tools/loop_reproject_probe.py [--out profiles/loop_reproject_probe.json] [--batches 1,256,4096] [--half 5] [--sigma 3]

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
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'examples'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import koopman_loop_probe as kp          # noqa: E402  (the shape, the host-driven loop and the statistics of the parent probe)


class HostLoopY(kp.HostLoop):
    """Loop (3): kp.HostLoop with measurement noise and the reference's two lines in front of every push."""

    def __init__(self, B, x0, y_hist, u_hist, u_prev0, Y):
        super().__init__(B, x0, y_hist, u_hist, u_prev0)
        self.Y, self.projected, self.samples = Y, 0, 0

    def clean(self, y):
        out = (y @ self.Y.A.T - self.Y.b).max(axis=1) > 0          # one batched `contains`
        if out.any():
            y = y.copy()
            y[out] = self.Y.project_to_polyhedron(y[out])
        self.projected += int(out.sum()); self.samples += len(y)
        return y

    def period(self, V):
        B = self.x.shape[0]
        _, xo, uo, _, st = self.node.step(self.k * kp.NK * kp.DT_SIM)
        bad = st != 0
        if bad.any() and self.xo is not None:
            xo[bad] = np.concatenate((self.xo[bad, 1:], self.xo[bad, -1:]), axis=1)
            uo[bad] = np.concatenate((self.uo[bad, 1:], self.uo[bad, -1:]), axis=1)
        self.xo, self.uo = xo, uo
        U = np.empty((B, kp.NK, uo.shape[2]))
        x = self.x
        for s in range(kp.NK):
            u = self.scaling.scale_up(u=uo[:, s // kp.R])
            A, Bm, d, _ = self.tp.linearize_batch(x, kp.DT_SIM)
            x = np.einsum('bij,bj->bi', A, x) + np.einsum('bij,bj->bi', Bm, u) + d
            self.node.push(self.clean((x @ self.C.T + self.y_ref) + V[s]), u)
            U[:, s] = u
        self.x = x
        self.k += 1
        return U


def probe(B, half, sigma, seed=0):
    from diamond_koopman_closed_loop_batch import diamond_koopman, tip_box, U0
    rng = np.random.default_rng(seed)
    Y = tip_box(half)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        with_y, model, scaling, tp, Cm, y_ref, zf, target = diamond_koopman(B, kp.NK, rollout_horizon=kp.RH, Y=Y)
        without = diamond_koopman(B, kp.NK, rollout_horizon=kp.RH)[0]
    x0 = 0.5 * rng.standard_normal((B, with_y.n_plant))
    y_hist = (x0 @ Cm.T + y_ref)[:, None, :]
    u_hist, u_prev0 = np.full((B, 1, model.m), U0), np.full((B, model.m), U0)
    for loop in (with_y, without):
        loop.reset(x0=x0, y_hist=y_hist, u_hist=u_hist, u_prev0=u_prev0)
    with quiet:
        host = HostLoopY(B, x0, y_hist, u_hist, u_prev0, Y)
    warm, timed = kp.periods_for(B)
    t1, t2, t3 = [], [], []
    words = {0: 0, 1: 0, -1: 0, -2: 0}
    u_rel = 0.0
    for k in range(warm + timed):
        V = sigma * rng.standard_normal((1, kp.NK, B, 3))
        order = (0, 1, 2) if k % 2 == 0 else (1, 0, 2)             # the two resident loops change sides
        dt = [0.0, 0.0, 0.0]
        for which in order:
            t0 = time.perf_counter()
            if which == 0:
                r = with_y.run(1, V=V)
            elif which == 1:
                without.run(1, V=V)
            else:
                with quiet:
                    Uh = host.period(V[0])
            dt[which] = 1e3 * (time.perf_counter() - t0)
        if k >= warm:
            t1.append(dt[0]); t2.append(dt[1]); t3.append(dt[2])
        for w, c in zip(*np.unique(r.proj[:, 1:], return_counts=True)):
            words[int(w)] += int(c)
        u_rel = max(u_rel, float(np.abs(r.u - Uh).max() / np.abs(Uh).max()))
    a, b, c = kp.stat(t1), kp.stat(t2), kp.stat(t3)
    n = sum(words.values())
    return dict(batch=B, warm_up_periods=warm, timed_periods=timed, share_projected=words[1] / n, status_words={str(k): v for k, v in words.items()},
                host_share_projected=host.projected / max(1, host.samples), u_rel_diff_resident_vs_host=u_rel,
                resident_with_Y_ms_per_period=a, resident_without_Y_ms_per_period=b, host_driven_with_Y_ms_per_period=c,
                with_Y_over_without=a['median'] / b['median'], host_over_resident_with_Y=c['median'] / a['median'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loop_reproject_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    ap.add_argument('--half', type=float, default=5.0)
    ap.add_argument('--sigma', type=float, default=3.0)
    args = ap.parse_args()
    res = dict(shape=dict(n_lift=66, n_u=4, n_y=3, N=kp.N, Ts=kp.TS, dt_sim=kp.DT_SIM, r=kp.R, rollout_horizon=kp.RH,
                          plant='a synthetic TPWL model of n_x = 60 at dt_sim', Y='box of half-width %g around the tip at rest, 6 rows' % args.half,
                          noise_sigma=args.sigma),
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the loops alternate period by period and the '
                    'two resident loops change sides every period; median, min, max over the timed periods',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(probe(B, args.half, args.sigma))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
