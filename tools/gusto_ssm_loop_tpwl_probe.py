"""Probe of the SSM closed loop on a TPWL plant (csrc/gusto_ssm_loop.hip: ssm_loop_advance_tpwl_kernel): B receding-horizon loops on the
hardware driver's shape (examples/hardware/diamond_SSM.py:353-361: planner n_x = 6, n_u = 4, cubic dynamics / quadratic maps, N = 3,
dt = 0.02, max_gusto_iters = 0), n_keep = 2 plant steps of dt_sim = 0.01 per period, on the synthetic Diamond TPWL plant (n_p = 60) measured
through a 6 x 60 map (n_o = 6), for B in {1, 256, 4096}.

Two loops over the same seeds, alternated period by period in one process:
  (a) SSMClosedLoopBatch.on_plant(...).run(1): prepare -> solve -> costs -> ONE advance launch on the device, the period's records copied
      back, one wait;
  (b) the same policy driven from the host: GuSTO.solve_batch, the shift in numpy, scipy's interp1d for the targets, then per sub-step one
      batched TPWL plant step (TPWLATV.rollout of one step), C x + y_ref in numpy and observed_to_reduced for the estimate: two host round
      trips per sub-step.  (b) runs twice (b, b2): the difference of the two medians is the spread.
The loops are compared as they run: iters / status equal, the applied inputs u within 1e-9 of their maximum; the figure is reported,
not widened.  Per period: host clock around work that ends in the loop's own wait; 3 warm-up + 20 timed periods; median, min, max.
Bytes across PCIe per period are computed from the shapes.  There is no target ratio.

    python tools/gusto_ssm_loop_tpwl_probe.py [--out profiles/gusto_ssm_loop_tpwl_probe.json] [--batches 1,256,4096]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gusto_ssm_loop_tpwl_probe.py --trace --batches 256 --out <dir>/trace_run.json
        (the kernel trace, in a run of its own: only loop (a), 3 + 20 periods)

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'examples')):
    sys.path.insert(0, p)

N_X, N_U, N_O, N, DT, N_KEEP, DT_SIM, WARM, TIMED = 6, 4, 6, 3, 0.02, 2, 0.01, 3, 20


def build(B, seed=0):
    """Planner model, the TPWL plant with C and y_ref, two GuSTO plans of B rollouts (one per loop kind), the target table, seeded initial
    plant states and phases."""
    import workloads as wl
    from scipy.interpolate import interp1d
    from oracle import ssm as ossm
    from test_ssm_gpu import product_ssm
    from diamond_koopman_closed_loop_batch import diamond_plant
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.ssm import SSMGuSTO
    from sofacontrol_amd.utils import HyperRectangle
    model = ossm.synthetic(N_X, N_U, 3, 2, seed=96)
    s = product_ssm(model, discr='be')
    tp, _, _ = diamond_plant()                              # pre-discretised at 0.01
    n_p = tp.get_state_dim()
    rng = np.random.default_rng(seed)
    xp0 = 0.5 * rng.standard_normal((B, n_p))
    # the tip's velocity and position rows, scaled into the range of the planner's outputs
    Cm = np.ascontiguousarray(wl.diamond_c2()['H'])
    Cm = Cm * (0.05 / np.abs(0.5 * np.random.default_rng(1).standard_normal((64, n_p)) @ Cm.T).max())
    y_ref = np.asarray(model['z_ref'], dtype=np.float64).copy()
    t = np.linspace(0.0, 2.0, 101)
    zt = np.zeros((101, N_X)); zt[:, 0] = 0.02 * np.sin(np.pi * t); zt[:, 1] = -0.01 * np.cos(np.pi * t); zt[:, 2] = 0.0075 * t
    zt = zt + ossm.observe(model, np.zeros(N_X))
    phase = rng.uniform(0.0, 1.0, B)
    zi = interp1d(t, zt, axis=0, bounds_error=False, fill_value=(zt[0], zt[-1]))
    x0 = np.zeros((B, N_X))
    u_init = np.zeros((B, N, N_U))
    x_init, _ = s.rollout(x0, u_init, DT)
    Qz = np.zeros((N_X, N_X)); Qz[0, 0] = Qz[1, 1] = Qz[2, 2] = 100.0

    def plan():
        return GuSTO(SSMGuSTO(s), N, DT, Qz, 1e-3 * np.eye(N_U), x0, u_init, x_init, z=zi(phase[:, None] + DT * np.arange(N + 1)),
                     U=HyperRectangle([3.0] * N_U, [-1.0] * N_U), verbose=0, convg_thresh=1e-5, max_gusto_iters=0, batch=B, first_solve_cap=1,
                     max_trace=0)
    return dict(s=s, tp=tp, C=Cm, y_ref=y_ref, n_p=n_p, plans=(plan(), plan()), xp0=xp0, phase=phase, t=t, zt=zt, zi=zi)


class HostLoop:
    """Loop (b): what a user of solve_batch, TPWLATV.rollout and W_map writes on the host."""

    def __init__(self, p, gusto):
        from sofacontrol_amd.scp.closed_loop import schedule
        self.p, self.gu, self.schedule = p, gusto, schedule
        s = p['s']
        self.x, self.k, self.xopt, self.uopt = p['xp0'].copy(), 0, None, None
        self.xhat = s.observed_to_reduced(((self.x @ p['C'].T + p['y_ref']) - s.z_ref).T).T

    def period(self):
        p, gu, s, tp = self.p, self.gu, self.p['s'], self.p['tp']
        B = self.x.shape[0]
        sc = self.schedule(N, DT, DT_SIM, N_KEEP, 0.0, self.k)
        x0 = self.xhat
        if self.k == 0:
            u_init = np.zeros((B, N, N_U))
            x_init, _ = s.rollout(x0, u_init, DT)
        else:
            x_init = self.xopt[:, np.minimum(np.arange(N + 1) + sc.idx0, N)]
            u_init = self.uopt[:, np.minimum(np.arange(N) + sc.idx0, N - 1)]
        z = p['zi']((sc.t_k + p['phase'])[:, None] + DT * np.arange(N + 1))
        xo, uo, _ = gu.solve_batch(x0, u_init, x_init, z=z)
        self.xopt, self.uopt = xo, uo
        uext = np.concatenate((uo, uo[:, -1:]), axis=1)
        U = np.empty((B, N_KEEP, N_U))
        x, xhat = self.x, self.xhat
        for q in range(N_KEEP):
            j, th = int(sc.j[q]), sc.theta[q]
            u = uext[:, j] + th * (uext[:, j + 1] - uext[:, j])
            X, _ = tp.rollout(x, np.ascontiguousarray(u[:, None, :]), DT_SIM)          # one batched plant step
            x = np.ascontiguousarray(np.asarray(X)[:, 1])
            y = x @ p['C'].T + p['y_ref']
            xhat = s.observed_to_reduced((y - s.z_ref).T).T
            U[:, q] = u
        self.x, self.xhat = x, xhat
        self.k += 1
        return U, x, xhat, gu.iters.copy(), gu.status.copy()


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def bytes_per_period(B, n_p):
    D, n, m, no = 8, N_X, N_U, N_O
    a = dict(up=0, down=B * ((N_KEEP + 1) * (n_p + n + 2 * no) + N_KEEP * m) * D + B * (4 + 4 + D))
    solve_up = B * (n + N * m + (N + 1) * n + (N + 1) * no) * D
    solve_down = B * ((N + 1) * n + N * m + (N + 1) * no) * D + B * 8
    step_up = B * ((n_p + m) + no) * D                   # rollout (x, u), observed_to_reduced (y)
    step_down = B * (2 * n_p + 2 * no + n) * D           # rollout (X of two rows, Z of two rows), x_hat
    return dict(resident=a, host_driven=dict(up=solve_up + N_KEEP * step_up, down=solve_down + N_KEEP * step_down))


def make_loop(p):
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    cl = SSMClosedLoopBatch.on_plant(p['plans'][0], p['tp'], DT_SIM, N_KEEP, t=p['t'], z=p['zt'], phase=p['phase'], max_steps_per_run=N_KEEP,
                                     C=p['C'], y_ref=p['y_ref'])
    cl.reset(p['xp0'])
    return cl


def probe(B):
    p = build(B)
    cl = make_loop(p)
    hb, hb2 = HostLoop(p, p['plans'][1]), HostLoop(p, p['plans'][1])
    ta, tb, tb2 = [], [], []
    agree = dict(iters_status_equal=True, u_rel_diff=0.0, x_rel_diff=0.0, x_hat_rel_diff=0.0)
    for k in range(WARM + TIMED):
        t0 = time.perf_counter()
        r = cl.run(1)
        t1 = time.perf_counter()
        Ub, xb, xhb, it, st = hb.period()
        t2 = time.perf_counter()
        hb2.period()
        t3 = time.perf_counter()
        if k >= WARM:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tb2.append(1e3 * (t3 - t2))
        agree['iters_status_equal'] &= bool(np.array_equal(r.iters[0], it) and np.array_equal(r.status[0], st))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Ub).max() / np.abs(Ub).max()))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(r.x[:, -1] - xb).max() / np.abs(xb).max()))
        agree['x_hat_rel_diff'] = max(agree['x_hat_rel_diff'], float(np.abs(r.x_hat[:, -1] - xhb).max() / np.abs(xhb).max()))
    agree['within_1e-9'] = bool(agree['iters_status_equal'] and agree['u_rel_diff'] <= 1e-9)
    a, b, b2 = stat(ta), stat(tb), stat(tb2)
    spread = abs(b['median'] - b2['median'])
    return dict(batch=B, agreement=agree, resident_ms_per_period=a, host_driven_ms_per_period=b, host_driven_repeat_ms_per_period=b2,
                host_driven_spread_ms=spread, waits_per_run=cl.stats()['waits_last_run'], pcie_bytes_per_period=bytes_per_period(B, p['n_p']))


def trace_run(B):
    """Loop (a) alone, for a kernel trace taken around this process."""
    cl = make_loop(build(B))
    for _ in range(WARM + TIMED):
        cl.run(1)
    return dict(batch=B, periods=WARM + TIMED, waits_per_run=cl.stats()['waits_last_run'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gusto_ssm_loop_tpwl_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    ap.add_argument('--trace', action='store_true', help='run only the resident loop (for rocprofv3 --kernel-trace --stats)')
    args = ap.parse_args()
    res = dict(shape=dict(n_x=N_X, n_u=N_U, rom_order=3, ssm_order=2, N=N, dt=DT, dt_sim=DT_SIM, n_keep=N_KEEP, n_o=N_O,
                          plant='the synthetic Diamond TPWL model (workloads.diamond_c2), n_p = 60, nearest point, zoh at dt_sim',
                          warm_up_periods=WARM, timed_periods=TIMED, max_gusto_iters=0),
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the three loops alternate period by '
                    'period; B = 1 is reported, not judged; the split of a period between prepare, solve and advance is in the kernel trace '
                    '(a run of its own), not in these figures',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(trace_run(B) if args.trace else probe(B))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
