"""Chained-policy probe (csrc/gusto_loop.hip: loop_chain_kernel): B receding-horizon loops on the C2 Diamond shape of
tools/gusto_loop_probe.py (workloads.diamond_c2: n_x = 60, n_u = 4, N = 50, dt = 0.05; n_keep = 10 plant steps of dt_sim = 0.01 per
period, per-point DARE gains), for B in {1, 256, 4096}.

Three loops over the same seeds, alternated period by period in one process:
  (a) ClosedLoopBatch(mpc=False, record_tape=True).run(1): the chained policy on the device, the period's records and tape copied back;
  (b) ClosedLoopBatch(mpc=True).run(1): the policy the loop had before, on the same build -- (a) is expected to cost (b) plus one small
      launch and the tape's bytes; nothing is judged, the figures are written down;
  (c) the chained policy driven from the host: tools/gusto_loop_probe.py's HostLoop (solve_batch, warm start and targets on the host,
      per sub-step one batched nearest-point call for the gains, one for the plant, the affine step in numpy) with the plans started
      from the previous plan at tau_end.  (c) runs twice (c, c2): the difference of the two medians is the spread.
(a) and (c) are the same policy: before timing is trusted they are compared -- iters / status equal, U within 1e-9 of its maximum (the
figure of tests/test_controllers_gpu.py for two routes to the same inputs); reported, not widened.
Per period: host clock around work that ends in the loop's own wait; 3 warm-up + 20 timed periods; median, min, max.
How a period splits between its kernels needs a kernel trace of its own; none is taken here.

    python tools/gusto_loop_chain_probe.py [--out profiles/gusto_loop_chain_probe.json] [--batches 1,256,4096]

Needs the GPU.  Every number is a measurement of this run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import gusto_loop_probe as base                                    # noqa: E402  (the shape, the model and the host-driven loop)

N_KEEP, DT_SIM, WARM, TIMED = base.N_KEEP, base.DT_SIM, base.WARM, base.TIMED


class ChainedHostLoop(base.HostLoop):
    """Loop (c): period k >= 1 plans from the previous plan at tau_end = n_keep dt_sim (tpwl/controllers.py:272), not from the plant."""

    def start_state(self):
        from sofacontrol_amd.scp.closed_loop import schedule_end
        if self.k == 0:
            return self.x
        j, th = schedule_end(self.w['N'], self.w['dt'], DT_SIM, N_KEEP)
        return self.xopt[:, j] + th * (self.xopt[:, j + 1] - self.xopt[:, j])


def probe(B, w):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    p = base.build(B, w)
    kw = dict(t=w['t'], z=w['z'], phase=p['phase'], K=p['K'], max_steps_per_run=N_KEEP)
    chained = ClosedLoopBatch(p['plans'][0], p['model'], DT_SIM, N_KEEP, mpc=False, record_tape=True, **kw)
    mpc = ClosedLoopBatch(p['plans'][0], p['model'], DT_SIM, N_KEEP, mpc=True, **kw)
    chained.reset(p['x0']); mpc.reset(p['x0'])
    hc, hc2 = ChainedHostLoop(p, p['plans'][1], w), ChainedHostLoop(p, p['plans'][1], w)
    ta, tb, tc, tc2 = [], [], [], []
    agree = dict(iters_status_equal=True, u_rel_diff=0.0, x_rel_diff=0.0)
    for k in range(WARM + TIMED):
        t0 = time.perf_counter()
        r = chained.run(1)
        t1 = time.perf_counter()
        mpc.run(1)
        t2 = time.perf_counter()
        Xc, Uc, Zc, it, st = hc.period()
        t3 = time.perf_counter()
        hc2.period()
        t4 = time.perf_counter()
        if k >= WARM:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tc.append(1e3 * (t3 - t2)); tc2.append(1e3 * (t4 - t3))
        agree['iters_status_equal'] &= bool(np.array_equal(r.iters[0], it) and np.array_equal(r.status[0], st))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Uc).max() / np.abs(Uc).max()))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(r.x[:, 1:] - Xc).max() / np.abs(Xc).max()))
    agree['within_1e-9'] = bool(agree['iters_status_equal'] and agree['u_rel_diff'] <= 1e-9)
    a, b, c, c2 = base.stat(ta), base.stat(tb), base.stat(tc), base.stat(tc2)
    n, m, nz = 2 * w['r'], w['m'], 6
    pcie = base.bytes_per_period(B, w['N'], n, m, nz)
    tape = B * (N_KEEP + 1) * (n + m) * 8
    return dict(batch=B, agreement_chained_device_vs_host=agree, chained_ms_per_period=a, mpc_true_ms_per_period=b,
                host_driven_chained_ms_per_period=c, host_driven_chained_repeat_ms_per_period=c2,
                host_driven_spread_ms=abs(c['median'] - c2['median']), chained_minus_mpc_true_median_ms=a['median'] - b['median'],
                waits_per_run=chained.stats()['waits_last_run'],
                pcie_bytes_per_period=dict(chained=dict(up=0, down=pcie['resident']['down'] + tape), mpc_true=pcie['resident'],
                                           host_driven=pcie['host_driven']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gusto_loop_chain_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    args = ap.parse_args()
    import workloads as wl
    w = wl.diamond_c2()
    res = dict(shape=dict(n_x=2 * w['r'], n_u=w['m'], N=w['N'], dt=w['dt'], dt_sim=DT_SIM, n_keep=N_KEEP, gains='DARE per point',
                          warm_up_periods=WARM, timed_periods=TIMED, max_gusto_iters=3),
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the four loops alternate period by '
                    'period; the chained period records its tape (x_bar, u_bar), the mpc=True period has none; no kernel trace was taken: '
                    'the split of a period between its kernels is not measured',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(probe(B, w))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
