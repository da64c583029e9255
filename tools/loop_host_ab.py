"""A/B of two builds of the library on the host path of a closed-loop period (csrc/gusto_loop_host.h and the five units around it): the
median period of run(1) over 3 warm-up and 20 timed periods of
  - contender (a) of tools/gusto_ssm_loop_probe.py (SSMClosedLoopBatch, the hardware driver's shape) at B = 1, 256, 4096;
  - the unobserved and the observed TPWL loop of tools/gusto_loop_observer_probe.py (ClosedLoopBatch.run / run_observed) at B = 256;
  - the ROMPC loop of tools/rompc_loop_probe.py (ROMPCClosedLoopBatch.run, the Diamond shape with the TPWL model as the plant) at B = 256;
  - the Koopman loop of tools/koopman_loop_probe.py (KoopmanClosedLoopBatch.run, the Diamond shape) at B = 256;
  - the iLQR loop of tools/ilqr_loop_probe.py (ILQRClosedLoopBatch, state feedback and observed, the Diamond shape) at B = 256: it has no
    periods, so the timed call is one run(N) of the probe's N = 100 steps behind a reset, under the policy of one plan().

    python tools/loop_host_ab.py --parent <library built from the parent commit> [--rounds 5] [--out profiles/loop_host_ab.json]

alternates parent, new, parent, new, ... (`new` is the in-tree library); every measurement runs in a fresh process (this script with
--measure, the library selected through SRH_LIB_PATH) and a failed one ends the run.  Per figure: the median over the rounds of each
build and the parent's own spread over its rounds, smallest to largest; the new build passes when its median lies inside that spread
(below it is reported as such: faster is no failure).  Needs the GPU."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'examples')]

SSM_BATCHES, TPWL_BATCH, ROMPC_BATCH, KOOPMAN_BATCH, ILQR_BATCH, ILQR_STEPS = (1, 256, 4096), 256, 256, 256, 256, 100
FIGURES = ['ssm_period_ms_B%d' % B for B in SSM_BATCHES] + ['tpwl_period_ms_B%d' % TPWL_BATCH, 'tpwl_observed_period_ms_B%d' % TPWL_BATCH,
                                                                'rompc_period_ms_B%d' % ROMPC_BATCH, 'koopman_period_ms_B%d' % KOOPMAN_BATCH,
                                                                'ilqr_run%d_ms_B%d' % (ILQR_STEPS, ILQR_BATCH),
                                                                'ilqr_observed_run%d_ms_B%d' % (ILQR_STEPS, ILQR_BATCH)]


def median_period_ms(period, warm, timed):
    ts = []
    for k in range(warm + timed):
        t0 = time.perf_counter()
        period(k)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[warm:]))


def median_run_ms(loop, x0, x_hat0, steps, warm, timed):
    """The iLQR loop: run(steps) from the same state every time (the reset is outside the clock)."""
    ts = []
    for k in range(warm + timed):
        loop.reset(x0, x_hat0)
        t0 = time.perf_counter()
        loop.run(steps, record_x=x_hat0 is not None)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[warm:]))


def measure():
    import gusto_loop_observer_probe as op
    import gusto_ssm_loop_probe as sp
    import ilqr_loop_probe as ip
    import koopman_loop_probe as kp
    import rompc_loop_probe as rp
    import workloads as wl
    from diamond_koopman_closed_loop_batch import diamond_koopman, U0
    from diamond_rompc_closed_loop_batch import diamond_rompc
    from sofacontrol_amd import _lib
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    assert _lib.device_count() >= 1, 'no GPU visible'
    _lib.set_device(0)
    out = {}
    for B in SSM_BATCHES:
        p = sp.build(B)
        cl = SSMClosedLoopBatch(p['plans'][0], p['s'], sp.DT_SIM, sp.N_KEEP, t=p['t'], z=p['zt'], phase=p['phase'], max_steps_per_run=sp.N_KEEP)
        cl.reset(p['x0'])
        out['ssm_period_ms_B%d' % B] = median_period_ms(lambda k: cl.run(1), sp.WARM, sp.TIMED)
        assert cl.stats()['waits_last_run'] == 1
    w = wl.diamond_c2()
    p = op.build(TPWL_BATCH, w)
    co, kw = op.make_loops(p, w, TPWL_BATCH)
    cu = ClosedLoopBatch(p['plans'][1], p['model'], op.DT_SIM, op.N_KEEP, **kw)
    cu.reset(p['x0'])
    out['tpwl_period_ms_B%d' % TPWL_BATCH] = median_period_ms(lambda k: cu.run(1, record_x=False), op.WARM, op.TIMED)
    co.reset_observed(p['x0'], p['x_hat0'])
    out['tpwl_observed_period_ms_B%d' % TPWL_BATCH] = median_period_ms(lambda k: co.run_observed(1, V=p['V'][k:k + 1], record_x=False), op.WARM, op.TIMED)
    rng = np.random.default_rng(0)
    with contextlib.redirect_stdout(io.StringIO()):
        loop, _, _, _ = diamond_rompc(ROMPC_BATCH, rp.NK, phase=rng.uniform(0.0, 1.0, ROMPC_BATCH))
    x0 = 0.5 * rng.standard_normal((ROMPC_BATCH, loop.n_x))
    loop.reset(x0, x0 + 0.1 * rng.standard_normal(x0.shape))
    out['rompc_period_ms_B%d' % ROMPC_BATCH] = median_period_ms(lambda k: loop.run(1), op.WARM, op.TIMED)
    assert loop.stats()['waits_last_run'] == 1
    B = KOOPMAN_BATCH
    with contextlib.redirect_stdout(io.StringIO()):
        loop, model, _, _, Cm, y_ref, _, _ = diamond_koopman(B, kp.NK, rollout_horizon=kp.RH)
    x0 = 0.5 * rng.standard_normal((B, loop.n_plant))
    loop.reset(x0=x0, y_hist=(x0 @ Cm.T + y_ref)[:, None, :], u_hist=np.full((B, 1, model.m), U0), u_prev0=np.full((B, model.m), U0))
    out['koopman_period_ms_B%d' % B] = median_period_ms(lambda k: loop.run(1), op.WARM, op.TIMED)
    assert loop.stats()['waits_last_run'] == 1
    B, N = ILQR_BATCH, ILQR_STEPS
    for observed, key in ((False, 'ilqr_run%d_ms_B%d'), (True, 'ilqr_observed_run%d_ms_B%d')):
        model, policy, x0, x_hat0, z = ip.problem(B, N, observed)
        obs = DiscreteEKFObserverBatch(model, B, W=100.0 * np.eye(x0.shape[1]), V=np.eye(30)) if observed else None
        loop = ILQRClosedLoopBatch(policy, model, ip.DT, B, z=z, observer=obs, max_steps_per_run=N)
        loop.reset(x0, x_hat0)
        loop.plan()
        out[key % (N, B)] = median_run_ms(loop, x0, x_hat0, N, op.WARM, op.TIMED)
        assert loop.stats()['waits_last_run'] == 1
    print('LOOP_HOST_AB ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--measure', action='store_true')
    ap.add_argument('--parent')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loop_host_ab.json'))
    args = ap.parse_args()
    if args.measure:
        return measure()
    if not args.parent or not os.path.exists(args.parent):
        ap.error('--parent: the library built from the parent commit')
    rounds = {'parent': [], 'new': []}
    for k in range(args.rounds):
        for build in ('parent', 'new'):
            env = {key: v for key, v in os.environ.items() if key != 'SRH_LIB_PATH'}
            if build == 'parent':
                env['SRH_LIB_PATH'] = os.path.abspath(args.parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--measure'], env=env, capture_output=True, text=True, timeout=400)
            line = [l for l in p.stdout.splitlines() if l.startswith('LOOP_HOST_AB ')]
            if p.returncode != 0 or not line:          # nothing more is started on the GPU after a failed measurement
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit('loop_host_ab: the %s measurement of round %d ended with code %d' % (build, k, p.returncode))
            rounds[build].append(json.loads(line[-1][len('LOOP_HOST_AB '):]))
            print('round %d %-6s %s' % (k, build, line[-1][len('LOOP_HOST_AB '):]), flush=True)
    verdict = {}
    for f in FIGURES:
        pv, nv = [r[f] for r in rounds['parent']], [r[f] for r in rounds['new']]
        nm, lo, hi = float(np.median(nv)), min(pv), max(pv)
        where = 'inside' if lo <= nm <= hi else ('below by %.4f ms' % (lo - nm) if nm < lo else 'ABOVE by %.4f ms' % (nm - hi))
        verdict[f] = dict(parent_median=float(np.median(pv)), parent_min=lo, parent_max=hi, new_median=nm, new_median_against_the_parents_spread=where)
        print('%-32s parent %8.4f [%8.4f, %8.4f]  new %8.4f  %s' % (f, np.median(pv), lo, hi, nm, where))
    res = dict(note='per round and build one fresh process: ms per period, median of 20 timed run(1) after 3 warm-up (host clock around a '
                    'period that ends in the loop\'s own wait); builds alternate parent, new within one run',
               rounds=rounds, figures=verdict)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
