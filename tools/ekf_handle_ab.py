"""A/B of two builds of the library on the filter's host paths (csrc/observer.hip): the single-filter step and the fused step as
bench.py's closed_loop_latency measures them (ekf_step_us, fused_step_us: medians over its own repetitions) and contender (a) of
tools/ekf_batch_probe.py (sekf_batch_step, ms per step) at B = 1, 256, 4096.

    python tools/ekf_handle_ab.py --parent <library built from the parent commit> [--rounds 3] [--out profiles/ekf_handle_ab.json]

alternates parent, new, parent, new, ... (`new` is the in-tree library); every measurement runs in a fresh process (this script
with --measure, the library selected through SRH_LIB_PATH) and a failed one ends the run.  Per figure: the median over the rounds
of each build, and the parent's spread (largest minus smallest of its per-round medians); the new build passes when its median does
not exceed the parent's by more than that spread.  Needs the GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tools')]

BATCHES = (1, 256, 4096)
FIGURES = ['ekf_step_us', 'fused_step_us'] + ['batch_step_ms_B%d' % B for B in BATCHES]


def measure():
    import bench
    import ekf_batch_probe
    import workloads as wl
    from sofacontrol_amd import _lib
    from sofacontrol_amd.mor.pod import POD
    assert _lib.device_count() >= 1, 'no GPU visible'
    _lib.set_device(0)
    w = wl.diamond_c2()
    rom = POD(dict(U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    tp, _ = bench.build_model(w)
    cl = bench.closed_loop_latency(w, rom, tp)
    out = dict(ekf_step_us=cl['ekf_step_us'], fused_step_us=cl['fused_step_us'])
    model = ekf_batch_probe.build(w)
    for B in BATCHES:
        r = ekf_batch_probe.probe(B, model, handles=False)
        assert r['failed_filters'] == 0, r
        out['batch_step_ms_B%d' % B] = r['batched_ms_per_step']['median']
    print('EKF_HANDLE_AB ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--measure', action='store_true')
    ap.add_argument('--parent')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ekf_handle_ab.json'))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--measure'], env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in p.stdout.splitlines() if l.startswith('EKF_HANDLE_AB ')]
            if p.returncode != 0 or not line:          # nothing more is started on the GPU after a failed measurement
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit('ekf_handle_ab: the %s measurement of round %d ended with code %d' % (build, k, p.returncode))
            rounds[build].append(json.loads(line[-1][len('EKF_HANDLE_AB '):]))
            print('round %d %-6s %s' % (k, build, line[-1][len('EKF_HANDLE_AB '):]), flush=True)
    verdict = {}
    for f in FIGURES:
        pv, nv = [r[f] for r in rounds['parent']], [r[f] for r in rounds['new']]
        pm, nm, spread = float(np.median(pv)), float(np.median(nv)), max(pv) - min(pv)
        verdict[f] = dict(parent_median=pm, new_median=nm, parent_spread=spread, new_not_above_parent_by_more_than_its_spread=bool(nm <= pm + spread))
        print('%-22s parent %10.4f  new %10.4f  parent spread %8.4f  %s' % (f, pm, nm, spread, 'ok' if nm <= pm + spread else 'ABOVE'))
    res = dict(note='per round and build one fresh process: bench.closed_loop_latency (us, its own medians) and ekf_batch_probe contender (a) '
                    '(ms per sekf_batch_step, median of 20 after 3 warm-up); builds alternate parent, new within one run',
               rounds=rounds, figures=verdict)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
