"""Continuous-time Riccati probe (csrc/care.hip): `care_batch` on 40 lightly damped second-order points at r = 30 (n_x = 60), n_u = 4
in one launch -- the `fem` family of tests/care_cases.py -- against the same 40 solves through scipy.linalg.solve_continuous_are on
the host of the same box (the only existing alternative), and `dare_batch` on the same points discretised (zero-order hold, dt =
0.01) as a sanity scale.  Wall time of the whole call (upload, one launch, synchronise, download): median over `--reps` repeats
after a warm-up.

What the Cayley start costs in doubling steps: both entry points are also timed with max_iter = 2 and 6, below their step counts
(they return SRH_ENUMERIC after exactly that many steps; only the download of K and P is then missing).  The slope is the time
of one doubling step, and (care - dare) at equal max_iter over that slope is the start's extra cost in steps.

    python tools/care_probe.py [--out profiles/care_probe.json]

Needs the GPU.  Every number is a measurement of this run; DESIGN.md quotes them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import care_cases as cc  # noqa: E402
from sofacontrol_amd import _lib  # noqa: E402
from sofacontrol_amd.lqr.lqr import _dare_call, care_batch, dare_batch  # noqa: E402

R_DIM, N_U, POINTS, DT = 30, 4, 40, 0.01


def med(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), n=int(len(v)))


def timed(fn, reps, warm):
    out = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= warm:
            out.append(1e3 * (t1 - t0))
    return med(out)


def capped(entry, A, B, Q, R, max_iter):
    try:
        _dare_call(entry, A, B, Q, R, 1e-14, max_iter)
    except _lib.HipError:
        return
    raise RuntimeError('%s converged within %d steps: the capped timing needs a smaller cap' % (entry, max_iter))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'care_probe.json'))
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warm', type=int, default=10)
    args = ap.parse_args()
    A, B, Q, R = cc.fem_case(R_DIM, N_U, members=POINTS)
    Ad = np.stack([scipy.linalg.expm(a * DT) for a in A])
    Bd = np.stack([np.linalg.solve(a, (ad - np.eye(2 * R_DIM)) @ b) for a, ad, b in zip(A, Ad, B)])

    Kc, Pc, itc = _dare_call('sric_care', A, B, Q, R, 1e-14, 100)
    Kd, Pd, itd = _dare_call('sric_dare', Ad, Bd, Q, R, 1e-14, 100)
    Ps = np.stack([scipy.linalg.solve_continuous_are(a, b, Q, R) for a, b in zip(A, B)])
    res = dict(shape=dict(n_x=2 * R_DIM, n_u=N_U, points=POINTS, dt_of_the_discrete_scale=DT),
               note='wall_ms: host clock around one call that ends in its one device synchronisation (upload, launch, download); '
                    'scipy_ms: the same 40 problems through scipy.linalg.solve_continuous_are on the host of the same box',
               care_steps=dict(min=int(itc.min()), max=int(itc.max())), dare_steps=dict(min=int(itd.min()), max=int(itd.max())),
               max_rel_diff_P_care_vs_scipy=float(np.abs(Pc - Ps).max() / np.abs(Ps).max()),
               max_real_part_closed_loop=float(max(np.linalg.eigvals(a + b @ k).real.max() for a, b, k in zip(A, B, Kc))),
               care_batch_wall_ms=timed(lambda: care_batch(A, B, Q, R), args.reps, args.warm),
               dare_batch_wall_ms=timed(lambda: dare_batch(Ad, Bd, Q, R), args.reps, args.warm),
               scipy_ms=timed(lambda: [scipy.linalg.solve_continuous_are(a, b, Q, R) for a, b in zip(A, B)], max(5, args.reps // 5), 1))
    res['scipy_over_care_batch'] = res['scipy_ms']['median'] / res['care_batch_wall_ms']['median']
    caps = {}
    for entry, (a, b) in (('sric_care', (A, B)), ('sric_dare', (Ad, Bd))):
        caps[entry] = {str(j): timed(lambda j=j: capped(entry, a, b, Q, R, j), args.reps, args.warm) for j in (2, 6)}
    step = (caps['sric_dare']['6']['median'] - caps['sric_dare']['2']['median']) / 4.0
    step_care = (caps['sric_care']['6']['median'] - caps['sric_care']['2']['median']) / 4.0
    res['capped_wall_ms'] = caps
    res['one_doubling_step_ms'] = dict(sric_dare=step, sric_care=step_care)
    res['cayley_start_in_doubling_steps'] = {j: (caps['sric_care'][j]['median'] - caps['sric_dare'][j]['median']) / step for j in ('2', '6')}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
