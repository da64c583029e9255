"""ROMPC baseline probe (csrc/rompc.hip, csrc/dare_wide.hip): the resident control step at (n_x, n_u, n_y, n_z) = (72, 4, 30, 6)
for batch 1 / 256 / 4096 -- device time (HIP events on the handle's stream, first copy in to last copy out) and wall time of
one `srompc_step` -- `replay` of T steps against T calls of `step`, `dare_wide` at (72, 30), and a numpy statement of the same
recursion timed on the same box.

    python tools/rompc_probe.py [--out profiles/rompc_probe.json]

Needs the GPU.  Every number is a measurement of this run; DESIGN.md quotes them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))

from sofacontrol_amd.baselines.rompc.observer import DiscreteLuenbergerObserver  # noqa: E402
from sofacontrol_amd.lqr.lqr import dare_wide  # noqa: E402

SHAPE = (72, 4, 30, 6)


class Sys:
    pass


def system(seed=0):
    n, m, ny, nz = SHAPE
    rng = np.random.default_rng(seed)
    s = Sys()
    s.A_d = 0.9 * np.linalg.qr(rng.standard_normal((n, n)))[0]
    s.B_d = rng.standard_normal((n, m)) / np.sqrt(m)
    s.d_d = 0.1 * rng.standard_normal(n)
    s.C = rng.standard_normal((ny, n)) / np.sqrt(n)
    s.y_ref = rng.standard_normal(ny)
    s.H = rng.standard_normal((nz, n)) / np.sqrt(n)
    s.z_ref = rng.standard_normal(nz)
    s.L = 0.3 * rng.standard_normal((n, ny)) / np.sqrt(ny)
    s.K = 0.3 * rng.standard_normal((m, n)) / np.sqrt(n)
    s.rom = None
    return s


def np_step(s, x, y, ubar, xbar):
    u = ubar + (x - xbar) @ s.K.T
    xn = x @ s.A_d.T + u @ s.B_d.T + s.d_d + ((y - s.y_ref) - x @ s.C.T) @ s.L.T
    return u, xn, xn @ s.H.T + s.z_ref


def med(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), n=int(len(v)))


def step_times(s, batch, reps, warm=20):
    n, m, ny, nz = SHAPE
    rng = np.random.default_rng(batch)
    ob = DiscreteLuenbergerObserver(s, None, None, batch=batch, L=s.L)
    ob.K = s.K
    x0 = rng.standard_normal((batch, n))
    ob.set_state(x0 if batch > 1 else x0[0])
    ob.set_timing(True)
    y, ub, xb = rng.standard_normal((batch, ny)), rng.standard_normal((batch, m)), rng.standard_normal((batch, n))
    wall, dev = [], []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        ob.step(y, ubar=ub, xbar=xb)
        t1 = time.perf_counter()
        if k >= warm:
            wall.append(1e3 * (t1 - t0)); dev.append(ob.stats()['device_ms'])
    x = x0
    host = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        _, x, _ = np_step(s, x, y, ub, xb)
        t1 = time.perf_counter()
        if k >= warm:
            host.append(1e3 * (t1 - t0))
    out = dict(batch=batch, wall_ms=med(wall), device_ms=med(dev), numpy_ms=med(host))
    out['numpy_over_wall'] = out['numpy_ms']['median'] / out['wall_ms']['median']
    return out


def replay_times(s, batch, T, reps):
    n, m, ny, nz = SHAPE
    rng = np.random.default_rng(100 + batch)
    Y, Ub, Xb = rng.standard_normal((T, batch, ny)), rng.standard_normal((T, batch, m)), rng.standard_normal((T, batch, n))
    x0 = rng.standard_normal((batch, n))
    ob = DiscreteLuenbergerObserver(s, None, None, batch=batch, L=s.L)
    ob.K = s.K
    ob.set_timing(True)
    rp_wall, rp_dev, st_wall = [], [], []
    for k in range(2 + reps):
        ob.set_state(x0)
        t0 = time.perf_counter()
        U, X, Z = ob.replay(Y, ubar=Ub, xbar=Xb)
        t1 = time.perf_counter()
        dev = ob.stats()['device_ms']
        ob.set_state(x0)
        t2 = time.perf_counter()
        for t in range(T):
            ob.step(Y[t], ubar=Ub[t], xbar=Xb[t])
        t3 = time.perf_counter()
        same = float(np.abs(X[-1] - ob.x).max())
        if k >= 2:
            rp_wall.append(1e3 * (t1 - t0)); rp_dev.append(dev); st_wall.append(1e3 * (t3 - t2))
    x = x0
    t0 = time.perf_counter()
    for t in range(T):
        _, x, _ = np_step(s, x, Y[t], Ub[t], Xb[t])
    host = 1e3 * (time.perf_counter() - t0)
    out = dict(batch=batch, T=T, replay_wall_ms=med(rp_wall), replay_kernel_ms=med(rp_dev), steps_wall_ms=med(st_wall), numpy_ms=host,
               max_abs_diff_replay_vs_steps=same, max_abs_diff_replay_vs_numpy=float(np.abs(X[-1] - x).max()))
    out['steps_over_replay'] = out['steps_wall_ms']['median'] / out['replay_wall_ms']['median']
    out['numpy_over_replay'] = host / out['replay_wall_ms']['median']
    return out


def dare_times(reps):
    import scipy.linalg as sl
    n, ny = SHAPE[0], SHAPE[2]
    rng = np.random.default_rng(5)
    V = rng.standard_normal((n, n))
    lam = 0.99 * rng.uniform(0.3, 1.0, n)
    A = np.real(V @ np.diag(lam) @ np.linalg.inv(V))
    Ct = rng.standard_normal((n, ny))
    Cq = rng.standard_normal((3, n))
    Q, R = Cq.T @ Cq, 1e-2 * np.eye(ny)
    dev, host = [], []
    for k in range(2 + reps):
        t0 = time.perf_counter()
        K, P = dare_wide(A, Ct, Q, R)
        t1 = time.perf_counter()
        Ps = sl.solve_discrete_are(A, Ct, Q, R)
        t2 = time.perf_counter()
        if k >= 2:
            dev.append(1e3 * (t1 - t0)); host.append(1e3 * (t2 - t1))
    return dict(n_x=n, n_u=ny, dare_wide_wall_ms=med(dev), scipy_ms=med(host), max_rel_diff_P=float(np.abs(P - Ps).max() / np.abs(Ps).max()),
                scipy_over_dare_wide=float(np.median(host) / np.median(dev)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rompc_probe.json'))
    ap.add_argument('--reps', type=int, default=300)
    args = ap.parse_args()
    s = system()
    res = dict(shape=dict(zip(('n_x', 'n_u', 'n_y', 'n_z'), SHAPE)),
               note='wall_ms: host clock around one srompc_step (ends in its one synchronisation); device_ms: HIP events on the '
                    'handle\'s stream from the first copy in to the last copy out; numpy_ms: the same recursion in numpy on the same box',
               step=[step_times(s, b, args.reps) for b in (1, 256, 4096)],
               replay=[replay_times(s, b, 50, 5) for b in (1, 256, 4096)],
               dare_wide=dare_times(5))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
