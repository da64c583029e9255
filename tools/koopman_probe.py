"""Koopman baseline probe (csrc/koopman.hip): bulk embed + lift bandwidth, resident MPC step latency against the host path
(MPCSolver.solve on a host-side lift), batched step throughput, and a numpy restatement of the reference's per-sample loop.

    python tools/koopman_probe.py [--out profiles/koopman_probe.json]

Needs the GPU.  Every number is a measurement of this run; see DESIGN.md for what they are compared against."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))

from sofacontrol_amd import _lib  # noqa: E402
from sofacontrol_amd.baselines.koopman import koopman_utils as ku  # noqa: E402
from sofacontrol_amd.baselines import mpc as bmpc  # noqa: E402
from sofacontrol_amd.utils import Polyhedron  # noqa: E402


def shipped(g):
    model = {k: g['model_' + k] for k in ('A', 'B', 'C', 'M', 'K')}
    params = {'n': 3, 'm': 4, 'N': 66, 'nzeta': 10, 'delays': 1, 'obs_degree': 2, 'obs_type': 'poly', 'Ts': 0.05,
              'scale': {k: g['scale_' + k] for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor')}}
    return ku.KoopmanModel(model, params)


def event_ms(fn, reps):
    L = _lib.lib()
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.srh_event_create(C.byref(e0)); L.srh_event_create(C.byref(e1))
    fn(); _lib.sync()
    L.srh_event_record(e0, None)
    for _ in range(reps):
        fn()
    L.srh_event_record(e1, None)
    ms = C.c_float()
    _lib.check(L.srh_event_elapsed_ms(e0, e1, C.byref(ms)), 'elapsed')
    L.srh_event_destroy(e0); L.srh_event_destroy(e1)
    return ms.value / reps


def bulk(km, T, reps):
    rng = np.random.default_rng(0)
    y = _lib.DeviceBuffer.from_array(km.scaling.y_offset[0] + rng.standard_normal((T, 3)))
    u = _lib.DeviceBuffer.from_array(200 + 1300 * rng.random((T, 4)))
    out = {}
    for name, W in (('W_identity', None), ('W_dense_66x66', rng.standard_normal((66, 66)))):
        lf = ku.KoopmanLift(3, 4, 1, 2, y_offset=km.scaling.y_offset, y_factor=km.scaling.y_factor, u_offset=km.scaling.u_offset,
                            u_factor=km.scaling.u_factor, W=W)
        o = _lib.DeviceBuffer(8 * (T - 1) * lf.n_out)
        ms = event_ms(lambda: lf.embed_lift_dev(y.ptr, u.ptr, T, o.ptr), reps)
        nbytes = 8 * (T * 7 + (T - 1) * lf.n_out)
        out[name] = dict(T=T, ms=ms, bytes=nbytes, TBps=nbytes / ms / 1e9, frac_of_8TBps=nbytes / ms / 1e9 / 8.0)
    return out


def problem(g, km):
    class Cost:
        Q, R, Qf = g['cost_Q'], g['cost_R'], None

    class Target:
        t, z, u = g['cost_t'], g['cost_z'], g['cost_u']
    return Cost, Target, Polyhedron(g['cost_UA'], g['cost_Ub'])


def latency(g, km, steps):
    cost, target, U = problem(g, km)
    node = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U)
    ys, us = g['trace_y'], g['tr_1_0_u']
    node.push(ys[199], us[199])
    res, host = [], []
    for k in range(steps):
        y, u = ys[200 + k % 50], us[200 + k % 50]
        t = time.perf_counter()
        node.step(0.05 * (k % 50), y, u)
        res.append(time.perf_counter() - t)
    # host path: KoopmanData on the host, device lift_data, W @, MPCSolver.solve (horizon sent each time through LOCP.update)
    data = ku.KoopmanData(km.scale, km.delays)
    data.add_measurement(ys[199], us[199])
    x0 = km.W @ km.lift_data(*np.hstack([km.scaling.scale_down(y=ys[200])[0], km.scaling.scale_down(y=ys[199])[0],
                                         km.scaling.scale_down(u=us[199])[0]]))
    solver = bmpc.MPCSolver(km, 5, km.Ts, cost, x0, target, U=U)
    for k in range(steps):
        y, u = ys[200 + k % 50], us[200 + k % 50]
        t = time.perf_counter()
        data.add_measurement(y, u)
        x0 = km.W @ np.asarray(km.lift_data(*data.get_zeta()))
        solver.solve(0.05 * (k % 50), x0)
        host.append(time.perf_counter() - t)
        if len(data.y_norm) > 8:
            data.y_norm, data.u_norm = data.y_norm[-4:], data.u_norm[-4:]
    # where the step's time goes: device events around its parts (skoop_mpc_set_timing), one step at a time, next to the host
    # wall time of the same steps.  The QP part is slocp_plan_solve_dev_resident (no transpose after the first step).
    node.set_timing(True)
    parts, wall, waits = [], [], []
    for k in range(min(steps, 300)):
        y, u = ys[200 + k % 50], us[200 + k % 50]
        t = time.perf_counter()
        node.step(0.05 * (k % 50), y, u)
        wall.append(time.perf_counter() - t)
        st = node.stats()
        parts.append([st['pre_qp_ms'], st['qp_ms'], st['copy_back_ms'], st['device_ms']])
        waits.append(st['waits_last_step'])
    node.set_timing(False)
    parts = np.median(np.array(parts), axis=0)
    wall_ms = 1e3 * float(np.median(wall))
    q = lambda a: dict(median_ms=1e3 * float(np.median(a)), p99_ms=1e3 * float(np.percentile(a, 99)))
    return dict(resident_step=q(res), host_path=q(host),
                step_parts_device_ms=dict(push_targets_lift=float(parts[0]), qp=float(parts[1]), copy_back=float(parts[2]),
                                          device_total=float(parts[3])),
                step_wall_ms_with_timing=wall_ms, qp_share_of_step_wall=float(parts[1]) / wall_ms,
                qp_share_of_device_time=float(parts[1] / parts[3]),
                host_waits_per_step=dict(min=int(min(waits)), max=int(max(waits))))


def batches(g, km, sizes, reps):
    cost, target, U = problem(g, km)
    out = {}
    for B in sizes:
        node = bmpc.KoopmanSolverNode(km, 5, km.Ts, cost, target, U=U, batch=B)
        ys = np.tile(g['trace_y'][200], (B, 1)) + np.linspace(-0.5, 0.5, B)[:, None]
        us = np.tile(g['tr_1_0_u'][200], (B, 1))
        node.push(ys, us)
        node.step(0.0, ys, us)
        t = time.perf_counter()
        for k in range(reps):
            _, _, _, _, st = node.step(0.05 * k, ys, us)
        dt = (time.perf_counter() - t) / reps
        out['batch_%d' % B] = dict(step_ms=1e3 * dt, problems_per_s=B / dt, solved=int((st == 0).sum()))
    return out


def numpy_reference_loop(km, T):
    """The reference's per-sample work on one core: add_measurement (np.append), get_zeta, lambdified monomials, W @."""
    exps = ku.observable_exponents(10, 2)
    rng = np.random.default_rng(1)
    Y = km.scaling.y_offset[0] + rng.standard_normal((T, 3)); U = 200 + 1300 * rng.random((T, 4))
    data = ku.KoopmanData(km.scale, 1)
    t = time.perf_counter()
    for i in range(T):
        data.add_measurement(Y[i], U[i])
        z = data.get_zeta()
        if z is not None:
            psi = [np.prod(z ** e) for e in exps]
            km.W @ np.asarray(psi)
    dt = time.perf_counter() - t
    return dict(samples=T, us_per_sample=1e6 * dt / T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'koopman_probe.json'))
    ap.add_argument('--steps', type=int, default=1000)
    a = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g22_koopman.npz')))
    km = shipped(g)
    rec = dict(bulk=bulk(km, 10 ** 6, 20), latency=latency(g, km, a.steps), batches=batches(g, km, (256, 4096), 20),
               numpy_reference_loop=numpy_reference_loop(km, 20000))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
