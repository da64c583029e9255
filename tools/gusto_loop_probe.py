"""Batched closed-loop probe (csrc/gusto_loop.hip): B receding-horizon loops on the C2 Diamond shape (workloads.diamond_c2: n_x = 60,
n_u = 4, N = 50, dt = 0.05), n_keep = 10 plant steps of dt_sim = 0.01 per period, per-point DARE gains installed, for B in {1, 256, 4096}.

Two loops over the same seeds, alternated period by period in one process:
  (a) ClosedLoopBatch.run(1): prepare -> solve -> advance on the device, the period's records copied back, one wait;
  (b) the host-driven loop the public API offered before: GuSTO.solve_batch with GuSTOSolverNode._warm_start per rollout and
      scipy's interp1d for the targets, then per sub-step one batched nearest-point call for the gains, one for the plant, and the
      affine update in numpy (rows grouped by region).  (b) runs twice (b, b2): the difference of the two medians is the spread.
Before timing, the loops are checked against each other: iters / status equal, U within 1e-9 of its maximum
(tests/test_controllers_gpu.py:216 uses that figure for two routes to the same inputs); the figure is reported, not widened.
Per period: host clock around work that ends in the loop's own wait; 3 warm-up + 20 timed periods; median, min, max.
Bytes across PCIe per period are computed from the shapes.

    python tools/gusto_loop_probe.py [--out profiles/gusto_loop_probe.json] [--batches 1,256,4096]

Needs the GPU.  Every number is a measurement of this run; DESIGN.md section 25 quotes them."""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

N_KEEP, DT_SIM, WARM, TIMED = 10, 0.01, 3, 20


def build(B, w, seed=0):
    """Model, plant, two GuSTO plans of B rollouts (one per loop kind), gains, seeded initial states and phases."""
    from scipy.interpolate import interp1d
    from sofacontrol_amd.lqr.lqr import dare_batch
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.utils import HyperRectangle, Polyhedron
    n_f, r = w['U'].shape
    m, N, dt = w['m'], w['N'], w['dt']
    Hf = linearModel(nodes=[1354], num_nodes=n_f // 3).C.tocsr()
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, discr_method='zoh')
    gm = TPWLGuSTO(model)
    with contextlib.redirect_stdout(io.StringIO()):
        gm.pre_discretize(dt)
    tab = model.tpwl_dict
    Ad, Bd, dd = model.discretize_batch(np.stack(tab['A_c']), np.stack(tab['B_c']), np.stack(tab['d_c']), DT_SIM)
    model.handle_for(DT_SIM, tables=(Ad, Bd, dd))
    H = np.asarray(model.H)
    K, _ = dare_batch(Ad, Bd, H.T @ w['Qz'] @ H + 1e-3 * np.eye(2 * r), 1e-4 * np.eye(m))
    rng = np.random.default_rng(seed)
    x0 = 0.5 * rng.standard_normal((B, 2 * r))
    phase = rng.uniform(0.0, float(w['t'][-1]) / 2, B)
    u_init = np.zeros((B, N, m))
    x_init, _ = gm.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    xc, fc = gm.get_characteristic_vals()

    def plan():
        return GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=zi(phase[:, None] + dt * np.arange(N + 1)),
                     U=HyperRectangle([1500.] * m, [0.] * m), X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3,
                     max_gusto_iters=3, batch=B, first_solve_cap=1, max_trace=0)
    return dict(model=model, gm=gm, plans=(plan(), plan()), K=np.asarray(K), tables=(np.asarray(Ad), np.asarray(Bd), np.asarray(dd)),
                x0=x0, phase=phase, zi=zi, H=H)


class HostLoop:
    """Loop (b): what a user of solve_batch writes on the host."""

    def __init__(self, p, gusto, w):
        from sofacontrol_amd.scp.closed_loop import schedule
        from sofacontrol_amd.scp.standalone import GuSTOSolverNode
        self.p, self.gu, self.w, self.schedule, self.ws = p, gusto, w, schedule, GuSTOSolverNode._warm_start
        self.x, self.k, self.xopt, self.uopt = p['x0'].copy(), 0, None, None

    def start_state(self):
        """The states the period's plans start from: the plant's (mpc=True; tools/gusto_loop_chain_probe.py overrides it)."""
        return self.x

    def period(self):
        p, gu, N, dt = self.p, self.gu, self.w['N'], self.w['dt']
        B, m = self.x.shape[0], self.w['m']
        s = self.schedule(N, dt, DT_SIM, N_KEEP, 0.0, self.k)
        x_start = self.start_state()
        if self.k == 0:
            u_init = np.zeros((B, N, m))
            x_init, _ = p['gm'].rollout(self.x, u_init, dt)
        else:
            u_init, x_init = np.empty((B, N, m)), np.empty((B, N + 1, self.x.shape[1]))
            for b in range(B):
                node = types.SimpleNamespace(topt=np.arange(N + 1.0), xopt=self.xopt[b], uopt=self.uopt[b], N=N)
                u_init[b], x_init[b] = self.ws(node, float(s.idx0))
        z = p['zi']((s.t_k + p['phase'])[:, None] + dt * np.arange(N + 1))
        xo, uo, _ = gu.solve_batch(x_start, u_init, x_init, z=z)
        self.xopt, self.uopt = xo, uo
        uext = np.concatenate((uo, uo[:, -1:]), axis=1)
        Ad, Bd, dd = p['tables']
        X, U = np.empty((B, N_KEEP, self.x.shape[1])), np.empty((B, N_KEEP, m))
        x = self.x
        for q in range(N_KEEP):
            j, th = int(s.j[q]), s.theta[q]
            x_bar = xo[:, j] + th * (xo[:, j + 1] - xo[:, j])
            u = uext[:, j] + th * (uext[:, j + 1] - uext[:, j])
            near = np.atleast_1d(p['model'].calc_nearest_point(x_bar))
            dx = x - x_bar
            for i in np.unique(near):
                rows = near == i
                u[rows] += dx[rows] @ p['K'][i].T
            reg = np.atleast_1d(p['model'].calc_nearest_point(x))
            xn = np.empty_like(x)
            for i in np.unique(reg):
                rows = reg == i
                xn[rows] = x[rows] @ Ad[i].T + u[rows] @ Bd[i].T + dd[i]
            x = xn
            X[:, q], U[:, q] = x, u
        self.x = x
        self.k += 1
        return X, U, X @ p['H'].T, gu.iters.copy(), gu.status.copy()


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def bytes_per_period(B, N, n, m, nz):
    D = 8
    a = dict(up=0, down=B * N_KEEP * (n + nz + m) * D + B * (4 + 4 + D))
    solve_up = B * (n + N * m + (N + 1) * n + (N + 1) * nz) * D
    solve_down = B * ((N + 1) * n + N * m + (N + 1) * nz) * D + B * 8
    b = dict(up=solve_up + 2 * N_KEEP * B * n * D, down=solve_down + 2 * N_KEEP * B * 4)
    return dict(resident=a, host_driven=b)


def probe(B, w):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    p = build(B, w)
    cl = ClosedLoopBatch(p['plans'][0], p['model'], DT_SIM, N_KEEP, t=w['t'], z=w['z'], phase=p['phase'], K=p['K'],
                         max_steps_per_run=N_KEEP)
    cl.reset(p['x0'])
    hb, hb2 = HostLoop(p, p['plans'][1], w), HostLoop(p, p['plans'][1], w)
    ta, tb, tb2 = [], [], []
    agree = dict(iters_status_equal=True, u_rel_diff=0.0, x_rel_diff=0.0)
    for k in range(WARM + TIMED):
        t0 = time.perf_counter()
        r = cl.run(1)
        t1 = time.perf_counter()
        Xb, Ub, Zb, it, st = hb.period()
        t2 = time.perf_counter()
        hb2.period()
        t3 = time.perf_counter()
        if k >= WARM:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tb2.append(1e3 * (t3 - t2))
        agree['iters_status_equal'] &= bool(np.array_equal(r.iters[0], it) and np.array_equal(r.status[0], st))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Ub).max() / np.abs(Ub).max()))
        agree['x_rel_diff'] = max(agree['x_rel_diff'], float(np.abs(r.x[:, 1:] - Xb).max() / np.abs(Xb).max()))
    agree['within_1e-9'] = bool(agree['iters_status_equal'] and agree['u_rel_diff'] <= 1e-9)
    a, b, b2 = stat(ta), stat(tb), stat(tb2)
    spread = abs(b['median'] - b2['median'])
    n, m, nz = 2 * w['r'], w['m'], 6
    return dict(batch=B, agreement=agree, resident_ms_per_period=a, host_driven_ms_per_period=b, host_driven_repeat_ms_per_period=b2,
                host_driven_spread_ms=spread, resident_not_above_host_driven_by_more_than_the_spread=bool(a['median'] <= b['median'] + spread),
                waits_per_run=cl.stats()['waits_last_run'], pcie_bytes_per_period=bytes_per_period(B, w['N'], n, m, nz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gusto_loop_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    args = ap.parse_args()
    import workloads as wl
    w = wl.diamond_c2()
    res = dict(shape=dict(n_x=2 * w['r'], n_u=w['m'], N=w['N'], dt=w['dt'], dt_sim=DT_SIM, n_keep=N_KEEP, gains='DARE per point',
                          warm_up_periods=WARM, timed_periods=TIMED, max_gusto_iters=3),
               note='ms per period: host clock around one period that ends in the loop\'s own wait; the three loops alternate period by '
                    'period; B = 1 is reported, not judged',
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
