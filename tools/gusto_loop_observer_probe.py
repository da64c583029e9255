"""Observed closed-loop probe (csrc/gusto_loop.hip with the batched filter of csrc/observer.hip inside): the setting of
tools/gusto_loop_probe.py -- C2 Diamond shape (n_x = 60, n_u = 4, N = 50, dt = 0.05), n_keep = 10 plant steps of dt_sim = 0.01 per period,
per-point DARE gains, max_gusto_iters = 3 -- with five measured nodes (n_y = 30), W = 100 I, V = I, measurement noise and a wrong initial
estimate.  Three measurements, every contender alternating with its rival step by step / period by period in one process, 3 warm-up + 20
timed (host clock around work that ends in the call's own wait; median, min, max):

  1. the batched filter alone (tools/ekf_batch_probe.py): sekf_batch_step against B one-filter handles stepped in turn, B = 1, 256, 4096;
  2. the observed loop, B = 1 and 256: (a) ClosedLoopBatch.run_observed(1) against (b) the host-driven statement on the earlier API --
     solve_batch from the estimates, the numpy advance of tools/gusto_loop_probe.py under the law at the estimate, y = C x + y_ref + v in
     numpy and B one-filter observers (sekf_step) per sub-step.  (b) runs twice (b, b2): the difference of the two medians is the spread;
  3. what the observer costs, B = 256 and 4096: the observed resident loop against the unobserved one (ClosedLoopBatch.run(1)).

Acceptance (1 and 2, at B = 256): the new path's median is not above the baseline's by more than the baseline's spread.
Bytes across PCIe per period are computed from the shapes.

    python tools/gusto_loop_observer_probe.py [--out profiles/gusto_loop_observer_probe.json]

Needs the GPU.  Every number is a measurement of this run; DESIGN.md section 26 quotes them."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import ekf_batch_probe as fp          # noqa: E402
import gusto_loop_probe as lp         # noqa: E402

N_KEEP, DT_SIM, WARM, TIMED, N_Y = lp.N_KEEP, lp.DT_SIM, lp.WARM, lp.TIMED, 30


def build(B, w):
    """tools/gusto_loop_probe.build plus the measurement model, the noise and the wrong initial estimates."""
    from sofacontrol_amd.measurement_models import linearModel
    p = lp.build(B, w)
    n_f = w['U'].shape[0]
    p['model'].set_measurement_model(linearModel(nodes=fp.NODES, num_nodes=n_f // 3).C.tocsr())
    rng = np.random.default_rng(1)
    p['x_hat0'] = p['x0'] + 0.1 * rng.standard_normal(p['x0'].shape)
    p['V'] = 0.05 * rng.standard_normal((WARM + TIMED, N_KEEP, B, N_Y))
    p['W'], p['Vc'] = 100.0 * np.eye(p['x0'].shape[1]), np.eye(N_Y)
    return p


class ObservedHostLoop(lp.HostLoop):
    """Loop (b): tools/gusto_loop_probe.HostLoop with B one-filter observers, plans and law at the estimates."""

    def __init__(self, p, gusto, w):
        super().__init__(p, gusto, w)
        from sofacontrol_amd import _lib
        self.lib = _lib
        lib, f64, dptr = _lib.lib(), _lib.f64, _lib.dptr
        model = p['model']
        self.Cm, self.yr = f64(model.C), f64(model.y_ref)
        mh = model.handle_for(DT_SIM)
        self.hs = []
        for b in range(self.x.shape[0]):
            h = C.c_void_p()
            _lib.check(lib.sekf_create(C.byref(h), mh, dptr(self.Cm), dptr(self.yr), C.c_int(N_Y), dptr(np.eye(self.x.shape[1])), dptr(p['W']),
                                       dptr(p['Vc'])), 'sekf_create')
            _lib.check(lib.sekf_set_state(h, dptr(f64(p['x_hat0'][b])), None), 'sekf_set_state')
            self.hs.append(h)
        self.xh = p['x_hat0'].copy()

    def close(self):
        for h in self.hs:
            self.lib.lib().sekf_destroy(h)

    def period(self):
        p, gu, N, dt = self.p, self.gu, self.w['N'], self.w['dt']
        lib, dptr = self.lib.lib(), self.lib.dptr
        B, m = self.x.shape[0], self.w['m']
        s = self.schedule(N, dt, DT_SIM, N_KEEP, 0.0, self.k)
        if self.k == 0:
            u_init = np.zeros((B, N, m))
            x_init, _ = p['gm'].rollout(self.xh, u_init, dt)
        else:
            u_init, x_init = np.empty((B, N, m)), np.empty((B, N + 1, self.x.shape[1]))
            for b in range(B):
                node = types.SimpleNamespace(topt=np.arange(N + 1.0), xopt=self.xopt[b], uopt=self.uopt[b], N=N)
                u_init[b], x_init[b] = self.ws(node, float(s.idx0))
        z = p['zi']((s.t_k + p['phase'])[:, None] + dt * np.arange(N + 1))
        xo, uo, _ = gu.solve_batch(self.xh, u_init, x_init, z=z)
        self.xopt, self.uopt = xo, uo
        uext = np.concatenate((uo, uo[:, -1:]), axis=1)
        Ad, Bd, dd = p['tables']
        U = np.empty((B, N_KEEP, m))
        x, xh = self.x, self.xh
        for q in range(N_KEEP):
            j, th = int(s.j[q]), s.theta[q]
            x_bar = xo[:, j] + th * (xo[:, j + 1] - xo[:, j])
            u = uext[:, j] + th * (uext[:, j + 1] - uext[:, j])
            near = np.atleast_1d(p['model'].calc_nearest_point(x_bar))
            dx = xh - x_bar
            for i in np.unique(near):
                rows = near == i
                u[rows] += dx[rows] @ p['K'][i].T
            reg = np.atleast_1d(p['model'].calc_nearest_point(x))
            xn = np.empty_like(x)
            for i in np.unique(reg):
                rows = reg == i
                xn[rows] = x[rows] @ Ad[i].T + u[rows] @ Bd[i].T + dd[i]
            x = xn
            y = np.ascontiguousarray(x @ self.Cm.T + self.yr + p['V'][self.k, q])
            u = np.ascontiguousarray(u)
            xh = np.empty_like(x)
            for b in range(B):
                rc = lib.sekf_step(self.hs[b], dptr(u[b]), dptr(y[b]), None, None, None, dptr(xh[b]))
                if rc:
                    self.lib.check(rc, 'sekf_step')
            U[:, q] = u
        self.x, self.xh = x, xh
        self.k += 1
        return U, gu.iters.copy(), gu.status.copy()


def bytes_per_period(B, N, n, m, nz):
    D = 8
    res = dict(up=N_KEEP * B * N_Y * D, down=B * N_KEEP * (2 * n + nz + m + N_Y) * D + B * (4 + 4 + D + 4))
    solve_up = B * (n + N * m + (N + 1) * n + (N + 1) * nz) * D
    solve_down = B * ((N + 1) * n + N * m + (N + 1) * nz) * D + B * 8
    host = dict(up=solve_up + 2 * N_KEEP * B * n * D + N_KEEP * B * (m + N_Y) * D, down=solve_down + 2 * N_KEEP * B * 4 + N_KEEP * B * (n * D + 4))
    return dict(resident_observed=res, host_driven=host)


def make_loops(p, w, B):
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    n = p['x0'].shape[1]
    obs = DiscreteEKFObserverBatch(p['model'], B, Sigma0=np.eye(n), W=p['W'], V=p['Vc'])
    kw = dict(t=w['t'], z=w['z'], phase=p['phase'], K=p['K'], max_steps_per_run=N_KEEP)
    return ClosedLoopBatch(p['plans'][0], p['model'], DT_SIM, N_KEEP, observer=obs, **kw), kw


def probe_loop(B, w):
    """Measurement 2: the observed resident loop against the host-driven statement."""
    p = build(B, w)
    cl, _ = make_loops(p, w, B)
    cl.reset_observed(p['x0'], p['x_hat0'])
    hb, hb2 = ObservedHostLoop(p, p['plans'][1], w), ObservedHostLoop(p, p['plans'][1], w)
    ta, tb, tb2 = [], [], []
    agree = dict(iters_status_equal=True, u_rel_diff=0.0)
    failed = 0
    for k in range(WARM + TIMED):
        t0 = time.perf_counter()
        r = cl.run_observed(1, V=p['V'][k:k + 1], record_x=False)
        t1 = time.perf_counter()
        Ub, it, st = hb.period()
        t2 = time.perf_counter()
        hb2.period()
        t3 = time.perf_counter()
        if k >= WARM:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); tb2.append(1e3 * (t3 - t2))
        agree['iters_status_equal'] &= bool(np.array_equal(r.iters[0], it) and np.array_equal(r.status[0], st))
        agree['u_rel_diff'] = max(agree['u_rel_diff'], float(np.abs(r.u - Ub).max() / np.abs(Ub).max()))
        failed += int(r.ekf_status.sum())
    hb.close(); hb2.close()
    a, b, b2 = lp.stat(ta), lp.stat(tb), lp.stat(tb2)
    spread = abs(b['median'] - b2['median'])
    return dict(batch=B, agreement=agree, filter_failures=failed, resident_observed_ms_per_period=a, host_driven_ms_per_period=b,
                host_driven_repeat_ms_per_period=b2, host_driven_spread_ms=spread,
                resident_not_above_host_driven_by_more_than_the_spread=bool(a['median'] <= b['median'] + spread),
                waits_per_run=cl.stats()['waits_last_run'], pcie_bytes_per_period=bytes_per_period(B, w['N'], 2 * w['r'], w['m'], 6))


def probe_cost(B, w):
    """Measurement 3: the observed resident loop against the unobserved one."""
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    p = build(B, w)
    co, kw = make_loops(p, w, B)
    cu = ClosedLoopBatch(p['plans'][1], p['model'], DT_SIM, N_KEEP, **kw)
    co.reset_observed(p['x0'], p['x_hat0'])
    cu.reset(p['x0'])
    to, tu = [], []
    for k in range(WARM + TIMED):
        t0 = time.perf_counter()
        co.run_observed(1, V=p['V'][k:k + 1], record_x=False)
        t1 = time.perf_counter()
        cu.run(1, record_x=False)
        t2 = time.perf_counter()
        if k >= WARM:
            to.append(1e3 * (t1 - t0)); tu.append(1e3 * (t2 - t1))
    o, u = lp.stat(to), lp.stat(tu)
    return dict(batch=B, resident_observed_ms_per_period=o, resident_unobserved_ms_per_period=u,
                observer_costs_ms_per_period=o['median'] - u['median'], observer_costs_ms_per_sub_step=(o['median'] - u['median']) / N_KEEP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gusto_loop_observer_probe.json'))
    ap.add_argument('--filter-batches', default='1,256,4096')
    ap.add_argument('--loop-batches', default='1,256')
    ap.add_argument('--cost-batches', default='256,4096')
    args = ap.parse_args()
    import workloads as wl
    w = wl.diamond_c2()
    ints = lambda v: [int(x) for x in v.split(',') if x]
    res = dict(shape=dict(n_x=2 * w['r'], n_u=w['m'], n_y=N_Y, N=w['N'], dt=w['dt'], dt_sim=DT_SIM, n_keep=N_KEEP, gains='DARE per point',
                          warm_up=WARM, timed=TIMED, timed_steps_of_the_one_filter_handles_at_4096=fp.TIMED_HANDLES_4096, max_gusto_iters=3),
               note='ms per filter step of all B filters / per period: host clock around work that ends in the call\'s own wait; contenders '
                    'alternate in one process; B = 256 is judged, the other sizes are reported',
               filter_alone=[], observed_loop=[], cost_of_the_observer=[])
    fmodel = fp.build(w)
    for key, fn, batches in (('filter_alone', lambda B: fp.probe(B, fmodel), ints(args.filter_batches)),
                             ('observed_loop', lambda B: probe_loop(B, w), ints(args.loop_batches)),
                             ('cost_of_the_observer', lambda B: probe_cost(B, w), ints(args.cost_batches))):
        for B in batches:
            res[key].append(fn(B))
            print(key, json.dumps(res[key][-1]), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, 'w') as f:          # after every measurement: a later one that fails does not lose the earlier ones
                json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
