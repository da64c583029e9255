#!/usr/bin/env python3
"""Benchmark of the sofacontrol hot path on MI355X (contract: see the task statement / DESIGN.md).

One "step" = one pass of the hot path over one batch of synthetic input, per GPU:
  1. POD projection of a resident batch of full-order FEM snapshots  X (B x n_f) -> (B x r)
     (srom_project_dev; its launches are timed with HIP events for the HBM roofline), and
  2. R independent receding-horizon SCP solves (GuSTO on the Diamond TPWL ROM, r = 30, N = 50) started
     from the projected states, all inside ONE persistent kernel launch (sgusto_plan_solve_dev).
`value` = SCP iterations (LOCP solves) per second summed over rollouts and ranks; inputs are resident in
HBM before the timed region.

A plain run sets up, warms up, times --steps steps and prints the result line (`roofline` from the projection
launches of those steps).  --full adds everything else: the secondary metrics, the layout A/B, the CPU port
(oracle/) on a bounded sample with the parity sample (rank 0 at N = 1), the detail files.  --dump-outputs DIR
writes what the last timed step computed (rank 0) as DIR/<name>.npy.
"""
import argparse
import ctypes as C
import io
import contextlib
import json
import os
import sys
import time


def _cpu_budget():
    """CPUs this process may keep busy: the affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, -(-int(quota) // int(period))))
    except Exception:
        pass
    return n


# BEFORE numpy / scipy load their BLAS: the thread pools follow the CPU budget, not the 256 logical CPUs the box shows.  With the default
# (one spinning OpenBLAS / OpenMP worker per logical CPU) the container's CFS quota of 16 CPUs x 100 ms is used up ~25 ms into a period
# after any BLAS-heavy host phase and the kernel freezes EVERY thread of the process -- including the one waiting in hipStreamSynchronize
# -- until the period ends: the 70-90 ms "solve" outliers of rounds 3-4 (cpu.stat: nr_throttled 21, 69 s throttled in one bench run;
# with the cap: none, max solve 0.7 ms -- tools/probes/check_horizon_outliers.py).
# Half the budget: OpenBLAS workers keep spinning for a while after a call, and the thread that waits for the GPU spins as well.
for _v in ('OPENBLAS_NUM_THREADS', 'OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(_v, str(max(1, _cpu_budget() // 2)))
os.environ.setdefault('OMP_WAIT_POLICY', 'passive')

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'soft-robot-control_amd'))

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def build_model(w, tip_node=1354):
    import scipy.sparse as sp
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    from sofacontrol_amd.scp.models.tpwl import TPWLGuSTO
    n_f = w['U'].shape[0]
    Hf = sp.lil_matrix((6, 2 * n_f))
    for a in range(3):
        Hf[a, 3 * tip_node + a] = 1.0
        Hf[3 + a, n_f + 3 * tip_node + a] = 1.0
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    tp = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf.tocsr(),
                 discr_method='zoh')
    gm = TPWLGuSTO(tp)
    with contextlib.redirect_stdout(io.StringIO()):
        gm.pre_discretize(w['dt'])
    return tp, gm


def usable_cpus():
    """CPUs this process can actually keep busy: the affinity mask, capped by the cgroup CPU quota (on the GPU box
    os.cpu_count() says 256 while cpu.max grants 16 CPUs' worth of time -- more threads than that only add switching)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(np.ceil(float(quota) / float(period)))))
    except Exception:
        pass
    return n


def cpu_baseline(w, x0, x_init, z, xc, fc, n_roll, proj_rows, max_iters):
    """The CPU side of the same workload on a bounded sample, on this box's host cores (oracle/ only: never the product):
      * native twin (oracle/csrc/sofacontrol_cpu.cpp) running THE ALGORITHM OF THE GPU KERNEL -- condensed (output-space)
        interior point for the QP without its trust-region rows, stage-wise Riccati interior point of the full QP when
        that minimiser leaves the trust region, nearest-point TPWL, the GuSTO loop -- on ONE thread and on ALL usable
        cores (one rollout per thread);
      * the same twin with the stage-wise Riccati interior point throughout (round 1's algorithm), one thread;
      * the numpy port (oracle.gusto around oracle.riccati_ipm) on a few rollouts;
      * the reference's solver class -- OSQP at cvxpy's default tolerances -- as restated in oracle.locp.solve_osqp, on
        the first QP of the first rollout: what it costs in ADMM iterations and what accuracy it delivers.
    `value` is the all-cores condensed number (the strongest CPU figure); `cores` = threads actually used."""
    from oracle import gusto as ogusto, pod as opod, locp as olocp, tpwl as otpwl, cpu_twin
    import workloads as wl
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    N, m = w['N'], w['m']
    kw = dict(z=None, U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, max_gusto_iters=max_iters)
    u0 = np.zeros((n_roll, N, m))

    def twin(nr, threads, algo):
        t0 = time.perf_counter()
        xo, uo, it, _ = cpu_twin.gusto_solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, w['dt'], w['Qz'], w['R'], x0[:nr], u0[:nr],
                                             x_init[:nr], **dict(kw, z=z[:nr]), threads=threads, algo=algo)
        return time.perf_counter() - t0, xo, uo, it
    cpu_twin.lib()
    ncpu = usable_cpus()
    t1, xo1, uo1, it1 = twin(min(16, n_roll), 1, 'condensed')
    tr1, _, _, itr1 = twin(min(4, n_roll), 1, 'riccati')
    nall = min(n_roll, 16 * ncpu)
    tall, xoa, uoa, ita = twin(nall, ncpu, 'condensed')
    sols = [(xoa[b], uoa[b], int(ita[b])) for b in range(nall)]
    # numpy port, a few rollouts
    nnp = min(3, n_roll)
    t0 = time.perf_counter()
    np_iters = 0
    np_sols = []
    for b in range(nnp):
        xe, ue, _, tr = ogusto.solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, w['dt'], w['Qz'], w['R'], x0[b], np.zeros((N, m)),
                                     x_init[b], **dict(kw, z=z[b]), qp_solver='riccati_ipm')
        np_iters += len(tr)
        np_sols.append((xe, ue, len(tr)))
    t_np = time.perf_counter() - t0
    # the reference's solver class on the first QP
    A_k, B_k, d_k, _ = ogusto.traj_dynamics(model, w['Ad'], w['Bd'], w['dd'], x_init[0])
    qp = olocp.build_qp(N, w['H'], w['Qz'], w['R'], A_k, B_k, d_k, x0[0], x_init[0], 1e4, 1.0, z=z[0], U=(w['UA'], w['Ub']),
                        X=(w['XA'], w['Xb']), x_scale=1.0 / np.abs(xc))
    t0 = time.perf_counter()
    wo, _, io = olocp.solve_osqp(qp)
    t_osqp = time.perf_counter() - t0
    xq, uq, _, Jq, _ = cpu_twin.locp_solve(N, w['H'], w['Qz'], w['R'], A_k, B_k, d_k, x0[0], x_init[0], 1e4, 1.0, z=z[0], U=(w['UA'], w['Ub']),
                                           X=(w['XA'], w['Xb']), x_scale=1.0 / np.abs(xc))
    xo_, uo_, _ = olocp.split(qp, wo)
    # projection
    X = wl.snapshots(w['q_ref'], proj_rows, seed=2)
    byt = X.nbytes + w['U'].nbytes + w['q_ref'].nbytes + proj_rows * w['r'] * 8
    proj = {}
    for name, thr in (('single_thread', 1), ('all_cores', ncpu)):
        cpu_twin.project(w['U'], w['q_ref'], X[:64], threads=thr)
        t0 = time.perf_counter()
        for _ in range(3):
            cpu_twin.project(w['U'], w['q_ref'], X, threads=thr)
        proj[name] = byt / ((time.perf_counter() - t0) / 3) / 1e9
    t0 = time.perf_counter()
    opod.project(w['U'], w['q_ref'], X)
    proj['numpy'] = byt / (time.perf_counter() - t0) / 1e9
    proj['numpy_blas_threads'] = int(os.environ.get('OPENBLAS_NUM_THREADS', '0') or 0)      # NOT usable_cpus(): see the cap at the top of this file
    cpu = 'unknown CPU'
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                cpu = line.split(':', 1)[1].strip()
                break
    except Exception:
        pass
    # SURVEY 8(d), CPU baseline (3): a cvxpy model of locp.py is timed only if cvxpy + osqp import on this box
    third_party = {}
    for mod in ('cvxpy', 'osqp'):
        try:
            __import__(mod)
            third_party[mod] = True
        except Exception as exc:
            third_party[mod] = '%s: %s' % (type(exc).__name__, exc)
    have_cvx = all(v is True for v in third_party.values())
    cvxpy_osqp = {'available': have_cvx,
                  'why': ('importable, but no cvxpy model is timed: the restated OSQP leg below stands in' if have_cvx else
                          'not installed on this box (no network): ' + '; '.join('%s -> %s' % kv for kv in third_party.items() if kv[1] is not True)),
                  'stand_in': 'osqp_restated_eps1e_5 (oracle.locp.solve_osqp: the published OSQP algorithm at cvxpy\'s default tolerances)'}
    out = dict(value=float(ita.sum()) / tall, unit='SCP iterations/s', cores=ncpu, kind='port', cvxpy_osqp=cvxpy_osqp,
               algorithm='condensed (output-space) interior point + Riccati interior point for trust-region-active QPs: the algorithm of '
                         'the GPU kernels (oracle/condensed_ipm.py, csrc/locp_lean.h); native C++, -O3 -march=x86-64-v3, no BLAS',
               host='%s, %d logical CPUs, %d usable by this process (affinity / cgroup quota)' % (cpu, os.cpu_count() or 1, ncpu),
               sample_short='C2 rollouts, cap %d: compiled twin %d rollouts/%d threads %.2f s (=value), 1 thread %d rollouts %.2f s; numpy port %d rollouts '
                            '%.1f s; restated OSQP 1 QP %.1f s' % (max_iters, nall, ncpu, tall, len(it1), t1, nnp, t_np, t_osqp),
               sample='native CPU twin (oracle/csrc), condensed algorithm, one rollout per thread: %d rollouts = %d SCP iterations in %.2f s on '
                      '%d threads; single thread: %d rollouts = %d SCP iterations in %.2f s' %
                      (nall, int(ita.sum()), tall, ncpu, len(it1), int(it1.sum()), t1),
               single_thread=dict(scp_iterations_per_s=float(it1.sum()) / t1, ms_per_scp_iteration=t1 / float(it1.sum()) * 1e3,
                                  ms_per_solve=t1 / len(it1) * 1e3, rollouts=len(it1), algorithm='condensed'),
               all_cores=dict(scp_iterations_per_s=float(ita.sum()) / tall, threads=ncpu, rollouts=nall, seconds=tall, algorithm='condensed'),
               riccati_single_thread=dict(scp_iterations_per_s=float(itr1.sum()) / tr1, ms_per_scp_iteration=tr1 / float(itr1.sum()) * 1e3,
                                          rollouts=len(itr1), algorithm='stage-wise Riccati interior point throughout (rounds 1-2 baseline)'),
               numpy_port=dict(scp_iterations_per_s=np_iters / t_np, rollouts=nnp, seconds=t_np, ms_per_scp_iteration_single=t_np / max(1, np_iters) * 1e3,
                               blas_threads=int(os.environ.get('OPENBLAS_NUM_THREADS', '0') or 0),
                               what='oracle.gusto around oracle.riccati_ipm (numpy; BLAS pool = OPENBLAS_NUM_THREADS = half the CPU budget), '
                                    'one rollout after the other'),
               osqp_restated_eps1e_5=dict(what='oracle.locp.solve_osqp (published OSQP algorithm, cvxpy defaults eps_abs = eps_rel = 1e-5, no polish) '
                                               'on the first QP of rollout 0; python + scipy SuperLU, so the seconds are not those of the C library',
                                          admm_iterations=int(io['iters']), status=io['status'], seconds=t_osqp,
                                          rel_traj_error_vs_exact=float(max(np.abs(xo_ - xq).max() / np.abs(xq).max(),
                                                                            np.abs(uo_ - uq).max() / np.abs(uq).max())),
                                          rel_cost_error_vs_exact=float(abs(olocp.objective(qp, wo) - Jq) / abs(Jq))),
               pod_projection_gbs=proj)
    return out, sols, np_sols


def closed_loop_latency(w, rom, tp):
    """Per-simulation-step pieces of the closed loop (closed_loop_controller.py:65-86, controllers.py:96-98):
    projection of ONE full state through the host-pointer API (PCIe both ways inside the time) and one EKF
    predict + update step.  Latency bound: reported in microseconds, not GB/s."""
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserver
    import scipy.sparse as sp
    n_f, r = w['U'].shape
    rng = np.random.default_rng(5)
    x = np.concatenate((w['v_ref'], w['q_ref'])) + rng.standard_normal(2 * n_f)
    def median_us(fn, reps, warm):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2] * 1e6, ts[int(len(ts) * 0.99)] * 1e6

    proj_med, proj_p99 = median_us(lambda: rom.compute_RO_state(xf=x), 300, 20)
    nodes = np.arange(0, 10 * 150, 150)
    Cf = sp.lil_matrix((30, 2 * n_f))
    for i, nd in enumerate(nodes):
        for a in range(3):
            Cf[3 * i + a, n_f + 3 * nd + a] = 1.0
    tp.set_measurement_model(Cf.tocsr())
    ekf = DiscreteEKFObserver(tp)
    u = np.full(w['m'], 100.0)
    y = tp.y_ref + 0.01 * rng.standard_normal(30)
    ekf_med, ekf_p99 = median_us(lambda: ekf.update(u, y, w['dt']), 200, 10)
    fused_med, fused_p99 = median_us(lambda: ekf.update_projected(rom, x, u, y, w['dt']), 300, 20)
    # the same call straight through the C ABI (what a compiled host pays: no numpy/ctypes marshalling)
    import ctypes as C
    from sofacontrol_amd import _lib as _lm
    lib = _lm.lib()
    xr, xh = np.empty(2 * r), np.empty(2 * r)
    px, pu, py, pxr, pxh = [a.ctypes.data_as(C.c_void_p) for a in (x, u, y, xr, xh)]
    fn = lib.sekf_step_projected
    fn.argtypes = [C.c_void_p] * 7
    hk, hr = ekf._h, rom.handle
    abi_med, abi_p99 = median_us(lambda: fn(hk, hr, px, pu, py, pxr, pxh), 300, 20)
    fn.argtypes = None
    return {'project_one_state_us': proj_med, 'project_one_state_p99_us': proj_p99, 'ekf_step_us': ekf_med,
            'ekf_step_p99_us': ekf_p99, 'fused_step_us': fused_med, 'fused_step_p99_us': fused_p99,
            'fused_step_c_abi_us': abi_med, 'fused_step_c_abi_p99_us': abi_p99,
            'fused_step': 'sekf_step_projected: projection (side stream) + EKF predict/update in one call',
            'cpu': 'no twin: per-step latencies of a 2 x 4884 -> 60 projection and a 60-state EKF step; numpy needs ~0.3 ms for the same two '
                   'operations (oracle/observer.py), i.e. the host is at par here -- the fused device step exists to keep the state resident',
            'statistic': 'median (and 99th percentile) of per-call wall times',

            'workload': 'one full state (2 x %d) -> 2r = %d; EKF n_x = %d, n_y = 30; host-pointer API' % (n_f, 2 * r, 2 * r)}


def scp_c5(_lib, rank, world, dist, total=256, max_iters=5, cpu=False):
    """BASELINE config C5: 256 parallel SCP rollouts on the Trunk shape (r = 30, n_u = 8, N = 50), STRONG scaling:
    the `total` rollouts are split over the ranks (distributed.shard_range), no data-path collective (`scp_c5_weak` calls it
    with total = 256 x world: 256 rollouts PER rank -- the curve that can scale).  cpu: also the native CPU twin on this rank's
    shard, all usable cores (rank 0 of a single-GPU run only)."""
    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.distributed import shard_range
    from sofacontrol_amd.mor.pod import POD
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    w = wl.trunk_c5()
    N, m, r, dt = w['N'], w['m'], w['r'], w['dt']
    lo, hi = shard_range(total, rank, world)
    Bn = hi - lo
    rom = POD(dict(U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    tp, gm = build_model(w, w['tip_node'])
    xc, fc = gm.get_characteristic_vals()
    X = wl.snapshots(w['q_ref'], total, seed=9)[lo:hi]
    x0 = np.concatenate((np.zeros((Bn, r)), rom.compute_RO_state(qf=X)), axis=1)
    u_init = np.zeros((Bn, N, m))
    x_init, _ = tp.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    z = np.stack([zi((lo + b) * (10.0 / total) + dt * np.arange(N + 1)) for b in range(Bn)])
    # first_solve_cap: the constructor's own solve at the cap of the timed calls (the reference-default 500 costs 1.3-1.8 s here -- the
    # trust-region-active tail of a few rollouts -- and was half of a bench run's GPU time; `scp_uncapped_500` reports that regime for C2)
    t_c = time.perf_counter()
    g = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']), x_char=xc, f_char=fc,
              convg_thresh=1e-3, batch=Bn, max_trace=0, max_gusto_iters=max_iters, first_solve_cap=max_iters)
    t_c = time.perf_counter() - t_c
    g.max_gusto_iters = max_iters
    if dist is not None:
        dist.barrier()
    _lib.sync()
    els = []
    for _ in range(3):       # best of 3 calls, all reported (ms_all_calls): the first call after other work in the process can carry a
        t0 = time.perf_counter()            # one-off allocation of the runtime (measured: 43 ms once, then 13.5 ms)
        g.solve_batch(x0, u_init, x_init, z=z)
        els.append(time.perf_counter() - t0)
    el = min(els)
    its = float(g.iters.sum())
    # the reduction step of the sharded batch: one all_gather of the per-rollout optimal costs, every rank
    # learns the global best rollout (outside the solve's wall time: 256 doubles)
    from sofacontrol_amd.distributed import gather_rollout_costs
    J_loc = g.costs
    if dist is not None:
        import torch
        J_all, best = gather_rollout_costs(torch.from_numpy(J_loc).cuda(), total)
        tt = torch.tensor([el, its], dtype=torch.float64, device='cuda')
        tm = tt.clone()
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        dist.all_reduce(tt, op=dist.ReduceOp.SUM)
        el, its = float(tm[0]), float(tt[1])
    else:
        J_all, best = gather_rollout_costs(J_loc, Bn)
    cpu_entry = None
    if cpu:
        try:
            from oracle import cpu_twin
            model = dict(w['tab'], w_q=1.0, w_v=0.0)
            ncpu = usable_cpus()
            nb = min(Bn, 16 * ncpu)
            t0 = time.perf_counter()
            _, _, itc, _ = cpu_twin.gusto_solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, dt, w['Qz'], w['R'], x0[:nb], u_init[:nb], x_init[:nb],
                                                z=z[:nb], U=(w['UA'], w['Ub']), x_char=xc, f_char=fc, convg_thresh=1e-3, max_gusto_iters=max_iters,
                                                threads=ncpu, algo='condensed')
            tc = time.perf_counter() - t0
            cpu_entry = {'what': 'native CPU twin (same algorithm), %d rollouts on %d threads' % (nb, ncpu), 'seconds': tc,
                         'iterations_per_s': float(itc.sum()) / tc, 'iterations_equal_gpu': bool((itc == g.iters[:nb]).all()),
                         'gpu_over_cpu_throughput': (its / el) / (float(itc.sum()) / tc)}
        except Exception as exc:
            cpu_entry = {'error': repr(exc)}
    return {'workload': 'C5: Trunk n_f=2127, r=30 (n_x=60, n_u=8), N=50, dt=%g, U box; %d rollouts in total, %d per rank, '
                        '%s; host buffers; best of 3 calls' % (dt, total, Bn, 'weak scaling (256 per rank)' if total == 256 * world else 'strong scaling (%d shared by %d ranks)' % (total, world)),
            'cpu': cpu_entry if cpu_entry is not None else 'no twin run on this rank / entry (see scp_c5 of a single-GPU run)',
            'iterations_per_s': its / el, 'ms': el * 1e3, 'ms_all_calls': [e * 1e3 for e in els], 'iterations': its,
            'constructor_s (plan creation + first solve at first_solve_cap = %d)' % max_iters: t_c,
            'not_converged_rank0': int((g.status != 0).sum()), 'kernel': g.kernel_info['kernel'],
            'rollouts_handed_to_fused_kernel': int(g.kernel_info['handed_over']),
            'best_rollout': {'global_index': best, 'cost': float(J_all[best]) if best >= 0 else None, 'costs_gathered': int(J_all.size),
                             'how': 'distributed.gather_rollout_costs: all_gather of the per-rollout optimal LOCP values (sgusto_plan_costs)'}}


def scp_c2_r36(_lib, total=1024, max_iters=5, cpu_rollouts=64):
    """C2 at the size of the reference's SHIPPED Diamond basis (examples/diamond/pod_model.pkl: r = 36, n_x = 72): the fixed-layout lean
    instantiation <4, 72, 4, 50, 18, 4> and the split-panel fused kernel behind it; `total` rollouts, host buffers, best of 3 calls;
    the native CPU twin on the first `cpu_rollouts` of them, all usable cores."""
    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.mor.pod import POD
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    w = wl.diamond_c2(r=36)
    N, m, r, dt = w['N'], w['m'], w['r'], w['dt']
    rom = POD(dict(U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    tp, gm = build_model(w, 1354)
    xc, fc = gm.get_characteristic_vals()
    X = wl.snapshots(w['q_ref'], total, seed=2)
    x0 = np.concatenate((np.zeros((total, r)), rom.compute_RO_state(qf=X)), axis=1)
    u_init = np.zeros((total, N, m))
    x_init, _ = tp.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    z = np.stack([zi(b * (10.0 / total) + dt * np.arange(N + 1)) for b in range(total)])
    g = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']), X=Polyhedron(w['XA'], w['Xb']), x_char=xc,
              f_char=fc, convg_thresh=1e-3, batch=total, max_trace=0, max_gusto_iters=max_iters, first_solve_cap=max_iters)
    _lib.sync()
    els = []
    for _ in range(3):
        t0 = time.perf_counter()
        g.solve_batch(x0, u_init, x_init, z=z)
        els.append(time.perf_counter() - t0)
    el, its = min(els), float(g.iters.sum())
    g1 = GuSTO(gm, N, dt, w['Qz'], w['R'], x0[0], u_init[0], x_init[0], z=z[0], U=Polyhedron(w['UA'], w['Ub']), X=Polyhedron(w['XA'], w['Xb']),
               x_char=xc, f_char=fc, convg_thresh=1e-3, max_trace=0, max_gusto_iters=max_iters, first_solve_cap=max_iters)
    per = []
    for b in range(8):
        bb = b * (total // 8)
        t0 = time.perf_counter()
        g1.solve(x0[bb], u_init[bb], x_init[bb], z=z[bb])
        per.append((time.perf_counter() - t0) / max(1, int(g1.iters[0])))
    cpu_entry = 'no twin run'
    try:
        from oracle import cpu_twin
        model = dict(w['tab'], w_q=1.0, w_v=0.0)
        ncpu, nb = usable_cpus(), min(total, cpu_rollouts)
        t0 = time.perf_counter()
        _, _, itc, _ = cpu_twin.gusto_solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, dt, w['Qz'], w['R'], x0[:nb], u_init[:nb], x_init[:nb], z=z[:nb],
                                            U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3,
                                            max_gusto_iters=max_iters, threads=ncpu, algo='condensed')
        tc = time.perf_counter() - t0
        cpu_entry = {'what': 'native CPU twin (same algorithm), %d rollouts on %d threads' % (nb, ncpu), 'seconds': tc,
                     'iterations_per_s': float(itc.sum()) / tc, 'iterations_equal_gpu': bool((itc == g.iters[:nb]).all()),
                     'gpu_over_cpu_throughput': (its / el) / (float(itc.sum()) / tc)}
    except Exception as exc:
        cpu_entry = {'error': repr(exc)}
    return {'workload': 'C2 at the shipped Diamond basis size: r = 36 (n_x = 72, n_u = 4), N = 50, dt = %g, U box + X box; %d rollouts, cap %d, '
                        'host buffers; best of 3 calls' % (dt, total, max_iters),
            'iterations_per_s': its / el, 'ms': el * 1e3, 'ms_all_calls': [e * 1e3 for e in els], 'iterations': its,
            'ms_per_scp_iteration_one_rollout_median': sorted(per)[4] * 1e3,
            'not_converged': int((g.status != 0).sum()), 'kernel': g.kernel_info['kernel'],
            'rollouts_handed_to_fused_kernel': int(g.kernel_info['handed_over']), 'cpu': cpu_entry}


def scp_single_rollout(w, gm, tp, xc, fc, x0, x_init, z, max_iters):
    """The reference's actual use: ONE receding-horizon solve at a time (scp/ros.py:94-127), C2 shape.  Wall time of
    GuSTO.solve through the host-pointer API (PCIe copies inside), per SCP iteration and per solve, against the replan
    budget of the Diamond driver (N_replan = 10 steps of 0.01 s: examples/diamond/diamond.py:230,249)."""
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    N, m = w['N'], w['m']
    out = {'workload': 'C2, one rollout at a time (batch = 1 plan), host buffers; median over rollouts', 'replan_budget_ms': 100.0}
    for cap, key in ((max_iters, 'capped'), (500, 'reference_default_500')):
        g = GuSTO(gm, N, w['dt'], w['Qz'], w['R'], x0[0], np.zeros((N, m)), x_init[0], z=z[0], U=Polyhedron(w['UA'], w['Ub']),
                  X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, max_trace=0, max_gusto_iters=cap)
        ts, its = [], []
        for b in range(8):
            t0 = time.perf_counter()
            g.solve(x0[b], np.zeros((N, m)), x_init[b], z=z[b])
            ts.append(time.perf_counter() - t0)
            its.append(int(g.iters[0]))
        per_it = sorted(t / i for t, i in zip(ts, its))
        out[key] = {'max_gusto_iters': cap, 'ms_per_solve_median': sorted(ts)[len(ts) // 2] * 1e3, 'ms_per_solve_max': max(ts) * 1e3,
                    'scp_iterations': its, 'ms_per_scp_iteration_median': per_it[len(per_it) // 2] * 1e3}
    out['cpu'] = 'cpu_baseline.gpu_vs_cpu.single_rollout_ms_per_scp_iteration (native twin, one thread, same problems)'
    out['ms_per_scp_iteration'] = out['capped']['ms_per_scp_iteration_median']
    out['within_replan_budget'] = bool(out['capped']['ms_per_solve_max'] <= 100.0)
    return out


def scp_reference_horizons(tip_node=1354):
    """The horizons the reference's own drivers solve on the Diamond (BASELINE C2 keeps N = 50): the closed-loop drivers replan a
    short horizon -- examples/diamond/diamond.py:309-316 (N = 5, dt = 0.05, U + X box, default cap of 500 SCP iterations) and
    examples/hardware/diamond.py:393-399 (N = 3, dt = 0.1, U box only, max_gusto_iters = 5) -- and the open-loop planner solves the
    whole figure-8 at once, examples/hardware/diamond.py:471-474 (N = 200, dt = 0.05, U box only, no warm start).  One rollout at a
    time through the host-pointer API, as the drivers do; same synthetic C2 model (workloads.diamond_c2 at that N / dt)."""
    import workloads as wl
    from scipy.interpolate import interp1d
    from sofacontrol_amd.mor.pod import POD
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    out = {}
    from oracle import cpu_twin
    for key, N, dt, with_X, cap, reps, ref in (('closed_loop_N5', 5, 0.05, True, 500, 8, 'examples/diamond/diamond.py:309-316'),
                                             ('hardware_closed_loop_N3', 3, 0.1, False, 5, 8, 'examples/hardware/diamond.py:393-399'),
                                             ('hardware_open_loop_N200', 200, 0.05, False, 500, 3, 'examples/hardware/diamond.py:471-474')):
        try:
            w = wl.diamond_c2(N=N, dt=dt, with_X=with_X)
            m, r = w['m'], w['r']
            rom = POD(dict(U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
            tp, gm = build_model(w, tip_node)
            xc, fc = gm.get_characteristic_vals()
            X = wl.snapshots(w['q_ref'], reps, seed=2)
            x0 = np.concatenate((np.zeros((reps, r)), rom.compute_RO_state(qf=X)), axis=1)
            u0 = np.zeros((N, m))
            x_init, _ = tp.rollout(x0, np.zeros((reps, N, m)), dt)
            zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
            z = np.stack([zi(b * 10.0 / reps + dt * np.arange(N + 1)) for b in range(reps)])
            g = GuSTO(gm, N, dt, w['Qz'], w['R'], x0[0], u0, x_init[0], z=z[0], U=Polyhedron(w['UA'], w['Ub']),
                      X=Polyhedron(w['XA'], w['Xb']) if with_X else None, x_char=xc, f_char=fc, convg_thresh=1e-3, max_trace=0, max_gusto_iters=cap)
            ts, its, st, slow = [], [], [], []
            nsolve = reps if N >= 200 else 64          # the closed-loop horizons: 64 CONSECUTIVE solves (cycling through the problems), as a
            for i in range(nsolve):                    # controller issues them -- first, median and worst are reported separately
                b = i % reps
                t0 = time.perf_counter()
                g.solve(x0[b], u0, x_init[b], z=z[b])
                ts.append(time.perf_counter() - t0)
                its.append(int(g.iters[0])); st.append(int(g.status[0]))
                if ts[-1] > 0.02 and N < 200:           # an outlier: what was that solve?
                    slow.append({'solve': i, 'problem': b, 'ms': ts[-1] * 1e3, 'scp_iterations': its[-1], 'status': st[-1],
                                 'handed_to_fused_kernel': int(g.kernel_info['handed_over'])})
            per = sorted(t / max(1, i) for t, i in zip(ts, its))
            ki = g.kernel_info
            med = sorted(ts)[len(ts) // 2]
            out[key] = {'reference_driver': ref, 'N': N, 'dt': dt, 'X_rows': 4 if with_X else 0, 'max_gusto_iters': cap, 'solves': nsolve,
                        'problem': "the synthetic C2 model (workloads.diamond_c2) at the driver's N / dt / state rows / cap; costs and U box are C2's "
                                   "(Qz on tip x and y, U in [0, 1500]) -- the hardware driver itself weights (y, z) and bounds U in [200, 2500] "
                                   "(examples/hardware/diamond.py:376-386): same problem class and size, not the same numbers",
                        'ms_first_solve': ts[0] * 1e3, 'ms_per_solve_median': med * 1e3, 'ms_per_solve_max': max(ts) * 1e3,
                        'ms_per_solve_max_excluding_first': max(ts[1:]) * 1e3, 'max_over_median': max(ts) / med,
                        'ms_per_solve_first_8': [t * 1e3 for t in ts[:8]], 'solves_above_20_ms': slow, 'scp_iterations': its[:reps],
                        'status_nonzero': int(sum(1 for v in st if v != 0)), 'ms_per_scp_iteration_median': per[len(per) // 2] * 1e3, 'kernel': ki['kernel'],
                        'handed_to_fused_kernel_last_solve': ki['handed_over']}
            if N < 200:
                # the reference's warm_start=True keeps the solver state across solves (locp.py:181): GuSTO(keep_solver_state=True) starts the
                # first QP of every solve from the previous solve's minimiser and multipliers -- the same 64-solve series with it
                gk = GuSTO(gm, N, dt, w['Qz'], w['R'], x0[0], u0, x_init[0], z=z[0], U=Polyhedron(w['UA'], w['Ub']),
                           X=Polyhedron(w['XA'], w['Xb']) if with_X else None, x_char=xc, f_char=fc, convg_thresh=1e-3, max_trace=0, max_gusto_iters=cap,
                           keep_solver_state=True)
                tk, ik = [], []
                for i in range(nsolve):
                    b = i % reps
                    t0 = time.perf_counter()
                    gk.solve(x0[b], u0, x_init[b], z=z[b])
                    tk.append(time.perf_counter() - t0)
                    ik.append(int(gk.iters[0]))
                perk = sorted(t / max(1, i) for t, i in zip(tk, ik))
                out[key]['keep_solver_state'] = {'honoured_by_the_kernels': bool(gk.solver_state_kept), 'what': 'GuSTO(keep_solver_state=True): solver state kept across solves like the reference\'s warm_start=True',
                                                 'ms_per_scp_iteration_median': perk[len(perk) // 2] * 1e3, 'ms_per_solve_median': sorted(tk)[len(tk) // 2] * 1e3,
                                                 'scp_iterations_equal_cold': bool(ik == its)}
                # the same `reps` problems as ONE batched launch (one workgroup each, concurrently): where the GPU overtakes a host core
                gb = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, np.zeros((reps, N, m)), x_init, z=z, U=Polyhedron(w['UA'], w['Ub']),
                           X=Polyhedron(w['XA'], w['Xb']) if with_X else None, x_char=xc, f_char=fc, convg_thresh=1e-3, batch=reps, max_trace=0,
                           max_gusto_iters=cap)
                tb = []
                for _ in range(8):
                    t0 = time.perf_counter()
                    gb.solve_batch(x0, np.zeros((reps, N, m)), x_init, z=z)
                    tb.append(time.perf_counter() - t0)
                out[key]['batch_of_%d' % reps] = {'ms_per_launch_median': sorted(tb)[len(tb) // 2] * 1e3, 'scp_iterations': int(gb.iters.sum()),
                                                  'ms_per_scp_iteration_amortised': sorted(tb)[len(tb) // 2] * 1e3 / max(1, int(gb.iters.sum()))}
            # SURVEY 8(d) "CPU baseline (1)": the native twin (same algorithm) on the same problems, ONE thread -- what one host core
            # needs for the solve a closed loop waits for
            try:
                model = dict(w['tab'], w_q=1.0, w_v=0.0)
                nb = reps if N < 200 else 1
                kw = dict(z=z[:nb], U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']) if with_X else None, x_char=xc, f_char=fc, convg_thresh=1e-3,
                          max_gusto_iters=cap)
                u0b = np.zeros((nb, N, m))
                cpu_twin.gusto_solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, dt, w['Qz'], w['R'], x0[:1], u0b[:1], x_init[:1], **dict(kw, z=z[:1]),
                                     threads=1, algo='condensed')
                t0 = time.perf_counter()
                _, _, itc, _ = cpu_twin.gusto_solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], N, dt, w['Qz'], w['R'], x0[:nb], u0b, x_init[:nb], **kw,
                                                    threads=1, algo='condensed')
                tc = time.perf_counter() - t0
                cpu_ms = tc / max(1, int(itc.sum())) * 1e3
                out[key]['cpu'] = {'what': 'native CPU twin, one thread, same algorithm, %d of the same problems' % nb,
                                   'ms_per_scp_iteration': cpu_ms, 'scp_iterations': [int(v) for v in itc],
                                   'iterations_equal_gpu': bool(all(int(a) == int(b_) for a, b_ in zip(itc, its[:nb]))),
                                   'cpu_over_gpu_latency': cpu_ms / out[key]['ms_per_scp_iteration_median']}
                if 'batch_of_%d' % reps in out[key]:
                    out[key]['cpu']['cpu_over_gpu_batch_of_%d' % reps] = cpu_ms / out[key]['batch_of_%d' % reps]['ms_per_scp_iteration_amortised']
            except Exception as exc:
                out[key]['cpu'] = {'error': repr(exc)}
        except Exception as exc:
            out[key] = {'error': repr(exc)}
    return out


def pod_shapes(L, _lib, B=65536):
    """the projection at the shipped r = 36 as well, the lift (pod.py:54-66) and the full-state form
    (both blocks, `compute_RO_state(xf=...)`); resident buffers, HIP events over 100 launches after 30 warm-up ones."""
    import workloads as wl
    from sofacontrol_amd.mor.pod import POD
    n_f = 4884
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.srh_event_create(C.byref(e0)); L.srh_event_create(C.byref(e1))

    def timed(fn, reps=100):
        for _ in range(30):
            fn()
        _lib.sync(); L.srh_event_record(e0, None)
        for _ in range(reps):
            fn()
        L.srh_event_record(e1, None); _lib.sync()
        ms = C.c_float(); L.srh_event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value / reps * 1e-3

    out = {'workload': 'B = %d snapshots x n_f = %d, f64, resident; GB/s of the algorithmic bytes' % (B, n_f),
           'cpu': 'cpu_baseline.pod_projection_gbs (native twin, one thread / all cores, and numpy) is the CPU side of the projection; the lift and '
                  'U^T M U have no twin (same memory-bound shape: the projection figure is representative)'}
    U0, q_ref, v_ref = wl.pod_basis(n_f, 30, seed=0)
    X = wl.snapshots(q_ref, B, seed=2)
    dX = _lib.DeviceBuffer.from_array(X)
    del X
    for r in (30, 36):
        U, q_ref, v_ref = wl.pod_basis(n_f, r, seed=0)
        rom = POD(dict(U=U, q_ref=q_ref, v_ref=v_ref))
        dXr = _lib.DeviceBuffer(B * r * 8)
        byt = 8.0 * (B * n_f + n_f * r + n_f + B * r)
        t = timed(lambda: _lib.check(L.srom_project_dev(rom.handle, 0, dX.ptr, C.c_int64(B), C.c_int64(n_f), dXr.ptr,
                                                        C.c_int64(r), None), 'project'))
        out['project_r%d' % r] = {'ms': t * 1e3, 'gbs': byt / t / 1e9, 'frac_of_hbm_peak': byt / t / 8e12}
        # full-state form on the same bytes: B/2 states [v; q] of 2 n_f
        t = timed(lambda: _lib.check(L.srom_project_dev(rom.handle, 2, dX.ptr, C.c_int64(B // 2), C.c_int64(2 * n_f), dXr.ptr,
                                                        C.c_int64(2 * r), None), 'project_x'))
        out['project_x_r%d' % r] = {'ms': t * 1e3, 'gbs': byt / t / 1e9, 'frac_of_hbm_peak': byt / t / 8e12}
        t = timed(lambda: _lib.check(L.srom_lift_dev(rom.handle, 0, dXr.ptr, C.c_int64(B), C.c_int64(r), dX.ptr,
                                                     C.c_int64(n_f), None), 'lift'))
        out['lift_r%d' % r] = {'ms': t * 1e3, 'gbs': byt / t / 1e9, 'frac_of_hbm_peak': byt / t / 8e12}
        # U^T M U of a dense n_f x n_f matrix (mor/pod.py:56-72) in one pass over M: the first 191 MB of the batch buffer
        # serve as M (the values do not matter for the time)
        dP = _lib.DeviceBuffer(r * r * 8)
        t = timed(lambda: _lib.check(L.srom_reduce_matrix_dev(rom.handle, dX.ptr, C.c_int64(n_f), 1, 1, dP.ptr, None), 'reduce'),
                  reps=300)
        out['utmu_r%d' % r] = {'us': t * 1e6, 'gbs': 8.0 * n_f * n_f / t / 1e9, 'frac_of_hbm_peak': 8.0 * n_f * n_f / t / 8e12,
                               'what': 'U^T M U, M 4884 x 4884 f64 resident, one pass + one reduction launch'}
        # K, D, M, S of one TPWL point in one launch pair (srom_reduce_matrices_dev; tpwl/tpwl_utils.py:96-103): four n_f x n_f windows of the batch buffer
        dP4 = [_lib.DeviceBuffer(r * r * 8) for _ in range(4)]
        PP = C.c_void_p * 4
        mp = PP(*[C.c_void_p(dX.ptr.value + i * n_f * n_f * 8) for i in range(4)])
        op = PP(*[b.ptr for b in dP4])
        t = timed(lambda: _lib.check(L.srom_reduce_matrices_dev(rom.handle, mp, 4, op, None), 'reduce4'), reps=100)
        alg4 = 4 * 8.0 * (n_f * n_f + 2 * n_f * r + r * r)
        out['utmu4_r%d' % r] = {'us': t * 1e6, 'us_per_matrix': t * 1e6 / 4, 'gbs': alg4 / t / 1e9, 'frac_of_hbm_peak': alg4 / t / 8e12,
                                'what': 'U^T M U of FOUR 4884 x 4884 f64 matrices in one launch pair (K, D, M, S of a TPWL point)'}
        for b in dP4:
            b.free()
        dP.free()
        dXr.free()
    dX.free()
    return out


def model_prep(_lib):
    """Round-6 kernels off the SCP path, each beside the host routine the reference calls for it: time discretisation of one horizon of
    blended TPWL models (tpwl.py:244-250, 272-297: scipy.linalg.expm / numpy inverses per model) and the full-spectrum eigh of a
    2048-snapshot Gramian without a vendor library (mor/pod.py:181-200: numpy SVD)."""
    import ctypes as C
    from sofacontrol_amd.mor.pod import _device_eigh
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import tpwl as otpwl
    rng = np.random.default_rng(0)
    n, m, batch, h = 60, 4, 51, 30
    A = np.zeros((batch, n, n)); B = rng.standard_normal((batch, n, m)); d = rng.standard_normal((batch, n))
    for b in range(batch):
        Q, _ = np.linalg.qr(rng.standard_normal((h, h)))
        K = Q @ np.diag(np.logspace(0, 4.5, h)) @ Q.T
        A[b, :h, :h], A[b, :h, h:], A[b, h:, :h] = -(0.02 * K + 0.5 * np.eye(h)), -K, np.eye(h)
    Ad = np.empty_like(A); Bd = np.empty_like(B); dd = np.empty_like(d)
    res = {'discretize': {'workload': '51 affine models, n_x = 60, n_u = 4 (one horizon of a weighting-mode TPWL linearisation), dt = 0.05, host buffers'}}
    for name, code in (('be', 1), ('bil', 2), ('zoh', 3)):
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            _lib.check(_lib.lib().stpwl_discretize(C.c_int(code), C.c_int(n), C.c_int(m), C.c_int64(batch), _lib.dptr(A), _lib.dptr(B), _lib.dptr(d),
                                                   C.c_double(0.05), _lib.dptr(Ad), _lib.dptr(Bd), _lib.dptr(dd)), 'stpwl_discretize')
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        worst = 0.0
        for b in range(batch):
            Ae, Be, de = otpwl.discretize(A[b], B[b], d[b], 0.05, name)
            worst = max(worst, float(np.abs(Ad[b] - Ae).max() / max(1.0, np.abs(Ae).max())))
        res['discretize'][name] = {'ms': min(ts[1:]) * 1e3, 'cpu_ms': (time.perf_counter() - t0) * 1e3, 'max_rel_A_vs_cpu': worst}
    ns = 2048
    S = rng.standard_normal((ns, ns + 3)) * np.logspace(0, -3, ns + 3)
    G = S @ S.T
    _device_eigh(G[:256, :256])
    t0 = time.perf_counter(); w, W = _device_eigh(G); t1 = time.perf_counter()
    t2 = time.perf_counter(); we, We = np.linalg.eigh(G); t3 = time.perf_counter()
    res['eigh_2048'] = {'kernel': 'block Jacobi (csrc/eigh.hip: bj_sub_kernel, bj_update_a_kernel, bj_update_v_kernel), eigenvectors included',
                        'ms': (t1 - t0) * 1e3, 'cpu_ms_numpy_eigh': (t3 - t2) * 1e3, 'blas_threads': int(os.environ.get('OPENBLAS_NUM_THREADS', '0') or 0),
                        'max_rel_w_vs_cpu': float(np.abs(w - we).max() / np.abs(we).max())}
    return res


def secondary(L, _lib, rank, world, dist):
    import workloads as wl
    """Secondary metrics of SURVEY.md section 8(d), measured outside the timed region of the headline metric:
    C3 iLQR iterations/s (SSM r=10, n_u=8, horizon 100), C4 per-GPU share of the snapshot Gramian (10 000
    snapshots x 50 000/8 DoF) in TFLOP/s plus the RCCL all-reduce of the Gramian when world > 1."""
    from sofacontrol_amd.SSM.ssm import SSMDynamics
    from sofacontrol_amd.lqr.ilqr import iLQR
    from sofacontrol_amd.utils import QuadraticCost
    out = {}
    # ---- C3
    c3 = wl.ssm_c3(256, rank)                        # C3 at dt = 0.05, backward Euler (examples/trunk/trunk.py:365);
    n, m, N, dt, Bn = c3['n'], c3['m'], c3['N'], c3['dt'], c3['x0'].shape[0]      # tests/test_ssm_gpu.py checks the same construction
    model = c3['model']

    def mat(v):
        a = np.empty((1, 1), dtype=object); a[0, 0] = np.asarray(v); return a
    sc = lambda v: mat(np.array([[v]]))
    s = SSMDynamics(model['z_ref'].copy(), discrete=False, discr_method=c3['discr'],
                    model=dict(Ts=sc(dt), w_coeff=mat(model['W']), v_coeff=mat(model['V']), r_coeff=mat(model['R']),
                               B=mat(model['B']), rd_coeff=mat(model['Rd']), Bd=mat(model['Bd'])),
                    params=dict(state_dim=sc(n), input_dim=sc(m), output_dim=sc(n), SSM_order=sc(2), ROM_order=sc(3)))
    s.H = model['W'][:, :n].copy()
    Qz, x0, zt = c3['Qz'], c3['x0'], c3['zt']
    il = iLQR(dt, s, QuadraticCost(Q=Qz, R=c3['R'], Qf=c3['Qf']), N)
    il.set_target(zt)
    il.ilqr_computation(x0)
    ts = []
    for _ in range(3):       # the 16 MB of fresh numpy outputs make the wall time bimodal (first-touch page faults of the D2H copy)
        t0 = time.perf_counter()
        il.ilqr_computation(x0)
        ts.append(time.perf_counter() - t0)
    t = min(ts)
    il1 = iLQR(dt, s, QuadraticCost(Q=Qz, R=c3['R'], Qf=c3['Qf']), N)
    il1.set_target(zt[0])
    il1.ilqr_computation(x0[0])
    t1s = []
    for _ in range(3):
        t0 = time.perf_counter()
        il1.ilqr_computation(x0[0])
        t1s.append(time.perf_counter() - t0)
    out['ilqr_c3'] = {'workload': 'C3 (workloads.ssm_c3): SSM n_x=10 (285 monomials), n_u=8, horizon 100, dt=0.05 backward Euler, %d problems, host buffers '
                                  '(PCIe copies inside the time); best of 3 calls' % Bn,
                      'iterations_per_s': float(il.iters.sum()) / t, 'ms': t * 1e3, 'ms_all_calls': [x * 1e3 for x in ts],
                      'iterations': int(il.iters.sum()), 'one_problem_ms': min(t1s) * 1e3, 'one_problem_iterations': int(np.atleast_1d(il1.iters)[0])}
    if rank == 0:
        try:      # SURVEY 8(d) "CPU baseline (1)": the native twin of the same iLQR (oracle/csrc, pinned to oracle/lqr.py), one thread and all cores
            from oracle import cpu_twin
            ncpu = usable_cpus()
            cargs = (n, m, 3, 2, model['R'], model['B'], model['W'], model['z_ref'], s.H, c3['discr'], dt, Qz, c3['R'], c3['Qf'], N)
            t0 = time.perf_counter()
            _, _, _, _, it1 = cpu_twin.ilqr_ssm(*cargs, x0[:4], zt[:4], threads=1)
            tc1 = (time.perf_counter() - t0) / 4
            t0 = time.perf_counter()
            _, _, _, _, ita = cpu_twin.ilqr_ssm(*cargs, x0, zt, threads=ncpu)
            tca = time.perf_counter() - t0
            out['ilqr_c3']['cpu'] = {'what': 'native CPU twin (oracle/csrc: analytic sparse Jacobians, Gauss-Jordan discretisation), same iLQR',
                                     'one_problem_ms_one_thread': tc1 * 1e3, 'all_problems_ms': tca * 1e3, 'threads': ncpu,
                                     'iterations_per_s_all_cores': float(ita.sum()) / tca,
                                     'iterations_equal_gpu': bool((ita == il.iters).all()),
                                     'gpu_over_cpu_throughput': (float(il.iters.sum()) / t) / (float(ita.sum()) / tca),
                                     'cpu_over_gpu_latency_one_problem': tc1 / min(t1s)}
        except Exception as exc:
            out['ilqr_c3']['cpu'] = {'error': repr(exc)}
    # ---- iLQR on the Diamond TPWL model of the headline configuration (the north star names "the reference CPU SCP/iLQR solve on the
    # Diamond robot (r = 30, horizon = 50)"; lqr/ilqr.py:27-300 through examples/diamond/diamond.py:190-230): one problem at a time
    # (the controller's use) and 256 problems in one launch; parity: tests/test_lqr_gpu.py
    try:
        wd = wl.diamond_c2()
        tpd, _ = build_model(wd, 1354)
        Nd, md, rd, dtd = wd['N'], wd['m'], wd['r'], wd['dt']
        romd = None
        Xs = wl.snapshots(wd['q_ref'], 256, seed=2)
        from sofacontrol_amd.mor.pod import POD
        romd = POD(dict(U=wd['U'], q_ref=wd['q_ref'], v_ref=wd['v_ref']))
        x0d = np.concatenate((np.zeros((256, rd)), romd.compute_RO_state(qf=Xs)), axis=1)
        zr = np.asarray(tpd.z_ref) if getattr(tpd, 'z_ref', None) is not None else np.zeros(6)
        ztd = wd['z'][:Nd + 1] + zr
        ild = iLQR(dtd, tpd, QuadraticCost(Q=wd['Qz'], R=1e-3 * np.eye(md), Qf=10 * wd['Qz']), Nd)
        ild.set_target(ztd)
        ild.ilqr_computation(x0d[0])
        per = []
        for b in range(8):
            t0 = time.perf_counter()
            ild.ilqr_computation(x0d[32 * b])
            per.append((time.perf_counter() - t0) * 1e3 / max(1, int(np.atleast_1d(ild.iters)[0])))
        per.sort()
        ild.ilqr_computation(x0d)
        tb = []
        for _ in range(3):
            t0 = time.perf_counter()
            ild.ilqr_computation(x0d)
            tb.append(time.perf_counter() - t0)
        out['ilqr_diamond'] = {'workload': 'Diamond TPWL (workloads.diamond_c2: n_x = 60, n_u = 4, P = 64), iLQR horizon %d, dt = %g, figure-8 target, '
                                           'R = 1e-3 I, Qf = 10 Qz; host buffers' % (Nd, dtd),
                               'ms_per_iteration_one_problem_median': per[4], 'ms_per_iteration_one_problem_min_max': [per[0], per[-1]],
                               'batch_256_ms': min(tb) * 1e3, 'batch_256_ms_all_calls': [t * 1e3 for t in tb],
                               'batch_256_iterations': int(ild.iters.sum()), 'batch_256_iterations_per_s': float(ild.iters.sum()) / min(tb)}
        if rank == 0:
            try:
                from oracle import cpu_twin
                ncpu = usable_cpus()
                modeld = dict(wd['tab'], w_q=1.0, w_v=0.0)
                targs = (modeld, wd['Ad'], wd['Bd'], wd['dd'], np.asarray(tpd.H), zr, wd['Qz'], 1e-3 * np.eye(md), 10 * wd['Qz'], Nd)
                ztb = np.broadcast_to(ztd, (256,) + ztd.shape).copy()
                t0 = time.perf_counter()
                _, _, _, _, itc1 = cpu_twin.ilqr_tpwl(*targs, x0d[:2], ztb[:2], threads=1)
                tc1 = (time.perf_counter() - t0) / max(1, int(itc1.sum()))
                t0 = time.perf_counter()
                _, _, _, _, itca = cpu_twin.ilqr_tpwl(*targs, x0d, ztb, threads=ncpu)
                tca = time.perf_counter() - t0
                out['ilqr_diamond']['cpu'] = {'what': 'native CPU twin of the same iLQR on the same TPWL tables (oracle/csrc)', 'threads': ncpu,
                                              'ms_per_iteration_one_problem_one_thread': tc1 * 1e3, 'batch_256_ms_all_cores': tca * 1e3,
                                              'batch_256_iterations_per_s_all_cores': float(itca.sum()) / tca,
                                              'iterations_equal_gpu': bool((itca == ild.iters).all()),
                                              'gpu_over_cpu_throughput': out['ilqr_diamond']['batch_256_iterations_per_s'] / (float(itca.sum()) / tca),
                                              'cpu_over_gpu_latency_one_problem': tc1 * 1e3 / per[4]}
            except Exception as exc:
                out['ilqr_diamond']['cpu'] = {'error': repr(exc)}
    except Exception as exc:                      # a secondary measurement never takes the line down
        out['ilqr_diamond'] = {'error': repr(exc)}
    # ---- the reference's real-time hardware driver: SSM + GuSTO as a real-time iteration (examples/hardware/diamond_SSM.py:
    # 193, 218, 359-361: n_x = 6, n_u = 4, N = 3, dt = 0.02, max_gusto_iters = 0, replanned every 2 steps = 40 ms)
    try:
        from sofacontrol_amd.scp.models.ssm import SSMGuSTO
        from sofacontrol_amd.scp.gusto import GuSTO
        from sofacontrol_amd.utils import HyperRectangle
        n6, m4, N3, dt2 = 6, 4, 3, 0.02
        mdl = wl.ssm_model(n6, m4, 3, 2, seed=96)
        s6 = SSMDynamics(mdl['z_ref'].copy(), discrete=False, discr_method='be',
                         model=dict(Ts=sc(dt2), w_coeff=mat(mdl['W']), v_coeff=mat(mdl['V']), r_coeff=mat(mdl['R']),
                                    B=mat(mdl['B']), rd_coeff=mat(mdl['Rd']), Bd=mat(mdl['Bd'])),
                         params=dict(state_dim=sc(n6), input_dim=sc(m4), output_dim=sc(n6), SSM_order=sc(2), ROM_order=sc(3)))
        gm6 = SSMGuSTO(s6)
        Qz6 = np.zeros((n6, n6)); Qz6[0, 0] = Qz6[1, 1] = Qz6[2, 2] = 100.0      # x, y, z of the end effector (diamond_SSM.py:322-326)
        R6 = 0.003 * np.eye(m4)
        x06 = np.zeros(n6)
        u6 = np.zeros((N3, m4))
        xi6, _ = s6.rollout(x06, u6, dt2)
        z6 = np.tile(np.array([0.02, -0.01, 0.015, 0, 0, 0.0]), (N3 + 1, 1))
        g6 = GuSTO(gm6, N3, dt2, Qz6, R6, x06, u6, xi6, z=z6, U=HyperRectangle([1500.0] * m4, [0.0] * m4), verbose=0,
                   max_gusto_iters=0, convg_thresh=1e-3, warm_start=True)
        ts6 = []
        for _ in range(30):
            t0 = time.perf_counter()
            g6.solve(x06, u6, xi6, z6, None, None)
            ts6.append(time.perf_counter() - t0)
        ts6.sort()
        # the same loop with the solver state kept between calls (the reference's GuSTO(warm_start=True) default hands the previous solution
        # to its QP solver, locp.py:181): the first QP of a call starts from the previous call's minimiser and multipliers
        tw6 = None
        try:
            g6w = GuSTO(gm6, N3, dt2, Qz6, R6, x06, u6, xi6, z=z6, U=HyperRectangle([1500.0] * m4, [0.0] * m4), verbose=0,
                        max_gusto_iters=0, convg_thresh=1e-3, warm_start=True, keep_solver_state=True)
            tw6 = []
            for _ in range(30):
                t0 = time.perf_counter()
                g6w.solve(x06, u6, xi6, z6, None, None)
                tw6.append(time.perf_counter() - t0)
            tw6.sort()
        except Exception:
            tw6 = None
        cpu6 = 'no compiled twin of this loop (the CPU twin\'s GuSTO is the nearest-point TPWL one)'
        if rank == 0 and world == 1:
            try:      # the reference-shaped CPU path: the numpy statement of the same loop (python loop + numpy, exact KKT solve of the QP)
                from oracle import gusto as ogusto, ssm as ossm
                om = ossm.make_model(n6, m4, 3, 2, mdl['R'], mdl['B'], mdl['W'], mdl['V'], mdl['z_ref'], rd_coeff=mdl['Rd'], Bd=mdl['Bd'])
                def dyn_d6(x, u):
                    return ossm.jacobians(om, x, u, dt2, 'be')
                def dyn_c6(x, u):
                    A, B_, d_ = ossm.continuous_jacobians(om, x, u)
                    return A @ x + B_ @ u + d_, A, B_
                tn6 = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    xo6, uo6, _, tr6 = ogusto.solve_generic(dyn_d6, dyn_c6, np.zeros((n6, n6)), N3, dt2, Qz6, R6, x06, u6, xi6, z=z6,
                                                            U=(np.kron(np.eye(m4), np.array([[1.0], [-1.0]])), np.tile([1500.0, 0.0], m4)),
                                                            obs_lin=lambda x: ossm.observer_jacobians(om, x), convg_thresh=1e-3, max_gusto_iters=0)
                    tn6.append(time.perf_counter() - t0)
                cpu6 = {'what': 'numpy statement of the same loop (oracle.gusto.solve_generic: python loop, exact KKT solve of the QP), one call',
                        'ms': min(tn6) * 1e3, 'max_rel_u_vs_gpu': float(np.abs(uo6 - g6.uopt).max() / max(1e-12, np.abs(uo6).max()))}
            except Exception as exc:
                cpu6 = {'error': repr(exc)}
        out['ssm_gusto_rti'] = {'cpu': cpu6,
                                'workload': 'SSM (n_x = 6, n_u = 4, cubic) + GuSTO real-time iteration with the driver\'s cost (three tip coordinates): N = 3, dt = 0.02, max_gusto_iters = 0 '
                                            '(one QP per call), U box; %s, host buffers' % ('the whole solve in one launch of csrc/gusto_ssm.hip' if getattr(g6, '_ssm', False) else 'host loop around the device QP'),
                                'kernel': g6.kernel_info['kernel'] if getattr(g6, '_ssm', False) else 'host loop + ' + str((g6.locp.kernel_info or {}).get('kernel')),
                                'ms_median': ts6[len(ts6) // 2] * 1e3, 'ms_p95': ts6[int(len(ts6) * 0.95)] * 1e3,
                                'ms_median_keep_solver_state': None if tw6 is None else tw6[len(tw6) // 2] * 1e3,
                                'budget_ms': 40.0, 'within_budget': bool(ts6[int(len(ts6) * 0.95)] * 1e3 <= 40.0)}
    except Exception as exc:
        out['ssm_gusto_rti'] = {'error': repr(exc)}
    # ---- C4 (per-GPU column shard): the local Gramian alone, then the whole sharded POD build of the product
    # (distributed.pod_from_column_shards: Gramian -> reduce-scatter + all-gather over RCCL when world > 1 -> replicated
    # eigen-decomposition -> local mode rows), everything resident in HBM, phases timed separately
    import torch
    from sofacontrol_amd.distributed import pod_from_column_shards
    n_s, n_f = 10000, 50000 // 8
    gen = torch.Generator(device='cuda')
    gen.manual_seed(7 + rank)
    # low rank (64) + 1e-3 noise; the left factor is the same on every rank (it is a property of the
    # snapshots, seed 7), the right factor and the noise are this rank's DoF columns
    gl = torch.Generator(device='cuda')
    gl.manual_seed(7)
    Lr = torch.randn((n_s, 64), dtype=torch.float64, device='cuda', generator=gl) * torch.linspace(40.0, 4.0, 64, dtype=torch.float64, device='cuda')
    S_t = Lr @ torch.randn((64, n_f), dtype=torch.float64, device='cuda', generator=gen)
    S_t += 1e-3 * torch.randn((n_s, n_f), dtype=torch.float64, device='cuda', generator=gen)
    del Lr
    G_t = torch.empty((n_s, n_s), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    sptr, gptr = C.c_void_p(S_t.data_ptr()), C.c_void_p(G_t.data_ptr())
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.srh_event_create(C.byref(e0)); L.srh_event_create(C.byref(e1))
    _lib.check(L.srom_gramian_dev(sptr, C.c_int64(n_s), C.c_int64(n_f), C.c_int64(n_f), gptr, None), 'gramian')
    _lib.sync()
    L.srh_event_record(e0, None)
    _lib.check(L.srom_gramian_dev(sptr, C.c_int64(n_s), C.c_int64(n_f), C.c_int64(n_f), gptr, None), 'gramian')
    L.srh_event_record(e1, None)
    _lib.sync()
    ms = C.c_float()
    L.srh_event_elapsed_ms(e0, e1, C.byref(ms))
    flop = float(n_s) * (n_s + 128) * n_f          # executed: upper triangle of 128 x 128 tiles, 2 flop per MAC
    out['gramian_c4'] = {'workload': 'C4 per-GPU shard: S %d x %d f64, G = S S^T' % (n_s, n_f), 'ms': ms.value,
                         'tflops_executed': flop / (ms.value * 1e-3) / 1e12,
                         'frac_of_f64_mfma_peak': flop / (ms.value * 1e-3) / 1e12 / 78.6}
    if rank == 0:
        try:      # CPU figure beside it: numpy (BLAS dgemm, its own threads) on a 2000-snapshot slice of the same shard shape
            Sc = np.random.default_rng(7).standard_normal((2000, n_f))
            Sc @ Sc[:64].T
            t0 = time.perf_counter()
            Gc = Sc @ Sc.T
            tc = time.perf_counter() - t0
            out['gramian_c4']['cpu'] = {'what': 'numpy S S^T (BLAS dgemm, all BLAS threads) on a 2000 x %d slice' % n_f, 'seconds': tc,
                                        'tflops': 2.0 * 2000 * 2000 * n_f / tc / 1e12,
                                        'gpu_over_cpu': out['gramian_c4']['tflops_executed'] / (2.0 * 2000 * 2000 * n_f / tc / 1e12)}
            del Sc, Gc
        except Exception as exc:
            out['gramian_c4']['cpu'] = {'error': repr(exc)}
    del G_t
    try:
        tm = {}
        pod_from_column_shards(S_t, 1e-4, rom_dim=64, timings=tm, keep_on_device=True, force_torch=True)      # first call: loads rocSOLVER
        tm = {}
        U_loc, k, Sig = pod_from_column_shards(S_t, 1e-4, rom_dim=64, timings=tm, keep_on_device=True, force_torch=True)
        out['pod_build_c4'] = {'workload': 'C4: 10000 snapshots x %d DoF columns per GPU (50000 over 8), %d GPU(s); k = 64 modes kept; '
                                           'S resident in HBM' % (n_f, world), 'world': world,
                               'phases_ms': {kk: (v * 1e3 if isinstance(v, float) else v) for kk, v in tm.items()},
                               'allreduce_payload_bytes': n_s * n_s * 8,
                               'cpu': 'no twin: the build is Gramian (CPU figure under gramian_c4) + eigen-decomposition (LAPACK dsyevd of 10 000 x 10 000 '
                                      'takes minutes on the host: outside the bounded CPU budget of this line)'}
        if dist is not None:          # the one exchange step as every rank saw it
            cs = torch.tensor([tm.get('collective_s', 0.0) * 1e3], dtype=torch.float64, device='cuda')
            call = torch.empty((world,), dtype=torch.float64, device='cuda')
            dist.all_gather_into_tensor(call, cs)
            out['pod_build_c4']['collective_ms_over_ranks'] = {'min': float(call.min()), 'max': float(call.max()), 'per_rank': [float(v) for v in call.cpu()]}
        del U_loc
    except Exception as exc:
        out['pod_build_c4'] = {'error': repr(exc)}
    del S_t
    torch.cuda.empty_cache()
    try:
        out['pod_shapes'] = pod_shapes(L, _lib)
    except Exception as exc:
        out['pod_shapes'] = {'error': repr(exc)}
    if world == 1:
        try:
            out['model_prep'] = model_prep(_lib)
        except Exception as exc:
            out['model_prep'] = {'error': repr(exc)}
    try:
        out['scp_c5'] = scp_c5(_lib, rank, world, dist, cpu=(world == 1 and rank == 0))
        if world == 1:       # what one GPU of an 8-GPU node gets of the 256 rollouts
            out['scp_c5_32_rollouts'] = scp_c5(_lib, 0, 1, None, total=32)
            out['scp_c5_weak'] = dict(out['scp_c5'], note='256 rollouts per rank; at one GPU this IS scp_c5 (same call), listed so that the '
                                                           'N > 1 lines have their N = 1 point')
        else:                # the sharding that can scale -- 256 rollouts PER rank, all_gather of the costs, global best
            out['scp_c5_weak'] = scp_c5(_lib, rank, world, dist, total=256 * world)
    except Exception as exc:
        out['scp_c5'] = {'error': repr(exc)}
    if world == 1:
        try:
            out['scp_c2_r36'] = scp_c2_r36(_lib)
        except Exception as exc:
            out['scp_c2_r36'] = {'error': repr(exc)}
    return out


def rank_environments(n, port=None):
    """The environment of each of the n rank processes (one per GPU of this node, rendezvous on 127.0.0.1)."""
    if port is None:
        import socket
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
    envs = []
    for rk in range(n):
        envs.append({'RANK': str(rk), 'LOCAL_RANK': str(rk), 'WORLD_SIZE': str(n), 'LOCAL_WORLD_SIZE': str(n),
                     'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'HSA_ENABLE_IPC_MODE_LEGACY': '0'})
    return envs


def launch_ranks(n, argv, dry, cmd=None):
    """Start n child processes of this file, one rank per GPU, and wait for them.  The parent never initialises a GPU
    (a process that has must not exec / fork GPU work); rank 0's stdout (the ONE JSON line) is passed through."""
    import subprocess
    if n < 1:
        print('bench.py: --gpus must be >= 1', file=sys.stderr)
        return 2
    envs = rank_environments(n)
    if cmd is None:
        cmd = [sys.executable, os.path.abspath(__file__)] + list(argv)
    if dry:
        print(json.dumps({'dry_launch': True, 'n_ranks': n, 'cmd': cmd, 'env': envs}))
        return 0
    procs = []
    for e in envs:
        procs.append(subprocess.Popen(cmd, env=dict(os.environ, **e), stdout=None if e['RANK'] == '0' else subprocess.DEVNULL))
    rc = 0
    deadline = None
    while procs:
        for p in list(procs):
            r = p.poll()
            if r is None:
                continue
            procs.remove(p)
            if r != 0 and rc == 0:
                rc = r if r > 0 else 1
                deadline = time.time() + 30.0      # a rank died: the others would wait in a collective for ever
        if deadline is not None and time.time() > deadline:
            for p in procs:
                p.kill()                           # exact PIDs of our own children
            for p in procs:
                p.wait()
            break
        time.sleep(0.05)
    return rc


MAX_LINE = 4096      # the driver keeps only a tail of stdout: the LAST line must be small enough to survive whole (round 5 lost a 20 KB line)


def _sig(v, digits=6):
    """Floats to `digits` significant digits (the line is a record, not a checkpoint); containers recursively."""
    if isinstance(v, float):
        return float('%.*g' % (digits, v)) if np.isfinite(v) else None
    if isinstance(v, dict):
        return {k: _sig(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, digits) for x in v]
    if isinstance(v, (np.floating, np.integer)):
        return _sig(v.item(), digits)
    return v


def compact_line(out):
    """The driver's line: the contract keys, `config`, `roofline`, `cpu_baseline` and `parity_sample` trimmed to scalars, and the
    north star's CPU/GPU ratio against each CPU figure it can be read on.  Everything else (`secondary`, the long descriptions)
    stays in the full record that `emit` prints on an EARLIER line and writes to bench_detail.json / bench_secondary.json."""
    keep = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
            'dtype', 'data')
    line = {k: out.get(k) for k in keep}
    if out.get('vs_baseline') is not None:
        line['vs_baseline_definition'] = 'nothing published; = compiled CPU twin (1 core) / GPU, ms per SCP iteration of one C2 rollout'
    cfg = out.get('config', {})
    line['config'] = {k: cfg[k] for k in ('workload', 'rollouts_per_gpu', 'proj_batch', 'proj_launches', 'max_gusto_iters',
                                          'scp_iters_per_step_rank0', 'scp_kernel', 'scp_rollouts_handed_to_fused_kernel',
                                          'solves_not_converged_rank0') if k in cfg}
    rf = out.get('roofline')
    if rf is not None:
        line['roofline'] = {k: rf[k] for k in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'avg_launch_ms',
                                               'algorithmic_bytes_per_launch') if k in rf}
    cb = out.get('cpu_baseline')
    if isinstance(cb, dict) and 'error' in cb:
        line['cpu_baseline'] = {'error': str(cb['error'])[:300]}
    elif isinstance(cb, dict):
        c = {k: cb[k] for k in ('value', 'unit', 'cores', 'kind') if k in cb}
        c['sample'] = cb.get('sample_short', cb.get('sample', ''))[:260]
        c['host'] = cb.get('host', '').split(',')[0][:48]
        st, al, npo, osq = (cb.get(k, {}) for k in ('single_thread', 'all_cores', 'numpy_port', 'osqp_restated_eps1e_5'))
        c['twin_1core_ms_per_it'] = st.get('ms_per_scp_iteration')
        c['numpy_port_it_per_s'] = npo.get('scp_iterations_per_s')
        c['osqp_restated_s_per_qp'] = osq.get('seconds')
        c['osqp_restated_rel_traj_err'] = osq.get('rel_traj_error_vs_exact')
        c['pod_projection_gbs_all_cores'] = cb.get('pod_projection_gbs', {}).get('all_cores')
        g = cb.get('gpu_vs_cpu', {}).get('single_rollout_ms_per_scp_iteration', {})
        gpu_ms = g.get('gpu')
        if gpu_ms:
            # the north star's ">= 10x over the reference CPU solve", read three ways, one rollout at a time and batched
            one = {'gpu_ms_per_it': gpu_ms}
            if npo.get('ms_per_scp_iteration_single'):
                one['vs_numpy_port'] = npo['ms_per_scp_iteration_single'] / gpu_ms
            if osq.get('seconds'):
                one['vs_osqp_restated'] = osq['seconds'] * 1e3 / gpu_ms
            if st.get('ms_per_scp_iteration'):
                one['vs_compiled_twin_1core'] = st['ms_per_scp_iteration'] / gpu_ms
            bat = {}
            if npo.get('scp_iterations_per_s'):
                bat['vs_numpy_port'] = out['value'] / npo['scp_iterations_per_s']
            if osq.get('seconds'):
                bat['vs_osqp_restated'] = out['value'] * osq['seconds']
            if al.get('scp_iterations_per_s'):
                bat['vs_compiled_twin_all_cores'] = out['value'] / al['scp_iterations_per_s']
            c['speedup_one_rollout'] = one
            c['speedup_batched'] = bat
        line['cpu_baseline'] = c
    ps = out.get('parity_sample')
    if isinstance(ps, dict):
        line['parity_sample'] = {k: ps[k] for k in ('max_rel_traj', 'iters_equal', 'rollouts_vs_numpy_oracle', 'max_rel_traj_vs_cpu_twin',
                                                    'iters_equal_vs_cpu_twin', 'rollouts_vs_cpu_twin', 'tolerance') if k in ps}
    line = _sig(line)
    text = json.dumps(line, separators=(',', ':'))
    if len(text) > MAX_LINE:            # never again: shed the optional parts before the contract keys
        for k in ('vs_baseline_definition', 'parity_sample'):
            line.pop(k, None)
            text = json.dumps(line, separators=(',', ':'))
            if len(text) <= MAX_LINE:
                break
    assert len(text) <= MAX_LINE, len(text)
    return text


def emit(out, write_files=True):
    """Full record first (one line, prefixed so that nothing mistakes it for THE line) and into bench_detail.json /
    bench_secondary.json (repo root and gpurun_out/, whichever is writable); the compact line LAST."""
    full = json.dumps(out)
    for d in (ROOT, os.path.join(ROOT, 'gpurun_out')) if write_files else ():
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, 'bench_detail.json'), 'w') as f:
                f.write(full + '\n')
            with open(os.path.join(d, 'bench_secondary.json'), 'w') as f:
                json.dump(out.get('secondary'), f)
        except OSError:
            pass
    print('BENCH_DETAIL ' + full)
    sys.stdout.flush()
    print(compact_line(out))
    sys.stdout.flush()


def _sample_rows(n, row_bytes, budget, seed):
    """All n rows if they fit the byte budget, else a fixed seeded sample of them in ascending order."""
    cap = max(1, budget // row_bytes)
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, size=cap, replace=False))


def dump_outputs(path, proj, xopt, uopt, zopt, iters, status):
    """--dump-outputs: what a caller of the timed path receives from its last step, float64, as <path>/<name>.npy -- the reduced
    states of the projection (B x r) and, per rollout, the solution xopt / uopt / zopt, the SCP iteration count and the status.
    Where the rows outgrow their budget (< 48 MB in all) a fixed seeded sample is written, with its row indices beside it."""
    os.makedirs(path, exist_ok=True)
    R_ = xopt.shape[0]
    pi = _sample_rows(proj.shape[0], proj[0].nbytes, 24 << 20, seed=1)
    ri = _sample_rows(R_, xopt[0].nbytes + uopt[0].nbytes + zopt[0].nbytes, 16 << 20, seed=2)
    si = _sample_rows(R_, 16, 4 << 20, seed=3)
    arrays = {'proj_reduced_states': proj[pi], 'proj_rows': pi, 'xopt': xopt[ri], 'uopt': uopt[ri], 'zopt': zopt[ri], 'solution_rollouts': ri,
              'scp_iterations': iters[si], 'status': status[si], 'status_rollouts': si}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + '.npy'), np.ascontiguousarray(a, dtype=np.float64))


def stub_main(args, rank, world):
    """SRH_BENCH_STUB_DEVICE=1: the multi-rank skeleton of this file WITHOUT a GPU -- gloo instead of RCCL, a seeded stand-in
    for the solve -- so that the launcher, the 127.0.0.1 rendezvous, the barrier-bracketed timing with its max over ranks,
    the reduction step of the sharded rollout batch and rank-0-only printing run for real on a CPU box
    (tests/test_bench_contract_cpu.py).  SRH_BENCH_STUB_FAIL_RANK=k makes rank k die before the first collective.
    Never a measurement: the line says "stub": true and carries no value."""
    import torch
    import torch.distributed as dist
    from sofacontrol_amd.distributed import gather_rollout_costs, shard_range
    if os.environ.get('SRH_BENCH_STUB_FAIL_RANK') == str(rank):
        print('bench.py (stub): rank %d exits before the rendezvous, as told' % rank, file=sys.stderr)
        raise SystemExit(3)
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    lo, hi = shard_range(256, rank, world)
    J = 100.0 + np.random.default_rng(11).standard_normal(256)
    for _ in range(args.steps):
        time.sleep(0.01 * (rank + 1))
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    J_all, best = gather_rollout_costs(J[lo:hi].copy(), 256)
    per_rank = [elapsed]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        allt = torch.empty((world,), dtype=torch.float64)
        dist.all_gather_into_tensor(allt, t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, per_rank = float(t[0]), [float(v) for v in allt]
    if rank == 0 and os.environ.get('SRH_BENCH_STUB_RECORD'):
        # the printing path of a real run, fed with a recorded full record (a committed profiles/*_bench.log): what the driver's
        # tail of stdout would hold -- tests/test_bench_contract_cpu.py checks that the last line parses alone and is < MAX_LINE
        lines = [l for l in open(os.environ['SRH_BENCH_STUB_RECORD']) if l.startswith(('{"metric"', 'BENCH_DETAIL '))]
        rec = json.loads(lines[-1].split(' ', 1)[1] if lines[-1].startswith('BENCH_DETAIL ') else lines[-1])
        if lines[-1].startswith('{"metric"') and len(lines) > 1 and lines[-2].startswith('BENCH_DETAIL '):
            rec = json.loads(lines[-2].split(' ', 1)[1])
        rec['stub'] = True
        emit(rec, write_files=False)
    elif rank == 0:
        print(json.dumps({'stub': True, 'metric': 'none (SRH_BENCH_STUB_DEVICE=1: launcher / rendezvous / reduction skeleton only)', 'value': None,
                          'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': elapsed / max(1, args.steps) * 1e3,
                          'ms_per_step_per_rank': [v / max(1, args.steps) * 1e3 for v in per_rank],
                          'best_rollout': best, 'best_is_global_argmin': bool(best == int(np.argmin(J))), 'costs_gathered': int(J_all.size)}))
    if world > 1:
        dist.destroy_process_group()


def parse_args(argv=None):
    """The command line and what it decides: a plain run measures the headline only -- no CPU baselines, no secondary metrics,
    and the GuSTO constructor's own solve at the cap of the timed calls (`first_solve_cap`) instead of the reference-default 500
    SCP iterations, whose throughput only `--full` reports (`secondary.scp_uncapped_500`)."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rollouts', type=int, default=4096, help='independent SCP rollouts per GPU per step')
    ap.add_argument('--proj-batch', type=int, default=65536, help='snapshots per GPU in the POD projection batch')
    ap.add_argument('--proj-launches', type=int, default=4, help='projection launches per step')
    ap.add_argument('--max-gusto-iters', type=int, default=5,
                    help='GuSTO iteration cap per solve (the reference default is 500; its real-time drivers use 0-5)')
    ap.add_argument('--full', action='store_true',
                    help='also the secondary metrics, the layout A/B, the CPU baselines with the parity sample and the detail files '
                         '(off: the headline figure only)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baselines and the parity sample')
    ap.add_argument('--no-secondary', action='store_true', help='with --full: skip the secondary metrics (iLQR C3, Gramian C4, ...)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (rank 0; seeded sample of the rollouts) as DIR/<name>.npy')
    ap.add_argument('--dry-launch', action='store_true',
                    help='with --gpus N > 1 and no WORLD_SIZE: print the per-rank environments / command lines and exit (no GPU call)')
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error('--steps must be >= 1')
    if not args.full:
        args.no_cpu_baseline = args.no_secondary = True
    args.first_solve_cap = None if args.full else args.max_gusto_iters
    return args


def main():
    args = parse_args()

    # `python bench.py --gpus N` on its own (no torch.distributed.run around it): this process is only a launcher.  It
    # starts N fresh rank processes of this file BEFORE anything touches a GPU (no torch.cuda.*, no _lib.lib()), waits,
    # and exits non-zero if any rank failed.  Under torch.distributed.run (WORLD_SIZE set) it is a rank already.
    if 'WORLD_SIZE' not in os.environ and (args.gpus > 1 or args.dry_launch):
        raise SystemExit(launch_ranks(args.gpus, [a for a in sys.argv[1:] if a != '--dry-launch'], args.dry_launch))
    if 'WORLD_SIZE' in os.environ and int(os.environ['WORLD_SIZE']) != args.gpus:
        print('bench.py: --gpus %d but WORLD_SIZE=%s: the launcher\'s world size is used' % (args.gpus, os.environ['WORLD_SIZE']),
              file=sys.stderr)

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if os.environ.get('SRH_BENCH_STUB_DEVICE') == '1':
        return stub_main(args, rank, world)
    dist = None
    # torch (device memory for the RCCL collective, C4 secondary) brings its own HIP runtime: it has to initialise
    # before the first call into libsofacontrol_hip
    import torch
    torch.cuda.set_device(local_rank)
    torch.cuda.init()
    if world > 1 or os.environ.get('SRH_FORCE_DIST') == '1':
        import torch.distributed as dist
        try:        # bind the process group to this rank's GPU (no device guessing from the global rank in barrier / the first collective)
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local_rank))
        except TypeError:
            dist.init_process_group('nccl', rank=rank, world_size=world)

    import workloads as wl
    from sofacontrol_amd import _lib
    from sofacontrol_amd.mor.pod import POD
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    from scipy.interpolate import interp1d

    if _lib.device_count() < 1:
        raise SystemExit('bench.py needs a GPU: libsofacontrol_hip.so has no CPU fallback')
    _lib.set_device(local_rank)
    L = _lib.lib()

    w = wl.diamond_c2()
    N, m, r, dt = w['N'], w['m'], w['r'], w['dt']
    n, nz, n_f = 2 * r, 6, w['U'].shape[0]
    R_, B = args.rollouts, args.proj_batch
    rom = POD(dict(U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    tp, gm = build_model(w)
    xc, fc = gm.get_characteristic_vals()

    # ---- resident inputs (each rank its own shard: seeds offset by the rank)
    X = wl.snapshots(w['q_ref'], B, seed=2 + 1000 * rank)
    dX = _lib.DeviceBuffer.from_array(X)
    dXr = _lib.DeviceBuffer(B * r * 8)
    # initial reduced states of the rollouts: x0 = [0 ; U^T (q - q_ref)] of the first R snapshots
    q0 = rom.compute_RO_state(qf=X[:R_])
    x0 = np.concatenate((np.zeros((R_, r)), q0), axis=1)
    del X
    u_init = np.zeros((R_, N, m))
    x_init, _ = tp.rollout(x0, u_init, dt)
    zi = interp1d(w['t'], w['z'], axis=0, bounds_error=False, fill_value=(w['z'][0], w['z'][-1]))
    phase = (np.arange(R_) + R_ * rank) * (10.0 / max(1, R_ * world))
    z = np.stack([zi(phase[b] + dt * np.arange(N + 1)) for b in range(R_)])
    _lib.sync()
    t_ctor = time.perf_counter()
    gusto = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']),
                  X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, batch=R_, max_trace=0,
                  max_gusto_iters=args.max_gusto_iters, first_solve_cap=args.first_solve_cap)
    t_ctor = time.perf_counter() - t_ctor
    # with --full the constructor solves with the reference's default cap of 500 SCP iterations (gusto.py:142-147): its throughput
    # is reported next to the capped (real-time iteration) headline; host buffers + plan creation inside this wall time.  A plain
    # run caps that solve like the timed ones (solves are independent: the timed launches compute the same either way).
    uncapped = None
    if args.full:
        uncapped = {'what': 'GuSTO constructor: plan creation + one solve of the %d rollouts at the reference-default cap of 500 SCP '
                            'iterations (trust-region-active QPs included), host buffers' % R_,
                    'seconds': t_ctor, 'scp_iterations': int(gusto.iters.sum()), 'max_iterations_of_a_rollout': int(gusto.iters.max()),
                    'scp_iterations_per_s': float(gusto.iters.sum()) / t_ctor, 'not_converged': int((gusto.status != 0).sum())}
    if uncapped is not None and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:      # the same uncapped solve on the host, all usable cores, bounded sample (the first 64 rollouts)
            from oracle import cpu_twin
            ncpu, nb = usable_cpus(), min(64, R_)
            t0 = time.perf_counter()
            _, _, itu, _ = cpu_twin.gusto_solve(dict(w['tab'], w_q=1.0, w_v=0.0), w['Ad'], w['Bd'], w['dd'], w['H'], N, dt, w['Qz'], w['R'], x0[:nb],
                                                u_init[:nb], x_init[:nb], z=z[:nb], U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']), x_char=xc, f_char=fc,
                                                convg_thresh=1e-3, max_gusto_iters=500, threads=ncpu, algo='condensed')
            tu = time.perf_counter() - t0
            uncapped['cpu'] = {'what': 'native CPU twin, same algorithm, first %d rollouts uncapped on %d threads' % (nb, ncpu), 'seconds': tu,
                               'scp_iterations_per_s': float(itu.sum()) / tu, 'iterations_equal_gpu': bool((itu == gusto.iters[:nb]).all()),
                               'gpu_over_cpu_throughput': uncapped['scp_iterations_per_s'] / (float(itu.sum()) / tu)}
        except Exception as exc:
            uncapped['cpu'] = {'error': repr(exc)}
    gusto.max_gusto_iters = args.max_gusto_iters
    _lib.check(L.sgusto_plan_set_max_iters(gusto.plan, C.c_int(args.max_gusto_iters)), 'set_max_iters')
    d = {k: _lib.DeviceBuffer.from_array(v) for k, v in dict(x0=x0, u_init=u_init, x_init=x_init, z=z).items()}
    o = dict(xopt=_lib.DeviceBuffer(R_ * (N + 1) * n * 8), uopt=_lib.DeviceBuffer(R_ * N * m * 8),
             zopt=_lib.DeviceBuffer(R_ * (N + 1) * nz * 8), iters=_lib.DeviceBuffer(R_ * 4), status=_lib.DeviceBuffer(R_ * 4))
    ev = [C.c_void_p() for _ in range(2 * args.proj_launches)]
    for e in ev:
        _lib.check(L.srh_event_create(C.byref(e)), 'event')

    def step(timed):
        """One pass of the hot path over one batch, everything resident: POD projection of the snapshot batch -> reduced
        states x0 = [0 ; q_r] of the first R rows (utils.qv2x) -> zero-input TPWL rollout = the initial guess of the solve
        (scp/ros.py:78-79) -> the receding-horizon SCP solves.  Nothing visits the host in between."""
        for i in range(args.proj_launches):
            if timed:
                L.srh_event_record(ev[2 * i], None)
            _lib.check(L.srom_project_dev(rom.handle, 0, dX.ptr, C.c_int64(B), C.c_int64(n_f), dXr.ptr, C.c_int64(r), None), 'project')
            if timed:
                L.srh_event_record(ev[2 * i + 1], None)
        _lib.check(L.srom_qv2x_dev(dXr.ptr, C.c_int64(r), None, C.c_int64(0), C.c_int64(R_), C.c_int(r), d['x0'].ptr, C.c_int64(n), None), 'qv2x')
        _lib.check(L.stpwl_rollout_dev(tp.handle_for(dt), d['x0'].ptr, d['u_init'].ptr, C.c_int(N), C.c_int64(R_), d['x_init'].ptr, None, None),
                   'rollout')
        _lib.check(L.sgusto_plan_solve_dev(gusto.plan, d['x0'].ptr, d['u_init'].ptr, d['x_init'].ptr, d['z'].ptr, None, None,
                                           o['xopt'].ptr, o['uopt'].ptr, o['zopt'].ptr, o['iters'].ptr, o['status'].ptr,
                                           None, None), 'gusto')

    def barrier():
        _lib.sync()
        if dist is not None:
            dist.barrier()
        _lib.sync()

    for _ in range(args.warmup):
        step(False)
    barrier()
    proj_ms = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
        _lib.sync()
        for i in range(args.proj_launches):
            ms = C.c_float()
            L.srh_event_elapsed_ms(ev[2 * i], ev[2 * i + 1], C.byref(ms))
            proj_ms.append(ms.value)
    barrier()
    elapsed = time.perf_counter() - t0
    iters = o['iters'].to_array((R_,), dtype=np.int32)
    status = o['status'].to_array((R_,), dtype=np.int32)
    kinfo = gusto.kernel_info          # the instantiation the timed launches ran + rollouts handed to the fused kernel in the last one
    n_par = min(R_, 512)         # the rollouts the CPU side may solve as well: GPU trajectories kept for `parity_sample`
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dXr.to_array((B, r)), o['xopt'].to_array((R_, N + 1, n)), o['uopt'].to_array((R_, N, m)),
                     o['zopt'].to_array((R_, N + 1, nz)), iters, status)
    if not args.no_cpu_baseline:
        gx = o['xopt'].to_array((R_, N + 1, n))[:n_par].copy()
        gu = o['uopt'].to_array((R_, N, m))[:n_par].copy()
    it_per_step = int(iters.sum())
    total_iters = it_per_step * args.steps
    per_rank_ms = [elapsed / args.steps * 1e3]
    if dist is not None:
        import torch
        t = torch.tensor([elapsed, float(total_iters)], dtype=torch.float64, device='cuda')
        allt = torch.empty((world,), dtype=torch.float64, device='cuda')
        dist.all_gather_into_tensor(allt, t[:1].clone())
        per_rank_ms = [float(v) / args.steps * 1e3 for v in allt.cpu()]
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        elapsed = float(tmax[0])
        total_iters = float(t[1])
    sec = None
    if not args.no_secondary:
        try:
            # per-step latencies BEFORE anything large is freed: after a hipFree of GB-sized buffers the HIP runtime
            # serves small synchronous calls ~100 us slower for the rest of the process (observed, ROCm 7.2)
            cl = closed_loop_latency(w, rom, tp) if rank == 0 else None
            single = scp_single_rollout(w, gm, tp, xc, fc, x0, x_init, z, args.max_gusto_iters) if rank == 0 else None
            # the closed-loop horizons of the reference's drivers too (latency series: taken with the other per-step latencies)
            horizons = scp_reference_horizons() if rank == 0 else None
        except Exception as exc:
            cl, single, horizons = {'error': repr(exc)}, None, None
        layout_ab = None
        if rank == 0 and world == 1:
            # the SCP launch of the timed step with the OTHER lean layout (SRH_LEAN_HALF read at plan creation): the full-size workgroup
            # (512 threads, 160 KB, one rollout per CU) beside the half-size one the plan picks for batches above the CU count
            try:
                def scp_ms(plan, reps=3):
                    ts = []
                    for _ in range(reps):
                        _lib.sync()
                        t0 = time.perf_counter()
                        _lib.check(L.sgusto_plan_solve_dev(plan, d['x0'].ptr, d['u_init'].ptr, d['x_init'].ptr, d['z'].ptr, None, None,
                                                           o['xopt'].ptr, o['uopt'].ptr, o['zopt'].ptr, o['iters'].ptr, o['status'].ptr, None, None), 'gusto')
                        _lib.sync()
                        ts.append(time.perf_counter() - t0)
                    return min(ts[1:]) * 1e3
                ms_this = scp_ms(gusto.plan)
                it_this = int(o['iters'].to_array((R_,), dtype=np.int32).sum())
                prev = os.environ.get('SRH_LEAN_HALF')
                other_half = 0 if kinfo['lean'] and kinfo['lean'][3] == kinfo['lean'][4] else 1
                os.environ['SRH_LEAN_HALF'] = str(other_half)
                try:
                    g2 = GuSTO(gm, N, dt, w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']), X=Polyhedron(w['XA'], w['Xb']),
                               x_char=xc, f_char=fc, convg_thresh=1e-3, batch=R_, max_trace=0, max_gusto_iters=args.max_gusto_iters,
                               first_solve_cap=args.max_gusto_iters)
                finally:
                    if prev is None:
                        os.environ.pop('SRH_LEAN_HALF', None)
                    else:
                        os.environ['SRH_LEAN_HALF'] = prev
                ms_other = scp_ms(g2.plan)
                it_other = int(o['iters'].to_array((R_,), dtype=np.int32).sum())
                k2 = g2.kernel_info
                layout_ab = {'what': 'sgusto_plan_solve_dev of the %d rollouts alone (no projection), best of 2 after a warm-up call, same inputs: the layout the '
                                     'plan picked against the other one' % R_,
                             'picked': {'kernel': kinfo['kernel'], 'threads': kinfo.get('threads'), 'lds_bytes': kinfo.get('lds_bytes_lean'), 'ms': ms_this,
                                        'scp_iterations_per_s': it_this / (ms_this * 1e-3)},
                             'other': {'kernel': k2['kernel'], 'threads': k2.get('threads'), 'lds_bytes': k2.get('lds_bytes_lean'), 'ms': ms_other,
                                       'scp_iterations_per_s': it_other / (ms_other * 1e-3)},
                             'scp_iterations_equal': bool(it_this == it_other), 'picked_over_other': ms_other / ms_this}
                del g2
            except Exception as exc:
                layout_ab = {'error': repr(exc)}
        for b in list(d.values()) + list(o.values()) + [dX, dXr]:
            b.free()
        try:
            sec = secondary(L, _lib, rank, world, dist)
            if layout_ab is not None:
                sec['scp_lean_layout_ab'] = layout_ab
            if cl is not None:
                sec['closed_loop_step'] = cl
            if single is not None:
                sec['scp_single_rollout'] = single
            if horizons is not None:
                sec['scp_reference_horizons'] = horizons
        except Exception as exc:      # never lose the headline line to a secondary measurement
            sec = {'error': repr(exc)}
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    alg_bytes = B * n_f * 8 + n_f * r * 8 + n_f * 8 + B * r * 8
    # HBM traffic of the same kernel at the same shape from PMC counters (separate rocprofv3 --pmc passes,
    # corrected as MI355X_MICROARCH.md prescribes; summary committed under profiles/)
    traffic, traffic_source = None, None
    for name in ('r06_proj_pmc.json', 'r05_proj_pmc.json', 'r04_proj_pmc.json', 'r03_proj_pmc.json', 'r02_proj_pmc.json'):
        try:
            pmc = json.load(open(os.path.join(ROOT, 'profiles', name)))
            if pmc.get('algorithmic_bytes_per_launch') == alg_bytes:
                traffic = pmc['traffic_bytes_per_launch']
                traffic_source = 'profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same kernel and shape; not measured in this run)' % name
                break
        except Exception:
            pass
    avg_ms = float(np.mean(proj_ms))
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    out = {
        'metric': 'SCP iterations/sec (Diamond r=30 H=50) + POD projection GB/s vs HBM roofline',
        'value': total_iters / elapsed, 'unit': 'SCP iterations/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': elapsed / args.steps * 1e3, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic', 'ms_per_step_per_rank': per_rank_ms,
        'config': {'workload': 'C2: Diamond n_f=4884, POD r=30 (n_x=60, n_u=4), TPWL P=64 nn/zoh, SCP horizon N=50 '
                               'dt=0.05, U box + X box, figure-8 target; %d independent receding-horizon rollouts per GPU '
                               'per step + POD projection of %d snapshots x %d launches' % (R_, B, args.proj_launches),
                   'rollouts_per_gpu': R_, 'proj_batch': B, 'proj_launches': args.proj_launches, 'max_gusto_iters': args.max_gusto_iters, 'scp_iters_per_step_rank0': it_per_step,
                   'scp_kernel': kinfo['kernel'], 'scp_rollouts_handed_to_fused_kernel': kinfo['handed_over'],
                   'solves_not_converged_rank0': int((status != 0).sum())},
        'roofline': {'kernel': 'proj_kernel (srom_project_dev)', 'bound': 'hbm', 'achieved': achieved,
                     'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': achieved / HBM_PEAK_GBS, 'traffic': traffic,
                     'avg_launch_ms': avg_ms, 'algorithmic_bytes_per_launch': alg_bytes, 'traffic_source': traffic_source},
    }
    if sec is not None and isinstance(sec, dict) and uncapped is not None:
        sec['scp_uncapped_500'] = uncapped
    if world == 1 and not args.no_cpu_baseline:
      try:
        out['cpu_baseline'], sols, np_sols = cpu_baseline(w, x0, x_init, z, xc, fc, n_roll=R_, proj_rows=4096,
                                                          max_iters=args.max_gusto_iters)
        rel = lambda a, b: float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))
        n_par = min(n_par, len(sols))
        out['parity_sample'] = {
            'what': 'trajectories and SCP iteration counts of the timed GPU launch vs the numpy oracle (oracle.gusto around '
                    'oracle.riccati_ipm; first %d rollouts) and vs the native CPU twin (condensed algorithm; first %d rollouts) on the '
                    'same inputs' % (len(np_sols), n_par),
            'kernel_variant': list(gusto.variant), 'kernel_info': kinfo, 'rollouts_vs_numpy_oracle': len(np_sols), 'rollouts_vs_cpu_twin': n_par,
            'max_rel_traj': max(max(rel(gx[b], np_sols[b][0]), rel(gu[b], np_sols[b][1])) for b in range(len(np_sols))),
            'iters_equal': bool(all(int(iters[b]) == np_sols[b][2] for b in range(len(np_sols)))),
            'max_rel_traj_vs_cpu_twin': max(max(rel(gx[b], sols[b][0]), rel(gu[b], sols[b][1])) for b in range(n_par)),
            'iters_equal_vs_cpu_twin': bool(all(int(iters[b]) == sols[b][2] for b in range(n_par))), 'tolerance': 1e-4}
        cb = out['cpu_baseline']
        if sec is not None and 'scp_single_rollout' in sec:
            g1 = sec['scp_single_rollout']
            cb['gpu_vs_cpu'] = {'what': 'both sides run the same algorithm (condensed interior point; Riccati for trust-region-active QPs)',
                                'throughput_vs_all_cores': out['value'] / cb['value'],
                                'throughput_vs_single_thread': out['value'] / cb['single_thread']['scp_iterations_per_s'],
                                'single_rollout_ms_per_scp_iteration': {'gpu': g1['ms_per_scp_iteration'],
                                                                        'cpu_single_thread': cb['single_thread']['ms_per_scp_iteration'],
                                                                        'ratio': cb['single_thread']['ms_per_scp_iteration'] / g1['ms_per_scp_iteration'],
                                                                        'cpu_riccati_single_thread': cb['riccati_single_thread']['ms_per_scp_iteration']}}
            # BASELINE.md holds no published number for this metric (the reference reports none): following the round-2 review,
            # vs_baseline = the north star's own ratio -- wall clock of ONE SCP iteration of one Diamond solve on the CPU (one
            # core, same algorithm) over the same on one MI355X (one rollout at a time, host buffers)
            out['vs_baseline'] = cb['gpu_vs_cpu']['single_rollout_ms_per_scp_iteration']['ratio']
            out['vs_baseline_definition'] = ('no published reference number exists (BASELINE.md); this is CPU-twin ms per SCP iteration (one core, '
                                             'condensed algorithm = the GPU kernel\'s) / GPU ms per SCP iteration, one Diamond C2 rollout at a time')
      except Exception as exc:            # never lose the headline line to the CPU leg
        out['cpu_baseline'] = {'error': repr(exc)}
    if sec is not None:
        out['secondary'] = sec
    emit(out, write_files=args.full)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
