"""CPU: the batched closed-loop surface exists -- every sgusto_loop_* entry point and the two additive plan accessors declared in
include/sofacontrol_hip.h and exported by the built library, scp.closed_loop.ClosedLoopBatch / schedule with the stated signatures --
and the host-only parts answer without a GPU: the schedule (numpy statement, direct statement and the library's own, bit for bit) and
the n_keep * dt_sim > N * dt refusal."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import cl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOOP_SYMBOLS = ['sgusto_loop_create', 'sgusto_loop_destroy', 'sgusto_loop_set_target', 'sgusto_loop_set_feedback', 'sgusto_loop_reset',
                'sgusto_loop_run', 'sgusto_loop_last_inputs', 'sgusto_loop_last_plan', 'sgusto_loop_advance', 'sgusto_loop_stats',
                'sgusto_loop_schedule', 'sgusto_plan_costs_dev', 'sgusto_plan_dims']


def test_loop_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in LOOP_SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^typedef struct sgusto_loop sgusto_loop_t;', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_loop_create\s*\(sgusto_loop_t \*\*out, sgusto_plan_t \*plan, stpwl_t \*planner_model, stpwl_t \*plant, '
                     r'double dt_sim, int n_keep,\s*int64_t max_steps_per_run\)', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_plan_costs_dev\s*\(sgusto_plan_t \*plan, double \*J_dev, void \*stream\)', src, flags=re.M)


def test_python_surface():
    from sofacontrol_amd.scp import closed_loop
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch, schedule
    params = list(inspect.signature(ClosedLoopBatch.__init__).parameters)
    assert params[:10] == ['self', 'gusto', 'plant', 'dt_sim', 'n_keep', 't', 'z', 'u', 'phase', 'K']
    sig = inspect.signature(ClosedLoopBatch.__init__).parameters
    assert all(sig[p].default is None for p in ('t', 'z', 'u', 'phase', 'K'))
    assert list(inspect.signature(ClosedLoopBatch.reset).parameters) == ['self', 'x0', 't_start']
    assert inspect.signature(ClosedLoopBatch.reset).parameters['t_start'].default == 0.0
    run = inspect.signature(ClosedLoopBatch.run).parameters
    assert list(run) == ['self', 'periods', 'W', 'record_x'] and run['W'].default is None and run['record_x'].default is True
    for m in ('step', 'last_inputs', 'last_plan', 'stats', '_advance'):
        assert callable(getattr(ClosedLoopBatch, m))
    assert callable(schedule) and closed_loop.schedule is schedule
    res = closed_loop.ClosedLoopResult(*range(7))
    assert (res.x, res.z, res.u, res.iters, res.status, res.J, res.t) == tuple(range(7))


@pytest.mark.parametrize('dt_sim,n_keeps', [(0.05, (1, 12, 10)), (0.01, (1, 60, 10)), (0.03, (1, 20, 10, 7))])
def test_schedule_equals_the_direct_statement_and_the_library(dt_sim, n_keeps):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import schedule
    N, dt = cc.N, cc.DT
    for n_keep in n_keeps:
        for t_start in (0.0, 0.1, 1.7):
            seen = set()
            for k in range(50):
                s = schedule(N, dt, dt_sim, n_keep, t_start, k)
                t_k, idx0, j, theta = cc.direct_schedule(N, dt, dt_sim, n_keep, t_start, k)
                lt, li, lj, lth = _lib.gusto_loop_schedule(N, dt, dt_sim, n_keep, t_start, k)
                assert s.t_k == t_k == lt and s.idx0 == idx0 == li, (n_keep, t_start, k)
                np.testing.assert_array_equal(s.j, j); np.testing.assert_array_equal(lj, j)
                assert s.theta.tobytes() == theta.tobytes() == lth.tobytes()
                assert 0 <= idx0 <= N and (j >= 0).all() and (j <= N - 1).all() and (theta >= 0).all() and (theta <= 1.0 + 1e-12).all()
                seen.add(idx0)
            assert 0 in seen and len(seen) >= 2


def test_the_period_skeleton_and_the_record_copies_are_stated_once():
    """The prepare kernel has one launch in csrc/, and neither loop unit copies a record back itself: both live in the shared host shell."""
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    assert sum(u.count('loop_prepare_kernel<<<') for u in units.values()) == 1
    for f in ('gusto_loop.hip', 'gusto_ssm_loop.hip'):
        calls = re.findall(r'hipMemcpyAsync\(.*?\);', units[f], flags=re.S)
        assert not [c for c in calls if 'hipMemcpyDeviceToHost' in c], f
        assert 'hipStreamCreateWithFlags' not in units[f], f
    assert sum(u.count('hipStreamCreateWithFlags') for f, u in units.items() if f.startswith('gusto_loop') or f == 'gusto_ssm_loop.hip') == 1


def test_the_plant_step_and_the_plan_point_are_stated_once():
    """The staged plant step lives in tpwl_dev.h alone -- its 16-byte copy and its slice product -- no kernel that steps a TPWL plant forms
    a panel address itself, and the plan point's interpolation is written in one file.  (pod.hip has a two-double vector type of its own
    for the POD products: it includes none of the TPWL headers.)"""
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    holding = lambda text: sorted(f for f, u in units.items() if text in u)
    assert [f for f in holding('ext_vector_type(2)') if f != 'pod.hip'] == ['tpwl_dev.h']
    assert holding('At[q * n + j]') == ['tpwl_dev.h']
    kernels_of_tpwl = units['tpwl.hip'].split('std::vector<double> transpose_batch')[0]
    assert '__global__' in kernels_of_tpwl and 'rollout_staged_kernel' in kernels_of_tpwl
    for f, text in (('gusto_loop.hip', units['gusto_loop.hip']), ('rompc_loop.hip', units['rompc_loop.hip']), ('lqr.hip', units['lqr.hip']),
                    ('tpwl.hip', kernels_of_tpwl)):
        assert 'AdT +' not in text and 'BdT +' not in text, f
    assert holding('th * (hi - lo)') == ['gusto_loop_prep.h']
    for f in ('stage_copy16', 'panel_copy16', 'rl_panel_copy16'):
        assert not holding(f), f


def test_refusals_on_the_host():
    """Argument checks that come before any device call."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    fused = types.SimpleNamespace(_fused=True, _ssm=False, N=12, dt=0.05, batch=3)
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.61 exceeds the horizon N \* dt = 0\.6'):
        ClosedLoopBatch(fused, None, 0.01, 61)
    for bad in (types.SimpleNamespace(_fused=True, _ssm=True, N=12, dt=0.05), types.SimpleNamespace(_fused=False, _ssm=False, N=12, dt=0.05)):
        with pytest.raises(RuntimeError, match='fused resident plan'):
            ClosedLoopBatch(bad, None, 0.01, 10)
    lib = _lib.lib()
    assert lib.sgusto_loop_create(None, None, None, None, C.c_double(0.01), C.c_int(10), C.c_int64(100)) == -1 and b'sgusto_loop_create' in lib.srh_last_error()
    assert lib.sgusto_loop_run(None, C.c_int(1), None, None, None, None, None, None, None) == -1 and b'sgusto_loop_run' in lib.srh_last_error()
    assert lib.sgusto_plan_dims(None, None, None, None, None, None, None, None) == -1 and b'sgusto_plan_dims' in lib.srh_last_error()
    assert lib.sgusto_plan_costs_dev(None, None, None) == -1 and b'sgusto_plan_costs_dev' in lib.srh_last_error()
