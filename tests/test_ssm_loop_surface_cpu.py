"""CPU: the surface of the batched SSM closed loop exists -- every sgusto_ssm_loop_* entry point, sssm_rollout_dev and the two additive
SSM plan accessors declared in include/sofacontrol_hip.h and exported by the built library, scp.closed_loop_ssm.SSMClosedLoopBatch with the
stated signature -- and the refusals that come before any device call answer without a GPU.  The schedule is closed_loop.schedule: the
module states no second one."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ['sgusto_ssm_loop_create', 'sgusto_ssm_loop_destroy', 'sgusto_ssm_loop_set_target', 'sgusto_ssm_loop_reset', 'sgusto_ssm_loop_run',
           'sgusto_ssm_loop_last_inputs', 'sgusto_ssm_loop_last_plan', 'sgusto_ssm_loop_stats', 'sgusto_ssm_loop_advance', 'sssm_rollout_dev',
           'sgusto_ssm_plan_dims', 'sgusto_ssm_plan_costs_dev']


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^typedef struct sgusto_ssm_loop sgusto_ssm_loop_t;', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_ssm_plan_costs_dev\s*\(sgusto_ssm_plan_t \*plan, double \*J_dev, void \*stream\)', src, flags=re.M)
    assert re.search(r'^int\s+sssm_rollout_dev\s*\(sssm_t \*h, const double \*x0_dev, const double \*U_dev, int N, int64_t batch, int mode, double dt, '
                     r'double \*X_dev,\s*double \*Z_dev, void \*stream\)', src, flags=re.M)


def test_python_surface_and_the_one_schedule():
    from sofacontrol_amd.scp import closed_loop, closed_loop_ssm
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    sig = inspect.signature(SSMClosedLoopBatch.__init__).parameters
    assert list(sig) == ['self', 'gusto', 'plant', 'dt_sim', 'n_keep', 't', 'z', 'u', 'phase', 'observe', 'max_steps_per_run']
    assert all(sig[p].default is None for p in ('t', 'z', 'u', 'phase', 'max_steps_per_run')) and sig['observe'].default is True
    rs = inspect.signature(SSMClosedLoopBatch.reset).parameters
    assert list(rs) == ['self', 'x0', 't_start', 'v0'] and rs['t_start'].default == 0.0 and rs['v0'].default is None
    run = inspect.signature(SSMClosedLoopBatch.run).parameters
    assert list(run) == ['self', 'periods', 'W', 'V', 'record_x'] and run['W'].default is None and run['V'].default is None
    assert run['record_x'].default is True
    for m in ('step', 'last_inputs', 'last_plan', 'stats'):
        assert callable(getattr(SSMClosedLoopBatch, m))
    # the schedule used is the TPWL loop's: the same function object, and no second statement in the module or in the new unit
    assert closed_loop_ssm.schedule is closed_loop.schedule
    assert 'def schedule' not in inspect.getsource(closed_loop_ssm)
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    assert sum(u.count('int sgusto_loop_schedule') for u in units.values()) == 1 and 'sgusto_loop_schedule' not in units['gusto_ssm_loop.hip']
    # the original loop still refuses SSM plans
    with pytest.raises(RuntimeError, match='fused resident plan'):
        closed_loop.ClosedLoopBatch(types.SimpleNamespace(_fused=True, _ssm=True, N=3, dt=0.02), None, 0.02, 2)


def test_refusals_on_the_host():
    """Argument checks that come before any device call."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    for bad in (types.SimpleNamespace(_fused=True, _ssm=False, N=3, dt=0.02), types.SimpleNamespace(_fused=False, N=3, dt=0.02)):
        with pytest.raises(RuntimeError, match='SSM plan is resident'):
            SSMClosedLoopBatch(bad, None, 0.02, 2)
    with pytest.raises(RuntimeError, match=r'4 input-rate rows \(dU\).*status -78'):
        SSMClosedLoopBatch(types.SimpleNamespace(_fused=True, _ssm=True, _rate_rows=4, N=3, dt=0.02), None, 0.02, 2)
    plain = types.SimpleNamespace(_fused=True, _ssm=True, _rate_rows=0, N=3, dt=0.02, batch=3)
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.08 exceeds the horizon N \* dt = 0\.06'):
        SSMClosedLoopBatch(plain, None, 0.02, 4)
    with pytest.raises(RuntimeError, match='n_keep >= 1 and dt_sim > 0'):
        SSMClosedLoopBatch(plain, None, 0.0, 2)
    # shapes of W, V and v0: checked before the library is called (a loop that was never created stands in)
    cl = SSMClosedLoopBatch.__new__(SSMClosedLoopBatch)
    cl.B, cl.n_x, cl.n_o, cl.n_u, cl.n_keep, cl.max_steps_per_run = 3, 6, 6, 4, 2, 32
    with pytest.raises(RuntimeError, match=r'W \(periods, n_keep, B, n_x\) must have shape \(4, 2, 3, 6\), got \(4, 3, 2, 6\)'):
        cl.run(4, W=np.zeros((4, 3, 2, 6)))
    with pytest.raises(RuntimeError, match=r'V \(periods, n_keep, B, n_o\) must have shape \(4, 2, 3, 6\), got \(8, 3, 6\)'):
        cl.run(4, V=np.zeros((8, 3, 6)))
    with pytest.raises(RuntimeError, match=r'v0 \(B, n_o\) must have shape \(3, 6\), got \(6,\)'):
        cl.reset(np.zeros((3, 6)), v0=np.zeros(6))
    lib = _lib.lib()
    assert lib.sgusto_ssm_loop_create(None, None, None, None, C.c_int(2), C.c_double(0.02), C.c_int(2), C.c_int(1), C.c_int64(32)) == -1
    assert b'sgusto_ssm_loop_create' in lib.srh_last_error()
    assert lib.sgusto_ssm_loop_run(None, C.c_int(1), None, None, None, None, None, None, None, None, None, None) == -1
    assert b'sgusto_ssm_loop_run' in lib.srh_last_error()
    assert lib.sgusto_ssm_loop_reset(None, None, None, C.c_double(0.0)) == -1 and b'sgusto_ssm_loop_reset' in lib.srh_last_error()
    assert lib.sgusto_ssm_plan_dims(None, None, None, None, None, None, None, None, None) == -1 and b'sgusto_ssm_plan_dims' in lib.srh_last_error()
    assert lib.sgusto_ssm_plan_costs_dev(None, None, None) == -1 and b'sgusto_ssm_plan_costs_dev' in lib.srh_last_error()
    assert lib.sssm_rollout_dev(None, None, None, C.c_int(3), C.c_int64(1), C.c_int(1), C.c_double(0.02), None, None, None) == -1
    assert b'sssm_rollout_dev' in lib.srh_last_error()
    assert lib.sgusto_ssm_loop_advance(None, C.c_int(1), None, C.c_double(0.02), C.c_int(3), C.c_int(2), C.c_int64(1), *([None] * 12)) == -1
    assert b'sgusto_ssm_loop_advance' in lib.srh_last_error()
