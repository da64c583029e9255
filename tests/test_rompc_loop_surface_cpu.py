"""CPU: the surface of the batched closed-loop ROMPC exists -- every srompc_loop_* entry point declared in include/sofacontrol_hip.h with
the stated signature and exported by the built library, baselines.rompc.closed_loop.ROMPCClosedLoopBatch / ROMPCLoopResult with the stated
methods -- and every refusal that is decided before a device call raises without a GPU."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['srompc_loop_create', 'srompc_loop_destroy', 'srompc_loop_set_target', 'srompc_loop_reset', 'srompc_loop_run', 'srompc_loop_last_inputs',
           'srompc_loop_last_plan', 'srompc_loop_stats', 'srompc_loop_chain', 'srompc_loop_advance']
D, I = r'const double \*', r'const int32_t \*'
SIGNATURES = {
    'srompc_loop_create': r'srompc_loop_t \*\*out, srompc_t \*ctrl, const slocp_problem \*prob, ' + D + 'A_mpc, ' + D + 'B_mpc, ' + D + 'd_mpc, '
                          r'double dt_mpc, stpwl_t \*plant, double dt_sim, int n_replan, int64_t max_steps_per_run',
    'srompc_loop_destroy': r'srompc_loop_t \*h',
    'srompc_loop_set_target': r'srompc_loop_t \*h, int T, ' + D + 't, ' + D + 'z, ' + D + 'u_des, ' + D + 'phase',
    'srompc_loop_reset': r'srompc_loop_t \*h, ' + D + 'x0, ' + D + 'x_hat0, double t_start',
    'srompc_loop_run': r'srompc_loop_t \*h, int periods, ' + D + 'W, ' + D + 'V, ' + D + r'X_plant, double \*X, double \*XH, double \*Y, double \*Z, '
                       r'double \*U, double \*Ubar, double \*Xbar, double \*J, int32_t \*status, int32_t \*iters',
    'srompc_loop_last_inputs': r'srompc_loop_t \*h, double \*x0, double \*z, double \*zf, double \*u_des',
    'srompc_loop_last_plan': r'srompc_loop_t \*h, double \*xopt, double \*uopt',
    'srompc_loop_stats': r'srompc_loop_t \*h, int64_t \*steps, int64_t \*waits_last_run',
    'srompc_loop_chain': r'srompc_loop_t \*h, ' + D + 'xopt_prev, ' + D + 'uopt_prev, ' + D + 'xopt, ' + D + 'uopt, ' + D + 'x0, ' + I +
                         r'status, int first, double \*xopt_out, double \*uopt_out, double \*x0_next',
    'srompc_loop_advance': r'srompc_loop_t \*h, ' + D + 'xopt, ' + D + 'uopt, ' + D + 'x, ' + D + 'x_hat, ' + D + 'W, ' + D + 'V, ' + D +
                           r'X_plant, double \*X, double \*XH, double \*Y, double \*Z, double \*U, double \*Ubar, double \*Xbar',
}


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    flat = re.sub(r'\s+', ' ', src).replace(' ,', ',')
    assert re.search(r'^typedef struct srompc_loop srompc_loop_t;', src, flags=re.M)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
        assert re.search(r'int %s\(%s ?\);' % (name, SIGNATURES[name]), flat), name
    # the controller's own entry points keep their signatures
    assert re.search(r'int srompc_step\(srompc_t \*h, srom_t \*rom, const double \*x_full, const double \*u_given, const double \*ubar, '
                     r'const double \*xbar, const double \*y, double \*u_out, double \*x_out, double \*z_out\);', flat)


def test_python_surface():
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch, ROMPCLoopResult
    init = list(inspect.signature(ROMPCClosedLoopBatch.__init__).parameters)
    assert init[:18] == ['self', 'observer', 'mpc_model', 'N', 'dt_mpc', 'cost_params', 'plant', 'dt_sim', 'n_replan', 't', 'z', 'u', 'phase', 'U',
                         'X', 'Xf', 'x_char', 'max_steps_per_run']
    assert list(inspect.signature(ROMPCClosedLoopBatch.reset).parameters) == ['self', 'x0', 'x_hat0', 't_start']
    run = inspect.signature(ROMPCClosedLoopBatch.run).parameters
    assert list(run) == ['self', 'periods', 'W', 'V', 'X_plant', 'record_x'] and run['record_x'].default is True
    for name in ('step', 'last_inputs', 'last_plan', 'stats', '_chain', '_advance'):
        assert callable(getattr(ROMPCClosedLoopBatch, name)), name
    assert list(inspect.signature(ROMPCLoopResult.__init__).parameters) == ['self', 'x', 'x_hat', 'y', 'z', 'u', 'u_bar', 'x_bar', 'iters', 'status',
                                                                            'J', 't']
    r = ROMPCLoopResult(*range(11))
    assert (r.x, r.x_hat, r.y, r.z, r.u, r.u_bar, r.x_bar, r.iters, r.status, r.J, r.t) == tuple(range(11))


def test_refusals_on_the_host():
    """Argument checks that come before any device call."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.baselines.rompc.closed_loop import ROMPCClosedLoopBatch
    from sofacontrol_amd.utils import QuadraticCost
    lib = _lib.lib()
    assert lib.srompc_loop_create(*[None] * 6, C.c_double(0.05), None, C.c_double(0.01), C.c_int(10), C.c_int64(160)) == -1
    assert b'srompc_loop_create: null' in lib.srh_last_error()
    assert lib.srompc_loop_reset(None, None, None, C.c_double(0.0)) == -1 and b'srompc_loop_reset' in lib.srh_last_error()
    assert lib.srompc_loop_run(None, C.c_int(1), *[None] * 13) == -1 and b'srompc_loop_run' in lib.srh_last_error()
    assert lib.srompc_loop_set_target(None, C.c_int(2), None, None, None, None) == -1 and b'srompc_loop_set_target' in lib.srh_last_error()
    assert lib.srompc_loop_last_inputs(None, None, None, None, None) == -1 and b'srompc_loop_last_inputs' in lib.srh_last_error()
    assert lib.srompc_loop_last_plan(None, None, None) == -1 and b'srompc_loop_last_plan' in lib.srh_last_error()
    assert lib.srompc_loop_stats(None, None, None) == -1 and b'srompc_loop_stats' in lib.srh_last_error()
    assert lib.srompc_loop_chain(*[None] * 7, C.c_int(0), None, None, None) == -1 and b'srompc_loop_chain' in lib.srh_last_error()
    assert lib.srompc_loop_advance(*[None] * 15) == -1 and b'srompc_loop_advance' in lib.srh_last_error()
    obs = types.SimpleNamespace(batch=3, n_x=8, n_u=3, n_y=30, n_z=6, _h=None)
    model = types.SimpleNamespace(H=np.ones((6, 8)), A_d=np.eye(8), B_d=np.ones((8, 3)), d_d=np.zeros(8))
    cost = QuadraticCost(Q=np.eye(6), R=np.eye(3))
    nn = lambda n=8, m=3, method='nn': types.SimpleNamespace(tpwl_method=method, get_state_dim=lambda: n, get_input_dim=lambda: m)
    with pytest.raises(RuntimeError, match=r'dU\) are not offered'):
        ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(), 0.01, 10, dU=object())
    with pytest.raises(RuntimeError, match='input_nullspace is not offered'):
        ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(), 0.01, 10, input_nullspace=np.ones(3))
    with pytest.raises(RuntimeError, match=r"weighting-mode plants \(tpwl_method = 'weighting'\) are not stepped on the device"):
        ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(method='weighting'), 0.01, 10)
    with pytest.raises(RuntimeError, match=r'n_replan \* dt_sim = 0.3 exceeds the horizon N \* dt_mpc = 0.25'):
        ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(), 0.01, 30)
    with pytest.raises(RuntimeError, match='need n_replan >= 1 and dt_sim > 0'):
        ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(), 0.01, 0)
    wide = types.SimpleNamespace(batch=3, n_x=8, n_u=17, n_y=30, n_z=6, _h=None)
    with pytest.raises(RuntimeError, match='n_u = 17 exceeds the limit n_x <= 128, n_u <= 16'):
        ROMPCClosedLoopBatch(wide, model, 5, 0.05, cost, None, 0.01, 10)
    for n, m in ((60, 3), (8, 4)):
        with pytest.raises(RuntimeError, match='the plant has n_x = %d, n_u = %d, the controller n_x = 8, n_u = 3' % (n, m)):
            ROMPCClosedLoopBatch(obs, model, 5, 0.05, cost, nn(n, m), 0.01, 10)
    # a run without a plant and without X_plant, and a run before a reset, on an object that never reached the device
    loop = ROMPCClosedLoopBatch.__new__(ROMPCClosedLoopBatch)
    loop.plant, loop._k, loop._h = None, None, C.c_void_p()
    with pytest.raises(RuntimeError, match='X_plant is required'):
        loop.run(1)
    loop.plant = nn()
    with pytest.raises(RuntimeError, match='call reset first'):
        loop.run(1)
