"""CPU: the surface of the batched closed-loop Koopman MPC exists -- every skoop_loop_* entry point declared in include/sofacontrol_hip.h
with the stated signature and exported by the built library, baselines.koopman.closed_loop.KoopmanClosedLoopBatch / KoopmanLoopResult with
the stated signatures -- every refusal that is decided before a device call raises without a GPU, the shape errors are raised on an
object that never reached the device, and the new unit keeps to the shared shell (text pins beside those of
tests/test_gusto_loop_surface_cpu.py)."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['skoop_loop_create', 'skoop_loop_destroy', 'skoop_loop_set_target', 'skoop_loop_reset', 'skoop_loop_run', 'skoop_loop_last_inputs',
           'skoop_loop_last_plan', 'skoop_loop_stats', 'skoop_loop_fixup', 'skoop_loop_advance']
D, I = r'const double \*', r'const int32_t \*'
SIGNATURES = {
    'skoop_loop_create': r'skoop_loop_t \*\*out, skoop_t \*h, const slocp_problem \*prob, ' + D + 'A, ' + D + r'B, double Ts, stpwl_t \*plant, ' + D +
                         'C, ' + D + 'y_ref, ' + D + r'u0, double dt_sim, int rollout_horizon, int64_t max_steps_per_run',
    'skoop_loop_destroy': r'skoop_loop_t \*h',
    'skoop_loop_set_target': r'skoop_loop_t \*h, int T, ' + D + 't, ' + D + 'z, ' + D + 'u_des, ' + D + 'phase',
    'skoop_loop_reset': r'skoop_loop_t \*h, ' + D + 'x0, ' + D + 'y0, ' + D + 'y_hist, ' + D + 'u_hist, ' + D + 'u_prev0, ' + D + 'v0, double t_start',
    'skoop_loop_run': r'skoop_loop_t \*h, int periods, ' + D + 'W, ' + D + 'V, ' + D + 'Y_plant, ' + D + r'U_applied, double \*X, double \*Y, '
                      r'double \*U, double \*Xlift, double \*J, int32_t \*status, int32_t \*iters',
    'skoop_loop_last_inputs': r'skoop_loop_t \*h, double \*x0, double \*z, double \*zf, double \*u_des',
    'skoop_loop_last_plan': r'skoop_loop_t \*h, double \*xopt, double \*uopt',
    'skoop_loop_stats': r'skoop_loop_t \*h, int64_t \*steps, int64_t \*waits_last_run',
    'skoop_loop_fixup': r'skoop_loop_t \*h, ' + D + 'xopt_prev, ' + D + 'uopt_prev, ' + D + 'xopt, ' + D + 'uopt, ' + D + 'x0, ' + I +
                        r'status, int first, double \*xopt_out, double \*uopt_out',
    'skoop_loop_advance': r'skoop_loop_t \*h, ' + D + 'uopt, ' + D + 'x, ' + D + 'W, ' + D + 'V, ' + D + 'Y_plant, ' + D +
                          r'U_applied, double \*X, double \*Y, double \*U, int32_t \*idx',
}


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    flat = re.sub(r'\s+', ' ', src).replace(' ,', ',')
    assert re.search(r'^typedef struct skoop_loop skoop_loop_t;', src, flags=re.M)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
        assert re.search(r'int %s\(%s ?\);' % (name, SIGNATURES[name]), flat), name
    # the lift's own entry points keep their signatures
    assert re.search(r'int skoop_ring_lift_dev\(skoop_t \*h, double \*out_dev\);', flat)
    assert re.search(r'int skoop_push\(skoop_t \*h, const double \*y, const double \*u\);', flat)


def test_python_surface():
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch, KoopmanLoopResult
    from sofacontrol_amd.scp import closed_loop
    from sofacontrol_amd.baselines.koopman import closed_loop as kcl
    sig = inspect.signature(KoopmanClosedLoopBatch.__init__).parameters
    assert list(sig) == ['self', 'model', 'N', 'cost_params', 'plant', 'C', 'y_ref', 'dt_sim', 'rollout_horizon', 't', 'z', 'u', 'phase', 'U', 'X',
                         'Xf', 'x_char', 'u0', 'batch', 'max_steps_per_run', 'dU', 'input_nullspace']
    assert all(sig[p].default is None for p in ('t', 'z', 'u', 'phase', 'U', 'X', 'Xf', 'x_char', 'u0', 'max_steps_per_run', 'dU', 'input_nullspace'))
    assert sig['batch'].default == 1 and 'input_hold' not in sig
    rs = inspect.signature(KoopmanClosedLoopBatch.reset).parameters
    assert list(rs) == ['self', 'x0', 'y0', 'y_hist', 'u_hist', 'u_prev0', 'v0', 't_start']
    assert all(rs[p].default is None for p in list(rs)[1:-1]) and rs['t_start'].default == 0.0
    run = inspect.signature(KoopmanClosedLoopBatch.run).parameters
    assert list(run) == ['self', 'periods', 'W', 'V', 'Y_plant', 'U_applied', 'record_x'] and run['record_x'].default is True
    assert all(run[p].default is None for p in ('W', 'V', 'Y_plant', 'U_applied'))
    for name in ('step', 'last_inputs', 'last_plan', 'stats', '_fixup', '_advance'):
        assert callable(getattr(KoopmanClosedLoopBatch, name)), name
    assert issubclass(KoopmanClosedLoopBatch, closed_loop._LoopBatch) and KoopmanClosedLoopBatch._sym == 'skoop_loop'
    assert list(inspect.signature(KoopmanLoopResult.__init__).parameters) == ['self', 'x', 'y', 'u', 'x_lift', 'iters', 'status', 'J', 't']
    r = KoopmanLoopResult(*range(8))
    assert (r.x, r.y, r.u, r.x_lift, r.iters, r.status, r.J, r.t) == tuple(range(8))
    # the schedule is the TPWL loop's: the same function object, no second statement
    assert kcl.schedule is closed_loop.schedule and 'def schedule' not in inspect.getsource(kcl)
    doc = kcl.__doc__
    for word in ('t_delay', 'Y= re-projection', 'input clipping', 'dU', 'input_nullspace', 'nonlinear_observer', 'weighting-mode', 'its own plant',
                 'input_hold'):
        assert word in doc, word


def test_the_unit_keeps_to_the_shared_shell():
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    unit = units['koopman_loop.hip']
    assert 'THE POLICY' in unit.split('#include')[0]
    assert 'struct skoop_loop : MpcLoopCore' in unit and 'struct MpcLoopCore : LoopCore' in units['mpc_loop_host.h']
    assert 'loop_run_periods(h, "skoop_loop_run"' in unit
    # the unit's one kernel is its advance kernel: the tile and the plan-shift kernels are the linear-MPC shell's, stated once for both units
    assert 'koop_loop_advance_kernel' in unit and unit.count('__launch_bounds__(256)') == 1 and unit.count('__global__') == 1
    for kernel in ('loop_plan_shift_kernel(', 'loop_tile_kernel('):
        assert [f for f, u in units.items() if '__global__ __launch_bounds__(256) void ' + kernel in u] == ['mpc_loop_host.h'], kernel
    assert sorted(f for f, u in units.items() if '#include "mpc_loop_host.h"' in u) == ['koopman_loop.hip', 'rompc_loop.hip']
    assert 'h->solve(p, a)' in unit and 'slocp_plan_solve_dev_resident(' not in unit and 'slocp_plan_create(' not in unit
    for text in ('loop_prepare_kernel<<<', 'hipMemcpyDeviceToHost', 'hipStreamCreate', 'AdT +', 'BdT +', 'ext_vector_type', 'th * (hi - lo)',
                 'int sgusto_loop_schedule', 'At[q * n + j]'):
        assert text not in unit, text
    for text in ('tpwl::nearest_wave', 'tpwl::panel_load', 'tpwl::step_slices', 'tpwl::step_sum', 'measure_row(', 'kl_advance_lds_bytes'):
        assert text in unit, text
    # the handle and the lift's launcher live in one header, included by both units
    assert [f for f, u in units.items() if 'struct skoop {' in u] == ['koopman_host.h']
    assert [f for f, u in units.items() if 'int koop_launch_lift(' in u] == ['koopman_host.h']
    assert [f for f, u in units.items() if 'struct KoopLiftArgs {' in u] == ['koopman_host.h']
    for f in ('koopman.hip', 'koopman_loop.hip'):
        assert '#include "koopman_host.h"' in units[f], f
    mk = open(os.path.join(csrc, 'Makefile')).read()
    for dep in (r'koopman_loop\.o[^\n]*: \$\(TPWL_H\)', r'koopman_loop\.o[^\n]*: gusto_loop_prep\.h gusto_loop_host\.h', r'koopman\.o koopman_loop\.o: koopman_host\.h',
                r'rompc_loop\.o koopman_loop\.o: mpc_loop_host\.h'):
        assert re.search(dep, mk), dep


def koopman_model(n_lift=66, n=3, m=4, delays=1, Ts=0.05):
    return types.SimpleNamespace(Ts=Ts, n=n, m=m, delays=delays, W=np.eye(n_lift), A_d=np.eye(n_lift), B_d=np.ones((n_lift, m)), H=np.ones((n, n_lift)))


def test_refusals_on_the_host():
    """Argument checks that come before any device call."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch as KL
    from sofacontrol_amd.utils import QuadraticCost
    lib = _lib.lib()
    assert lib.skoop_loop_create(*[None] * 5, C.c_double(0.05), *[None] * 4, C.c_double(0.01), C.c_int(1), C.c_int64(80)) == -1
    assert b'skoop_loop_create: null' in lib.srh_last_error()
    assert lib.skoop_loop_destroy(None) == -1 and b'skoop_loop_destroy' in lib.srh_last_error()
    assert lib.skoop_loop_set_target(None, C.c_int(2), None, None, None, None) == -1 and b'skoop_loop_set_target' in lib.srh_last_error()
    assert lib.skoop_loop_reset(*[None] * 7, C.c_double(0.0)) == -1 and b'skoop_loop_reset' in lib.srh_last_error()
    assert lib.skoop_loop_run(None, C.c_int(1), *[None] * 11) == -1 and b'skoop_loop_run' in lib.srh_last_error()
    assert lib.skoop_loop_last_inputs(None, None, None, None, None) == -1 and b'skoop_loop_last_inputs' in lib.srh_last_error()
    assert lib.skoop_loop_last_plan(None, None, None) == -1 and b'skoop_loop_last_plan' in lib.srh_last_error()
    assert lib.skoop_loop_stats(None, None, None) == -1 and b'skoop_loop_stats' in lib.srh_last_error()
    assert lib.skoop_loop_fixup(*[None] * 7, C.c_int(0), None, None) == -1 and b'skoop_loop_fixup' in lib.srh_last_error()
    assert lib.skoop_loop_advance(*[None] * 11) == -1 and b'skoop_loop_advance' in lib.srh_last_error()
    cost = QuadraticCost(Q=np.eye(3), R=np.eye(4))
    nn = lambda n=72, m=4, method='nn': types.SimpleNamespace(tpwl_method=method, get_state_dim=lambda: n, get_input_dim=lambda: m)
    Cm, yr = np.ones((3, 72)), np.zeros(3)
    km = koopman_model()
    with pytest.raises(RuntimeError, match=r'dU\) are not offered'):
        KL(km, 5, cost, nn(), Cm, yr, 0.01, 1, dU=object())
    with pytest.raises(RuntimeError, match='input_nullspace is not offered'):
        KL(km, 5, cost, nn(), Cm, yr, 0.01, 1, input_nullspace=np.ones(4))
    with pytest.raises(RuntimeError, match=r"weighting-mode plants \(tpwl_method = 'weighting'\) are not stepped on the device"):
        KL(km, 5, cost, nn(method='weighting'), Cm, yr, 0.01, 1)
    for dt_sim in (0.03, 0.0100001, 0.1):                         # Ts / dt_sim = 1.67, 4.99995, 0.5
        with pytest.raises(RuntimeError, match=r'Ts / dt_sim = [0-9.]+ is not an integer >= 1'):
            KL(km, 5, cost, nn(), Cm, yr, dt_sim, 1)
    with pytest.raises(RuntimeError, match='need Ts > 0 and dt_sim > 0'):
        KL(km, 5, cost, nn(), Cm, yr, 0.0, 1)
    for rh in (0, 6):
        with pytest.raises(RuntimeError, match=r'rollout_horizon = %d is outside 1 \.\. N = 5' % rh):
            KL(km, 5, cost, nn(), Cm, yr, 0.01, rh)
    with pytest.raises(RuntimeError, match='n_lift = 97 exceeds the limit n_lift <= 96'):
        KL(koopman_model(n_lift=97), 5, cost, nn(), Cm, yr, 0.01, 1)
    with pytest.raises(RuntimeError, match='n_u = 17 exceeds the limit n_u <= 16'):
        KL(koopman_model(m=17), 5, cost, nn(m=17), Cm, yr, 0.01, 1)
    with pytest.raises(RuntimeError, match=r"the plant's n_x = 130 exceeds the limit n_x <= 128"):
        KL(km, 5, cost, nn(n=130), np.ones((3, 130)), yr, 0.01, 1)
    with pytest.raises(RuntimeError, match='the plant has n_u = 3, the model n_u = 4'):
        KL(km, 5, cost, nn(m=3), Cm, yr, 0.01, 1)
    for bad_C, bad_y in ((np.ones((72, 3)), yr), (np.ones((2, 72)), yr), (Cm, np.zeros(4)), (None, yr), (Cm, None)):
        with pytest.raises(RuntimeError, match=r'C must have shape \(n_y, n_plant\) = \(3, 72\) and y_ref n_y = 3 entries'):
            KL(km, 5, cost, nn(), bad_C, bad_y, 0.01, 1)


def test_shape_errors_on_an_object_that_never_reached_the_device():
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch as KL
    cl = KL.__new__(KL)
    cl._h, cl._k, cl.plant = C.c_void_p(), None, None
    cl.B, cl.N, cl.n_x, cl.n_plant, cl.n_y, cl.n_u, cl.delays, cl.n_keep, cl.max_steps_per_run = 3, 5, 66, 72, 3, 4, 1, 5, 80
    with pytest.raises(RuntimeError, match='Y_plant is required'):
        cl.run(1)
    with pytest.raises(RuntimeError, match='y0 is required'):
        cl.reset(y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((3, 1, 4)))
    cl.plant = object()
    with pytest.raises(RuntimeError, match='call reset first'):
        cl.run(1)
    with pytest.raises(RuntimeError, match='x0 is required'):
        cl.reset()
    with pytest.raises(RuntimeError, match='the model has 1 delays: y_hist and u_hist are required'):
        cl.reset(np.zeros((3, 72)))
    with pytest.raises(RuntimeError, match=r'x0 \(B, n_plant\) must have shape \(3, 72\), got \(72,\)'):
        cl.reset(np.zeros(72), y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((3, 1, 4)))
    with pytest.raises(RuntimeError, match=r'y_hist \(B, delays, n_y\) must have shape \(3, 1, 3\), got \(3, 3\)'):
        cl.reset(np.zeros((3, 72)), y_hist=np.zeros((3, 3)), u_hist=np.zeros((3, 1, 4)))
    with pytest.raises(RuntimeError, match=r'u_hist \(B, delays, n_u\) must have shape \(3, 1, 4\), got \(1, 3, 4\)'):
        cl.reset(np.zeros((3, 72)), y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((1, 3, 4)))
    with pytest.raises(RuntimeError, match=r'u_prev0 \(B, n_u\) must have shape \(3, 4\), got \(4,\)'):
        cl.reset(np.zeros((3, 72)), y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((3, 1, 4)), u_prev0=np.zeros(4))
    with pytest.raises(RuntimeError, match=r'v0 \(B, n_y\) must have shape \(3, 3\), got \(3,\)'):
        cl.reset(np.zeros((3, 72)), y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((3, 1, 4)), v0=np.zeros(3))
    cl._k = 0
    with pytest.raises(RuntimeError, match=r'W \(periods, n_keep, B, n_plant\) must have shape \(4, 5, 3, 72\), got \(4, 3, 5, 72\)'):
        cl.run(4, W=np.zeros((4, 3, 5, 72)))
    with pytest.raises(RuntimeError, match=r'V \(periods, n_keep, B, n_y\) must have shape \(4, 5, 3, 3\), got \(20, 3, 3\)'):
        cl.run(4, V=np.zeros((20, 3, 3)))
    with pytest.raises(RuntimeError, match=r'Y_plant \(B, S \+ 1, n_y\) must have shape \(3, 21, 3\), got \(3, 20, 3\)'):
        cl.run(4, Y_plant=np.zeros((3, 20, 3)))
    with pytest.raises(RuntimeError, match=r'U_applied \(B, S, n_u\) must have shape \(3, 20, 4\), got \(20, 3, 4\)'):
        cl.run(4, U_applied=np.zeros((20, 3, 4)))
    cl.plant, cl.n_plant = None, 0
    with pytest.raises(RuntimeError, match=r'y0 \(B, n_y\) must have shape \(3, 3\), got \(3,\)'):
        cl.reset(y0=np.zeros(3), y_hist=np.zeros((3, 1, 3)), u_hist=np.zeros((3, 1, 4)))
    cl._h = C.c_void_p()                                          # (nothing to destroy)
