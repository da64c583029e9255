"""CPU: the surface of the SSM closed loop on a TPWL plant exists -- sgusto_ssm_loop_create_tpwl and sgusto_ssm_loop_advance_tpwl declared in
include/sofacontrol_hip.h with the shipped signatures and exported by the built library, SSMClosedLoopBatch.on_plant and
closed_loop_ssm.advance_tpwl with the stated signatures --, the refusals that come before any device call answer without a GPU, and the
unit states the estimate once and keeps to the shared rules (point search, step rule, plan point, measurement row)."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['sgusto_ssm_loop_create_tpwl', 'sgusto_ssm_loop_advance_tpwl']


def header():
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = header()
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^int\s+sgusto_ssm_loop_create_tpwl\s*\(sgusto_ssm_loop_t \*\*out, sgusto_ssm_plan_t \*plan, sssm_t \*planner_model, '
                     r'stpwl_t \*plant, const double \*C,\s*const double \*y_ref, int n_o, double dt_sim, int n_keep, int64_t max_steps_per_run\)',
                     src, flags=re.M)
    assert re.search(r'^int\s+sgusto_ssm_loop_advance_tpwl\s*\(stpwl_t \*plant, const double \*C, const double \*y_ref, int n_o, '
                     r'sssm_t \*observer_model, double dt_sim, int N,\s*int n_keep, int64_t batch, const int32_t \*j, const double \*theta, '
                     r'const double \*uopt, const double \*x,\s*const double \*W, const double \*V, double \*X, double \*Z, double \*U, double \*Y, '
                     r'double \*Xhat, int32_t \*idx\)', src, flags=re.M)
    # the handle type is the SSM loop's: the other entry points serve both plant kinds, and keep their signatures
    assert len(re.findall(r'^typedef struct sgusto_ssm_loop sgusto_ssm_loop_t;', src, flags=re.M)) == 1
    assert re.search(r'^int\s+sgusto_ssm_loop_reset\s*\(sgusto_ssm_loop_t \*h, const double \*x0, const double \*v0, double t_start\)', src, flags=re.M)
    lib = _lib.lib()
    assert lib.sgusto_ssm_loop_create_tpwl(None, None, None, None, None, None, C.c_int(6), C.c_double(0.02), C.c_int(2), C.c_int64(32)) == -1
    assert b'sgusto_ssm_loop_create_tpwl' in lib.srh_last_error()
    assert lib.sgusto_ssm_loop_advance_tpwl(None, None, None, C.c_int(6), None, C.c_double(0.02), C.c_int(3), C.c_int(2), C.c_int64(1),
                                            *([None] * 12)) == -1
    assert b'sgusto_ssm_loop_advance_tpwl' in lib.srh_last_error()


def test_the_estimate_is_stated_once_and_the_kernel_keeps_to_the_shared_rules():
    unit = open(os.path.join(ROOT, 'soft-robot-control_amd', 'csrc', 'gusto_ssm_loop.hip')).read()
    code = re.sub(r'//[^\n]*', '', unit)
    assert len(re.findall(r'void ssm_loop_estimate\(', code)) == 1                # one definition ...
    assert len(re.findall(r'\bssm_loop_estimate\(', code)) == 3                   # ... called from both advance kernels
    assert code.count('ssm::basis_l(') == 1 and code.count('wg::group_sum<8>(') == 1          # the estimate's sums are nowhere else in the unit
    for kernel in ('ssm_loop_advance_kernel', 'ssm_loop_advance_tpwl_kernel'):
        m = re.search(r'__global__[^\n]*void %s\(.*?\n}\n' % kernel, code, flags=re.S)
        assert m and m.group(0).count('ssm_loop_estimate(') == 1, kernel
    body = re.search(r'__global__[^\n]*void ssm_loop_advance_tpwl_kernel\(.*?\n}\n', code, flags=re.S).group(0)
    for text in ('tpwl::nearest_wave(', 'tpwl::panel_load(', 'tpwl::step_slices(', 'tpwl::step_sum(', 'tpwl::step_carve(', 'plan_at(', 'out_row(',
                 'measure_row('):
        assert text in body, text
    for text in ('ext_vector_type(2)', 'At[q * n + j]', 'th * (hi - lo)', 'AdT +', 'BdT +', 'sqrt('):
        assert text not in code, text
    assert code.count('ssm_loop_advance_tpwl_kernel<<<') == 1 and code.count('ssm_loop_advance_kernel<<<') == 1


def test_python_surface():
    from sofacontrol_amd.scp import closed_loop_ssm
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    sig = inspect.signature(SSMClosedLoopBatch.on_plant).parameters
    assert list(sig) == ['gusto', 'plant', 'dt_sim', 'n_keep', 't', 'z', 'u', 'phase', 'observe', 'max_steps_per_run', 'C', 'y_ref']
    assert sig['C'].default is None and sig['y_ref'].default is None and sig['observe'].default is True
    adv = inspect.signature(closed_loop_ssm.advance_tpwl).parameters
    assert list(adv) == ['plant', 'C', 'y_ref', 'observer_model', 'dt_sim', 'N', 'j', 'theta', 'uopt', 'x', 'W', 'V']
    assert adv['W'].default is None and adv['V'].default is None
    assert SSMClosedLoopBatch.n_plant is None


def fake_gusto(n_u=4, n_o=6, **kw):
    d = dict(_fused=True, _ssm=True, _rate_rows=0, N=3, dt=0.02, batch=3, n_x=6, n_u=n_u, n_z=n_o, plan=None,
             model=types.SimpleNamespace(dyn_sys=types.SimpleNamespace(output_dim=n_o, handle=None)))
    d.update(kw)
    return types.SimpleNamespace(**d)


def no_device(*a, **k):
    raise AssertionError('a device call was reached')


def fake_tpwl(n=60, m=4, method='nn'):
    return types.SimpleNamespace(tpwl_method=method, get_state_dim=lambda: n, get_input_dim=lambda: m, handle_for=no_device)


def fake_ssm():
    return types.SimpleNamespace(output_dim=6, discr_method='be', discrete=False)


def test_refusals_on_the_host():
    """Argument checks that come before any device call: the fakes raise when their handle is asked for."""
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    make = SSMClosedLoopBatch.on_plant
    Cm, yr = np.zeros((6, 60)), np.zeros(6)
    with pytest.raises(RuntimeError, match=r'observe=False is not offered on a TPWL plant: the plant state is not the planner\'s state'):
        make(fake_gusto(), fake_tpwl(), 0.01, 2, observe=False, C=Cm, y_ref=yr)
    with pytest.raises(RuntimeError, match=r"weighting-mode plants \(tpwl_method = 'weighting'\)"):
        make(fake_gusto(), fake_tpwl(method='weighting'), 0.01, 2, C=Cm, y_ref=yr)
    for kw in (dict(C=Cm), dict(y_ref=yr), dict(C=Cm, y_ref=yr)):
        with pytest.raises(RuntimeError, match='C and y_ref belong to a TPWL plant'):
            make(fake_gusto(), fake_ssm(), 0.01, 2, **kw)
    for kw in (dict(), dict(C=Cm), dict(y_ref=yr)):
        with pytest.raises(RuntimeError, match=r'a TPWL plant needs its measurement C \(n_o, n_plant\) and y_ref \(n_o,\)'):
            make(fake_gusto(), fake_tpwl(), 0.01, 2, **kw)
    with pytest.raises(RuntimeError, match=r'a TPWL plant needs its measurement'):
        SSMClosedLoopBatch(fake_gusto(), fake_tpwl(), 0.01, 2)
    with pytest.raises(RuntimeError, match=r'C must have shape \(n_o, n_plant\) = \(6, 60\), got \(60, 6\)'):
        make(fake_gusto(), fake_tpwl(), 0.01, 2, C=Cm.T, y_ref=yr)
    with pytest.raises(RuntimeError, match=r'C must have shape \(n_o, n_plant\) = \(6, 60\), got \(4, 60\)'):
        make(fake_gusto(), fake_tpwl(), 0.01, 2, C=Cm[:4], y_ref=yr)
    with pytest.raises(RuntimeError, match=r'y_ref must have shape \(n_o,\) = \(6,\), got \(1, 6\)'):
        make(fake_gusto(), fake_tpwl(), 0.01, 2, C=Cm, y_ref=yr[None])
    with pytest.raises(RuntimeError, match=r"the plant's n_x = 130 exceeds the limit n_x <= 128"):
        make(fake_gusto(), fake_tpwl(n=130), 0.01, 2, C=np.zeros((6, 130)), y_ref=yr)
    with pytest.raises(RuntimeError, match=r'the plant has n_u = 3, the plan n_u = 4'):
        make(fake_gusto(), fake_tpwl(m=3), 0.01, 2, C=Cm, y_ref=yr)
    with pytest.raises(RuntimeError, match=r'4 input-rate rows \(dU\).*status -78'):
        make(fake_gusto(_rate_rows=4), fake_tpwl(), 0.01, 2, C=Cm, y_ref=yr)
    with pytest.raises(RuntimeError, match='SSM plan is resident'):
        make(fake_gusto(_ssm=False), fake_tpwl(), 0.01, 2, C=Cm, y_ref=yr)
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.08 exceeds the horizon N \* dt = 0\.06'):
        make(fake_gusto(), fake_tpwl(), 0.02, 4, C=Cm, y_ref=yr)
    # shapes of x0, W, V and v0 on a TPWL plant: checked before the library is called (a loop that was never created stands in)
    cl = SSMClosedLoopBatch.__new__(SSMClosedLoopBatch)
    cl.B, cl.n_x, cl.n_o, cl.n_u, cl.n_keep, cl.max_steps_per_run, cl.n_plant = 3, 6, 6, 4, 2, 32, 60
    with pytest.raises(RuntimeError, match=r'x0 \(B, n_plant\) must have shape \(3, 60\), got \(3, 6\)'):
        cl.reset(np.zeros((3, 6)))
    with pytest.raises(RuntimeError, match=r'W \(periods, n_keep, B, n_plant\) must have shape \(4, 2, 3, 60\), got \(4, 2, 3, 6\)'):
        cl.run(4, W=np.zeros((4, 2, 3, 6)))
    with pytest.raises(RuntimeError, match=r'V \(periods, n_keep, B, n_o\) must have shape \(4, 2, 3, 6\), got \(4, 2, 3, 60\)'):
        cl.run(4, V=np.zeros((4, 2, 3, 60)))
