"""CPU: the batched-filter and observed-loop surface exists -- every sekf_batch_* entry point declared in include/sofacontrol_hip.h and exported by the
built library, tpwl.observer.DiscreteEKFObserverBatch with the stated methods -- every refusal that is decided before a device call
raises without a GPU, and the members of tests/ekf_batch_cases.py that tests/test_ekf_batch_gpu.py holds to the long-double
reference meet the input conditions of tests/ekf_cases.py: nearest-point margin above MARGIN at every predictor, e_oracle <=
E_ORACLE_MAX, the kernel path the shape is labelled with.  The observed loop's entry points (sgusto_loop_set_observer, _reset_observed,
_run_observed, _advance_observed) and ClosedLoopBatch(observer=...) are checked the same way."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import ekf_batch_cases as bc
import ekf_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['sekf_batch_create', 'sekf_batch_destroy', 'sekf_batch_plan', 'sekf_batch_set_state', 'sekf_batch_get_state', 'sekf_batch_last_points',
           'sekf_batch_step']


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^typedef struct sekf_batch sekf_batch_t;', src, flags=re.M)
    assert re.search(r'^int\s+sekf_batch_create\s*\(sekf_batch_t \*\*out, stpwl_t \*model, const double \*C, const double \*y_ref, int n_y,\s*'
                     r'const double \*Sigma0, const double \*W, const double \*V, int64_t batch\)', src, flags=re.M)
    assert re.search(r'^int\s+sekf_batch_step\s*\(sekf_batch_t \*h, const double \*u, const double \*y, double \*x_out\)', src, flags=re.M)
    assert re.search(r'^int\s+sekf_batch_get_state\s*\(sekf_batch_t \*h, double \*x, double \*Sigma, int \*status\)', src, flags=re.M)
    # the one-filter entry points keep their signatures
    assert re.search(r'^int\s+sekf_step\s*\(sekf_t \*h, const double \*u, const double \*y, const double \*A_d, const double \*B_d,\s*'
                     r'const double \*d_d, double \*x_out\)', src, flags=re.M)


LOOP_SYMBOLS = ['sgusto_loop_set_observer', 'sgusto_loop_reset_observed', 'sgusto_loop_run_observed', 'sgusto_loop_advance_observed']


def test_observed_loop_symbols_and_python_surface():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch, ClosedLoopResult
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in LOOP_SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^int\s+sgusto_loop_set_observer\s*\(sgusto_loop_t \*h, sekf_batch_t \*observer\)', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_loop_reset_observed\s*\(sgusto_loop_t \*h, const double \*x0, const double \*x_hat0, double t_start\)', src, flags=re.M)
    init = inspect.signature(ClosedLoopBatch.__init__).parameters
    assert 'observer' in init and init['observer'].default is None
    assert list(inspect.signature(ClosedLoopBatch.reset_observed).parameters) == ['self', 'x0', 'x_hat0', 't_start']
    run = inspect.signature(ClosedLoopBatch.run_observed).parameters
    assert list(run) == ['self', 'periods', 'W', 'V', 'record_x'] and run['V'].default is None
    assert callable(ClosedLoopBatch._advance_observed)
    res = ClosedLoopResult(*range(7))
    assert res.x_hat is None and res.y is None and res.ekf_status is None
    res = ClosedLoopResult(*range(7), x_hat=7, y=8, ekf_status=9)
    assert (res.x_hat, res.y, res.ekf_status) == (7, 8, 9)
    lib = _lib.lib()
    assert lib.sgusto_loop_set_observer(None, None) == -1 and b'sgusto_loop_set_observer' in lib.srh_last_error()
    assert lib.sgusto_loop_reset_observed(None, None, None, C.c_double(0.0)) == -1 and b'sgusto_loop_reset_observed' in lib.srh_last_error()
    assert lib.sgusto_loop_run_observed(None, C.c_int(1), *[None] * 11) == -1 and b'sgusto_loop_run_observed' in lib.srh_last_error()
    assert lib.sgusto_loop_advance_observed(*[None] * 16) == -1 and b'sgusto_loop_advance_observed' in lib.srh_last_error()
    # an observer of another batch, n_x or n_u is refused before any device call
    fused = types.SimpleNamespace(_fused=True, _ssm=False, N=12, dt=0.05, batch=3, n_x=8, n_u=3)
    for shape, text in (((2, 8, 3), 'batch = 2, n_x = 8, n_u = 3'), ((3, 60, 3), 'batch = 3, n_x = 60, n_u = 3'), ((3, 8, 4), 'batch = 3, n_x = 8, n_u = 4')):
        obs = types.SimpleNamespace(batch=shape[0], state_dim=shape[1], input_dim=shape[2])
        with pytest.raises(RuntimeError, match='the observer has %s; the loop needs batch = 3, n_x = 8, n_u = 3' % text):
            ClosedLoopBatch(fused, None, 0.01, 10, observer=obs)


def test_python_surface():
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    assert list(inspect.signature(DiscreteEKFObserverBatch.__init__).parameters)[:3] == ['self', 'dyn_sys', 'batch']
    assert list(inspect.signature(DiscreteEKFObserverBatch.initialize).parameters) == ['self', 'x']
    assert list(inspect.signature(DiscreteEKFObserverBatch.update).parameters) == ['self', 'u', 'y', 'dt']
    assert list(inspect.signature(DiscreteEKFObserverBatch.predict_state).parameters) == ['self', 'u', 'dt']
    assert list(inspect.signature(DiscreteEKFObserverBatch.update_state).parameters) == ['self', 'y']
    assert callable(DiscreteEKFObserverBatch.kernel_plan)
    for prop in ('x', 'Sigma', 'status', 'points'):
        assert isinstance(getattr(DiscreteEKFObserverBatch, prop), property), prop


def dyn_sys(n=8, ny=6, m=4, method='nn'):
    return types.SimpleNamespace(C=np.ones((ny, n)), y_ref=np.zeros(ny), tpwl_method=method, get_state_dim=lambda: n,
                                 get_input_dim=lambda: m)


def test_refusals_on_the_host():
    """Argument checks that come before any device call."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    none = dyn_sys(); none.C = None
    with pytest.raises(RuntimeError, match='Need to set meas. model'):
        DiscreteEKFObserverBatch(none, 2)
    with pytest.raises(RuntimeError, match=r"weighting-mode models \(tpwl_method = 'weighting'\) are not batched"):
        DiscreteEKFObserverBatch(dyn_sys(method='weighting'), 2)
    for bad in (0, -3, 1.5):
        with pytest.raises(RuntimeError, match='batch must be an integer >= 1'):
            DiscreteEKFObserverBatch(dyn_sys(), bad)
    with pytest.raises(RuntimeError, match=r'Sigma0 must have shape \(8, 8\), got \(7, 7\)'):
        DiscreteEKFObserverBatch(dyn_sys(), 2, Sigma0=np.eye(7))
    with pytest.raises(RuntimeError, match=r'W must have shape \(8, 8\)'):
        DiscreteEKFObserverBatch(dyn_sys(), 2, W=np.eye(6))
    with pytest.raises(RuntimeError, match=r'V must have shape \(6, 6\)'):
        DiscreteEKFObserverBatch(dyn_sys(), 2, V=np.eye(8))
    with pytest.raises(RuntimeError, match='no filter kernel takes n_x = 200, n_y = 30'):
        DiscreteEKFObserverBatch(dyn_sys(200, 30), 2)
    with pytest.raises(RuntimeError, match='no filter kernel takes n_x = 6, n_y = 8'):
        DiscreteEKFObserverBatch(dyn_sys(6, 8), 2)
    lib = _lib.lib()
    assert lib.sekf_batch_create(None, None, None, None, C.c_int(6), None, None, None, C.c_int64(2)) == -1 and b'sekf_batch_create: null' in lib.srh_last_error()
    assert lib.sekf_batch_step(None, None, None, None) == -1 and b'sekf_batch_step: null' in lib.srh_last_error()
    assert lib.sekf_batch_set_state(None, None, None) == -1 and b'sekf_batch_set_state' in lib.srh_last_error()
    assert lib.sekf_batch_get_state(None, None, None, None) == -1 and b'sekf_batch_get_state' in lib.srh_last_error()
    assert lib.sekf_batch_plan(None, None, None, None, None) == -1 and b'sekf_batch_plan' in lib.srh_last_error()


@pytest.mark.parametrize('shape', bc.SHAPES, ids=str)
def test_members_meet_the_input_conditions(shape):
    from sofacontrol_amd import _lib
    assert _lib.ekf_plan(shape[1], shape[2])['path'] == ec.PATH_CODE[shape[0]]
    base = ec.case(ec.spec(shape))
    ops = bc.batch_operations(shape, range(bc.SMALL))
    assert [o[0] for o in ops[:2]] == ['reset', 'step'] and ops[1][2].shape == (bc.SMALL, shape[3]) and ops[1][3].shape == (bc.SMALL, shape[2])
    for b in range(bc.SMALL):
        c = bc.member(shape, b)
        assert c['C'] is base['C'] and c['W'] is base['W'] and c['model'] is base['model']
        traj, ref, e_oracle = bc.reference(shape, b)
        print('%s member %d: e_oracle %.2e, %d calls, points %s, least margin %.2e' % (shape, b, e_oracle, len(traj), sorted(set(ref.picks)), min(ref.margins)))
        assert len(traj) == c['steps'] + c['steps'] // 2 and len(ref.margins) == c['steps']
        assert e_oracle <= ec.E_ORACLE_MAX, (shape, b, e_oracle)
        assert min(ref.margins) > ec.MARGIN, (shape, b, min(ref.margins))
        assert len(set(ref.picks)) >= 3, (shape, b, ref.picks)
    # the members differ: they do not all walk the table points in the same order
    assert len({tuple(bc.reference(shape, b)[1].picks) for b in range(bc.SMALL)}) > 1
    # the failing covariance of the isolation test fails in long double at the last pivot
    import ekf_reference as er
    (name, Sigma, pivot), = [t for t in ec.indefinite_sigmas(base) if t[0] == 'last_pivot']
    c = bc.member(shape, bc.FAILING)
    with pytest.raises(np.linalg.LinAlgError) as info:
        er.update(c['C'], c['y_ref'], c['resets'][0], Sigma, c['y'][0], c['V'])
    assert info.value.pivot == pivot == shape[2] - 1
