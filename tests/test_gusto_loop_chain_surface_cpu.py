"""CPU: the surface of the chained policy (the reference's mpc=False) exists -- the four entry points declared in
include/sofacontrol_hip.h and exported by the built library, the Python keywords and helpers with the stated defaults -- and the parts
that need no device answer: the end row of the schedule (Python statement, direct statement and the library's own, bit for bit), and
the refusals that come before any device call."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import cl_cases as cc
import cl_chain_reference as ch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHAIN_SYMBOLS = ['sgusto_loop_set_chained', 'sgusto_loop_run_tape', 'sgusto_loop_end_row', 'sgusto_loop_chain']


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read(), flags=re.S)


def test_chain_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = header()
    for name in CHAIN_SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, src, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^int\s+sgusto_loop_set_chained\s*\(sgusto_loop_t \*h, int on\)', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_loop_chain\s*\(sgusto_loop_t \*h, const double \*xopt, const double \*uopt, double \*x_next, '
                     r'double \*Xbar_rows, double \*Ubar_rows\)', src, flags=re.M)
    assert re.search(r'^int\s+sgusto_loop_run_tape\s*\(sgusto_loop_t \*h, int periods, const double \*W, const double \*V, double \*X_cl, '
                     r'double \*Z_cl, double \*U_cl,\s*int32_t \*iters, int32_t \*status, double \*J, double \*Xhat, double \*Y_cl, '
                     r'int32_t \*ekf_status, double \*Xbar, double \*Ubar\)', src, flags=re.M)
    # the earlier entry points keep their signatures
    assert re.search(r'^int\s+sgusto_loop_run\s*\(sgusto_loop_t \*h, int periods, const double \*W, double \*X_cl, double \*Z_cl, double \*U_cl, '
                     r'int32_t \*iters,\s*int32_t \*status, double \*J\)', src, flags=re.M)


def test_one_chain_kernel_one_launch_and_the_plan_point_rule():
    """loop_chain_kernel is one kernel with one launch, in gusto_loop.hip; it forms its values by plan_at alone; the shared device
    header does not know about it."""
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    assert [f for f, u in units.items() if 'loop_chain_kernel' in u] == ['gusto_loop.hip']
    unit = units['gusto_loop.hip']
    assert unit.count('loop_chain_kernel<<<') == 1 and unit.count('void loop_chain_kernel(') == 1
    body = unit.split('void loop_chain_kernel(')[1].split('\n}\n')[0]
    assert body.count('plan_at(') == 2 and 'atomic' not in body and '__shared__' not in body and 'asm' not in body


def test_python_surface():
    from sofacontrol_amd.scp import closed_loop
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch, ClosedLoopResult
    init = inspect.signature(ClosedLoopBatch.__init__).parameters
    assert init['mpc'].default is True and init['record_tape'].default is False
    assert list(init)[:10] == ['self', 'gusto', 'plant', 'dt_sim', 'n_keep', 't', 'z', 'u', 'phase', 'K']
    assert list(inspect.signature(closed_loop.schedule_end).parameters) == ['N', 'dt', 'dt_sim', 'n_keep']
    assert list(inspect.signature(ClosedLoopBatch._chain).parameters) == ['self', 'xopt', 'uopt']
    assert callable(ClosedLoopBatch.set_record_tape)
    doc = ClosedLoopBatch.__init__.__doc__
    assert "REFERENCE's default" in doc and 'controllers.py:236' in doc
    res = ClosedLoopResult(*range(7))
    assert res.x_bar is None and res.u_bar is None
    res = ClosedLoopResult(*range(7), x_hat=7, y=8, ekf_status=9, x_bar=10, u_bar=11)
    assert (res.x_hat, res.y, res.ekf_status, res.x_bar, res.u_bar) == (7, 8, 9, 10, 11)


@pytest.mark.parametrize('dt_sim,n_keeps', [(0.05, (1, 12, 10, 5)), (0.01, (1, 60, 10, 59)), (0.03, (1, 20, 10, 7))])
def test_end_row_equals_the_direct_statement_and_the_library(dt_sim, n_keeps):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import schedule_end
    for n_keep in n_keeps:
        for N, dt in ((cc.N, cc.DT), (3, 0.2), (25, 0.024)):
            if n_keep * dt_sim > N * dt:
                continue
            j, theta = schedule_end(N, dt, dt_sim, n_keep)
            dj, dtheta = ch.direct_end(N, dt, dt_sim, n_keep)
            lj, ltheta = _lib.gusto_loop_end_row(N, dt, dt_sim, n_keep)
            assert j == dj == lj, (N, dt, n_keep)
            assert np.float64(theta).tobytes() == np.float64(dtheta).tobytes() == np.float64(ltheta).tobytes(), (N, dt, n_keep)
            assert 0 <= j <= N - 1 and 0.0 <= theta <= 1.0 + 1e-12
    lib = _lib.lib()
    assert lib.sgusto_loop_end_row(C.c_int(12), C.c_double(0.05), C.c_double(0.01), C.c_int(10), None, None) == 0
    assert lib.sgusto_loop_end_row(C.c_int(0), C.c_double(0.05), C.c_double(0.01), C.c_int(10), None, None) == -1
    assert b'sgusto_loop_end_row' in lib.srh_last_error()


def test_refusals_on_the_host():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    lib = _lib.lib()
    assert lib.sgusto_loop_set_chained(None, C.c_int(1)) == -1 and b'sgusto_loop_set_chained' in lib.srh_last_error()
    assert lib.sgusto_loop_run_tape(None, C.c_int(1), *[None] * 13) == -1 and b'sgusto_loop_run_tape' in lib.srh_last_error()
    assert lib.sgusto_loop_chain(None, None, None, None, None, None) == -1 and b'sgusto_loop_chain' in lib.srh_last_error()
    # the checks of the constructor that come first are those of every policy
    fused = types.SimpleNamespace(_fused=True, _ssm=False, N=12, dt=0.05, batch=3)
    with pytest.raises(RuntimeError, match=r'n_keep \* dt_sim = 0\.61 exceeds the horizon N \* dt = 0\.6'):
        ClosedLoopBatch(fused, None, 0.01, 61, mpc=False)
    with pytest.raises(RuntimeError, match='fused resident plan'):
        ClosedLoopBatch(types.SimpleNamespace(_fused=False, _ssm=False, N=12, dt=0.05), None, 0.01, 10, mpc=False, record_tape=True)
    # a tape without the chained policy: refused by name, on a loop that was never created
    shell = ClosedLoopBatch.__new__(ClosedLoopBatch)
    shell.mpc, shell.record_tape, shell._h = True, False, None
    with pytest.raises(RuntimeError, match='record_tape=True needs mpc=False'):
        shell.set_record_tape(True)
    assert shell.set_record_tape(False) is shell
    shell.mpc = False
    assert shell.set_record_tape(True).record_tape is True
    shell.B, shell.N, shell.n_x, shell.n_u, shell.n_keep = 3, 12, 8, 3, 10
    with pytest.raises(RuntimeError, match=r'_chain: xopt must have shape \(B, N \+ 1, n_x\) = \(3, 13, 8\)'):
        shell._chain(np.zeros((3, 12, 8)), np.zeros((3, 12, 3)))
