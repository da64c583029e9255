"""CPU: the surface of the Koopman fit exists -- every skoop_fit_* entry point declared in include/sofacontrol_hip.h and exported by the
built library, skoop_fit_plan answering on the host, baselines.koopman.sysid with the stated signatures -- every refusal that is decided
before a device call raises without a GPU, NULL handles answer -1 and name the entry point, and the new unit keeps the text pins of the
units beside it."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import koopman_fit_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['skoop_fit_plan', 'skoop_fit_create', 'skoop_fit_destroy', 'skoop_fit_reset', 'skoop_fit_minmax', 'skoop_fit_minmax_dev', 'skoop_fit_add',
           'skoop_fit_add_dev', 'skoop_fit_sums', 'skoop_fit_solve']


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    flat = re.sub(r'\s+', ' ', code)
    assert re.search(r'^typedef struct skoop_fit skoop_fit_t;', code, flags=re.M)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, code, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
    assert 'int skoop_fit_plan(int nzeta, int degree, int dmd, int m, int *n_psi, int *n, int *rows_per_chunk, int64_t *lds_bytes);' in flat
    assert 'int skoop_fit_create(skoop_fit_t **out, skoop_t *lift);' in flat
    assert re.search(r'int skoop_fit_add_dev\(skoop_fit_t \*f, const double \*y_dev, const double \*u_dev, int64_t E, int64_t T, int stride, '
                     r'int u_lag, void \*stream\);', flat)
    assert re.search(r'int skoop_fit_solve\(skoop_fit_t \*f, double ridge, double \*A, double \*B, int32_t \*info\);', flat)
    # the definition is restated where the issue asks for it
    unit = open(os.path.join(ROOT, 'soft-robot-control_amd', 'csrc', 'koopman_fit.hip')).read()
    for text in (src, unit.split('#include')[0], open(os.path.join(ROOT, 'INTEGRATION.md')).read()):
        for word in ('u_lag', 'ridge', 'stride', 'lasso', 'weights', 'G + ridge I'):
            assert word in text, word


def test_plan_answers_on_the_host():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.baselines.koopman import sysid
    from sofacontrol_amd.baselines.koopman.koopman_utils import num_observables
    for shape, n in kc.SHAPES.items():
        ny, m, d, degree, dmd = shape
        nz = ny * (d + 1) + m * d
        p = sysid.fit_plan(nz, degree, dmd, m)
        assert p['n'] == n and p['n_psi'] == num_observables(nz, degree, dmd) == n - m and p['rows_per_chunk'] == kc.TR
        assert 0 < p['lds_bytes'] <= 160 * 1024 and p['lds_bytes'] % 2560 == 0
    ny, m, d, degree, dmd = kc.REFUSED
    with pytest.raises(RuntimeError, match=r'n = n_psi \+ m = 120 \+ 9 = 129 exceeds the limit n <= 128'):
        sysid.fit_plan(ny, degree, dmd, m)
    lib = _lib.lib()
    assert lib.skoop_fit_plan(C.c_int(11), C.c_int(2), C.c_int(0), C.c_int(4), None, None, None, None) == 0
    out = C.c_int(-5)
    assert lib.skoop_fit_plan(C.c_int(14), C.c_int(2), C.c_int(0), C.c_int(9), C.byref(out), None, None, None) == -1 and out.value == 0
    for bad in ((65, 1, 1), (3, 5, 1), (0, 2, 1), (3, 2, 0)):
        assert lib.skoop_fit_plan(C.c_int(bad[0]), C.c_int(bad[1]), C.c_int(0), C.c_int(bad[2]), None, None, None, None) == -1
        assert b'skoop_fit_plan' in lib.srh_last_error()


def test_python_surface():
    from sofacontrol_amd.baselines.koopman import sysid
    sig = inspect.signature(sysid.KoopmanSysID.__init__).parameters
    assert list(sig) == ['self', 'n_y', 'm', 'Ts', 'obs_degree', 'delays', 'DMD', 'scale']
    assert (sig['obs_degree'].default, sig['delays'].default, sig['DMD'].default, sig['scale'].default) == (2, 1, False, None)
    add = inspect.signature(sysid.KoopmanSysID.add).parameters
    assert list(add)[:5] == ['self', 'Y', 'U', 'stride', 'u_lag'] and add['stride'].default == 1 and add['u_lag'].default == 0
    assert inspect.signature(sysid.KoopmanSysID.solve).parameters['ridge'].default == 0.0
    for name in ('sums', 'reset', 'solve'):
        assert callable(getattr(sysid.KoopmanSysID, name)), name
    assert isinstance(sysid.KoopmanSysID.pairs, property)
    fk = inspect.signature(sysid.fit_koopman).parameters
    assert list(fk)[:3] == ['Y', 'U', 'Ts'] and fk['ridge'].default == 0.0 and fk['u_lag'].default == 0 and fk['stride'].default == 1
    assert list(inspect.signature(sysid.one_step_error).parameters)[:3] == ['model', 'Y', 'U']
    r = sysid.KoopmanFitResult(5, 0.1, 0.2)
    assert (r.pairs, r.ridge, r.residual_rms) == (5, 0.1, 0.2)
    for word in ('u_lag', 'stride', 'ridge', 'lasso', 'weights', 'non-polynomial', 'truncation', 'max == min', 'n = P + m <= 128'):
        assert word in sysid.__doc__, word


def test_refusals_on_the_host():
    """Argument checks that come before any device call: no handle exists yet when they raise."""
    from sofacontrol_amd.baselines.koopman.sysid import KoopmanSysID, fit_koopman
    with pytest.raises(RuntimeError, match='exceeds the limit n <= 128'):
        KoopmanSysID(14, 9, 0.05, obs_degree=2, delays=0)
    with pytest.raises(RuntimeError, match='truncated models are not fitted'):
        KoopmanSysID.for_lift(types.SimpleNamespace(has_w=True), 0.05)
    one = dict(y_offset=np.zeros(3), y_factor=np.ones(3), u_offset=np.zeros(4), u_factor=np.ones(4))
    with pytest.raises(RuntimeError, match=r'channel u\[2\] is constant'):
        KoopmanSysID(3, 4, 0.05, scale=dict(one, u_factor=np.array([1.0, 2.0, 0.0, 1.0])))
    with pytest.raises(RuntimeError, match=r"scale\['y_offset'\] must have 3 entries, got 2"):
        KoopmanSysID(3, 4, 0.05, scale=dict(one, y_offset=np.zeros(2)))
    with pytest.raises(RuntimeError, match='need n_y, m, obs_degree >= 1, delays >= 0 and Ts > 0'):
        KoopmanSysID(3, 4, 0.0)
    sid = KoopmanSysID(3, 4, 0.05, scale=one)
    assert sid._lift is None and sid.pairs == 0 and (sid.n_psi, sid.n, sid.nzeta) == (66, 70, 10)
    Y, U = np.zeros((2, 9, 3)), np.zeros((2, 9, 4))
    with pytest.raises(RuntimeError, match=r'Y must have shape \(E, T, n_y\) or \(T, n_y\) with n_y = 3, got \(2, 9, 4\)'):
        sid.add(U, U)
    with pytest.raises(RuntimeError, match=r'U \(E, T, m\) must have shape \(2, 9, 4\), got \(2, 8, 4\)'):
        sid.add(Y, U[:, :8])
    with pytest.raises(RuntimeError, match=r'U \(E, T, m\) must have shape \(1, 9, 4\), got \(1, 9, 3\)'):
        sid.add(Y[0], Y[0])
    for u_lag in (2, -1, 0.5):
        with pytest.raises(RuntimeError, match='u_lag = .*need 0 .* or 1'):
            sid.add(Y, U, u_lag=u_lag)
    for stride in (0, -3, 1.5):
        with pytest.raises(RuntimeError, match='need an integer stride >= 1'):
            sid.add(Y, U, stride=stride)
    with pytest.raises(RuntimeError, match=r'no pairs have been added \(S = 0\)'):
        sid.solve()
    with pytest.raises(RuntimeError, match='need a finite ridge >= 0'):
        sid.solve(-1.0)
    with pytest.raises(RuntimeError, match='u_lag'):
        fit_koopman(Y, U, 0.05, u_lag=3)
    assert sid._lift is None                                       # nothing reached the device
    assert sid.sums()['pairs'] == 0 and sid.sums()['G'].shape == (70, 70)
    sid.reset()


def test_null_handles_answer_minus_one_and_name_the_entry_point():
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    i64, ci, dbl = C.c_int64, C.c_int, C.c_double
    calls = {
        'skoop_fit_create': lambda: lib.skoop_fit_create(None, None),
        'skoop_fit_destroy': lambda: lib.skoop_fit_destroy(None),
        'skoop_fit_reset': lambda: lib.skoop_fit_reset(None),
        'skoop_fit_minmax': lambda: lib.skoop_fit_minmax(None, None, i64(1), i64(4), ci(1), ci(1), ci(1), None, None, None, None),
        'skoop_fit_minmax_dev': lambda: lib.skoop_fit_minmax_dev(None, None, i64(1), i64(4), ci(1), ci(1), ci(1), None, None, None, None, None),
        'skoop_fit_add': lambda: lib.skoop_fit_add(None, None, None, i64(1), i64(4), ci(1), ci(0)),
        'skoop_fit_add_dev': lambda: lib.skoop_fit_add_dev(None, None, None, i64(1), i64(4), ci(1), ci(0), None),
        'skoop_fit_sums': lambda: lib.skoop_fit_sums(None, None, None, None, None),
        'skoop_fit_solve': lambda: lib.skoop_fit_solve(None, dbl(0.0), None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() + b':' in lib.srh_last_error(), (name, lib.srh_last_error())


def test_the_unit_keeps_the_text_pins():
    csrc = os.path.join(ROOT, 'soft-robot-control_amd', 'csrc')
    unit = open(os.path.join(csrc, 'koopman_fit.hip')).read()
    assert '#include "koopman_host.h"' in unit and '#include "dev_la.h"' in unit
    for text in ('struct skoop {', 'struct KoopLiftArgs {', 'int koop_launch_lift(', 'ext_vector_type(2)', 'At[q * n + j]', 'th * (hi - lo)',
                 'loop_prepare_kernel<<<', 'int sgusto_loop_schedule', 'atomicAdd', 'unsafeAtomicAdd'):
        assert text not in unit, text
    for text in ('__builtin_amdgcn_mfma_f64_16x16x4f64', 'ext_vector_type(4)', 'kf_accum_kernel', 'kf_reduce_kernel', 'kf_minmax_kernel',
                 'kf_solve_kernel', 'THE FIT', 'h->par.as<int32_t>()', 'h->scale.as<double>()', 'has_w'):
        assert text in unit, text
    assert 'constexpr int KF_TR = %d;' % kc.TR in unit
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert re.search(r'^koopman\.o koopman_loop\.o: koopman_host\.h$', mk, flags=re.M)
    assert re.search(r'^koopman_fit\.o: koopman_host\.h$', mk, flags=re.M)
