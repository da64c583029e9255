"""CPU: the surface of the TPWL fit exists -- every stpwl_fit_* entry point declared in include/sofacontrol_hip.h and exported by the
built library, stpwl_fit_plan answering on the host, tpwl.sysid with the stated signatures -- every refusal that is decided before a
device call raises without a GPU, and NULL handles answer -1 and name the entry point."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tpwl_fit_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['stpwl_fit_plan', 'stpwl_fit_create', 'stpwl_fit_destroy', 'stpwl_fit_reset', 'stpwl_fit_add', 'stpwl_fit_add_dev',
           'stpwl_fit_counts', 'stpwl_fit_sums', 'stpwl_fit_solve']


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    sysid._bind()
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'^typedef struct stpwl_fit stpwl_fit_t;', code, flags=re.M)
    for name in SYMBOLS:
        assert re.search(r'^int\s+%s\s*\(' % name, code, flags=re.M), name
        assert hasattr(_lib.lib(), name), name
        assert getattr(_lib.lib(), name).argtypes is not None, name
    # the argument counts of the ctypes signatures are those of the declarations
    for name in SYMBOLS:
        decl = re.search(r'^int\s+%s\s*\((.*?)\);' % name, code, flags=re.M | re.S).group(1)
        assert len(getattr(_lib.lib(), name).argtypes) == len(decl.split(',')), name
    unit = open(os.path.join(ROOT, 'soft-robot-control_amd', 'csrc', 'tpwl_fit.hip')).read()
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64' in unit and 'tpwl::nearest_wave' in unit
    assert re.findall(r'atomicAdd\(([^,]*),', unit) == ['&tf_hist[p]']                    # the one atomic add is the integer histogram's
    for text in (src, unit.split('#include')[0], open(os.path.join(ROOT, 'INTEGRATION.md')).read(), sysid.__doc__):
        for word in ('stride', 'ridge', 'x_p', 'D^-1/2', '/ Ts', 'd_c', 'first'):
            assert word in text, word


def test_plan_answers_on_the_host():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    p = sysid.fit_plan(64, 30, 4)                                # the shipped Diamond shape: n_x = 60, m = 4
    assert p['n'] == 65 and p['rows_per_chunk'] == fr.TR and 0 < p['lds_bytes'] <= 160 * 1024 and p['lds_bytes'] % 2560 == 0
    p = sysid.fit_plan(8, 36, 4)
    assert p['n'] == 77
    p = sysid.fit_plan(2, 60, 7)                                 # the limit itself: 36 + 64 tiles, 25 per wave
    assert p['n'] == 128 == sysid.MAX_N and p['tiles_per_wave'] == 25 and p['lds_bytes'] <= 160 * 1024
    assert sysid.fit_plan(1024, 4, 3)['n'] == 12
    with pytest.raises(RuntimeError, match=r'stpwl_fit_plan: n = n_x \+ m \+ 1 = 120 \+ 8 \+ 1 = 129 exceeds the limit n <= 128'):
        sysid.fit_plan(2, 60, 8)
    with pytest.raises(RuntimeError, match=r'stpwl_fit_plan: P = 1025 exceeds the limit P <= 1024'):
        sysid.fit_plan(1025, 4, 3)
    with pytest.raises(RuntimeError, match=r'stpwl_fit_plan: m = 17 exceeds the limit m <= 16'):
        sysid.fit_plan(4, 4, 17)
    lib = _lib.lib()
    out = C.c_int(-5)
    assert lib.stpwl_fit_plan(C.c_int(2), C.c_int(60), C.c_int(8), C.byref(out), None, None, None) == -1 and out.value == 0
    for bad in ((0, 4, 3), (4, 0, 3), (4, 4, 0), (4, 64, 1)):
        assert lib.stpwl_fit_plan(*[C.c_int(v) for v in bad], None, None, None, None) == -1, bad
        assert b'stpwl_fit_plan' in lib.srh_last_error()


def test_python_surface():
    from sofacontrol_amd import tpwl
    from sofacontrol_amd.tpwl import sysid
    for name in ('TPWLSysID', 'TPWLFitResult', 'fit_tpwl', 'one_step_error', 'points_from_records'):
        assert getattr(tpwl, name) is getattr(sysid, name), name
    assert list(inspect.signature(sysid.TPWLSysID.__init__).parameters) == ['self', 'q', 'v', 'dist_weights', 'm', 'Ts']
    add = inspect.signature(sysid.TPWLSysID.add).parameters
    assert list(add) == ['self', 'X', 'U', 'stride', 'shape', 'stream'] and add['stride'].default == 1
    st = inspect.signature(sysid.TPWLSysID.solve_tables).parameters
    assert list(st) == ['self', 'ridge', 'min_samples'] and (st['ridge'].default, st['min_samples'].default) == (0.0, None)
    so = inspect.signature(sysid.TPWLSysID.solve).parameters
    assert list(so) == ['self', 'rom_info', 'ridge', 'min_samples', 'on_fail', 'Cf', 'Hf'] and so['on_fail'].default == 'raise'
    for name in ('counts', 'sums', 'reset'):
        assert callable(getattr(sysid.TPWLSysID, name)), name
    ose = inspect.signature(sysid.one_step_error).parameters
    assert list(ose)[:5] == ['model', 'X', 'U', 'stride', 'worst'] and ose['worst'].default is False
    pfr = inspect.signature(sysid.points_from_records).parameters
    assert list(pfr)[:4] == ['X', 'k', 'random_state', 'n_init'] and (pfr['random_state'].default, pfr['n_init'].default) == (0, 10)
    r = sysid.TPWLFitResult(5, np.array([5, 0]), np.array([0, 1]), np.array([-1, -1]), 0.1, np.array([1.0, np.nan]), np.array([0.5, np.nan]))
    assert r.samples == 5 and r.ridge == 0.1 and 'solved=1' in repr(r)
    assert [sysid.column_name(c, 8, 3) for c in (6, 9, 11)] == ['state x7', 'input u2', 'constant']
    for word in ('Two `add`', 'n = n_x + m + 1 <= 128', 'weighting-mode', 'sample weights', 'compute_RO_state'):
        assert word in sysid.__doc__, word


def test_refusals_on_the_host():
    """Argument checks that come before any device call: no handle exists yet when they raise."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import TPWLSysID, fit_tpwl
    q, v, w = np.zeros((3, 4)), np.zeros((3, 4)), {'q': 1.0, 'v': 0.0}
    with pytest.raises(RuntimeError, match=r'q and v must both have shape \(P, r\), got \(3, 4\) and \(3, 5\)'):
        TPWLSysID(q, np.zeros((3, 5)), w, 3, 0.01)
    with pytest.raises(RuntimeError, match="dist_weights must be"):
        TPWLSysID(q, v, {'q': 1.0}, 3, 0.01)
    with pytest.raises(RuntimeError, match='need a finite Ts > 0'):
        TPWLSysID(q, v, w, 3, 0.0)
    with pytest.raises(RuntimeError, match='exceeds the limit n <= 128'):
        TPWLSysID(np.zeros((2, 60)), np.zeros((2, 60)), w, 8, 0.01)
    with pytest.raises(RuntimeError, match='non-finite'):
        TPWLSysID(np.full((3, 4), np.nan), v, w, 3, 0.01)
    sid = TPWLSysID(q, v, w, 3, 0.01)
    assert not sid._h and sid.samples == 0 and (sid.P, sid.r, sid.n_x, sid.n) == (3, 4, 8, 12)
    X, U = np.zeros((2, 9, 8)), np.zeros((2, 9, 3))
    with pytest.raises(RuntimeError, match=r'X must have shape \(E, T, n_x\) or \(T, n_x\) with n_x = 8, got \(2, 9, 3\)'):
        sid.add(U, U)
    with pytest.raises(RuntimeError, match=r'U \(E, T, m\) must have shape \(2, 9, 3\), got \(2, 8, 3\)'):
        sid.add(X, U[:, :8])
    for stride in (0, -3, 1.5):
        with pytest.raises(RuntimeError, match='need an integer stride >= 1'):
            sid.add(X, U, stride=stride)

    class Fake(_lib.DeviceBuffer):
        def __init__(self, nbytes):
            self.ptr, self.nbytes = C.c_void_p(), nbytes

    with pytest.raises(RuntimeError, match=r'DeviceBuffer records need shape = \(E, T\)'):
        sid.add(Fake(8 * 144), Fake(8 * 54))
    with pytest.raises(RuntimeError, match='both be arrays or both be DeviceBuffers'):
        sid.add(Fake(8 * 144), U)
    with pytest.raises(RuntimeError, match='the DeviceBuffers are smaller than'):
        sid.add(Fake(8 * 143), Fake(8 * 54), shape=(2, 9))
    rom = dict(type='POD')
    with pytest.raises(RuntimeError, match=r'no samples have been added \(S = 0\)'):
        sid.solve(rom)
    with pytest.raises(RuntimeError, match=r'no samples have been added \(S = 0\)'):
        sid.solve_tables()
    with pytest.raises(RuntimeError, match="on_fail = 'skip', need 'raise' or 'drop'"):
        sid.solve(rom, on_fail='skip')
    with pytest.raises(RuntimeError, match='need a finite ridge >= 0'):
        sid.solve_tables(-1.0)
    with pytest.raises(RuntimeError, match='min_samples = 0, need an integer >= 1'):
        sid.solve_tables(min_samples=0)
    with pytest.raises(RuntimeError, match=r'point 3 is outside 0 \.\. 2'):
        sid.sums(3)
    with pytest.raises(RuntimeError, match='DeviceBuffer records need m'):
        fit_tpwl(Fake(8), Fake(8), q, v, w, 0.01, rom, shape=(1, 1))
    assert not sid._h                                              # nothing reached the device
    assert sid.counts().tolist() == [0, 0, 0] and sid.sums(0)['G'].shape == (12, 12) and sid.sums(0)['samples'] == 0
    sid.reset()


def test_null_handles_answer_minus_one_and_name_the_entry_point():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    lib = sysid._bind()
    i64, ci, dbl = C.c_int64, C.c_int, C.c_double
    calls = {
        'stpwl_fit_create': lambda: lib.stpwl_fit_create(None, ci(2), ci(3), ci(1), None, None, dbl(1.0), dbl(0.0), dbl(0.01)),
        'stpwl_fit_destroy': lambda: lib.stpwl_fit_destroy(None),
        'stpwl_fit_reset': lambda: lib.stpwl_fit_reset(None),
        'stpwl_fit_add': lambda: lib.stpwl_fit_add(None, None, None, i64(1), i64(4), ci(1)),
        'stpwl_fit_add_dev': lambda: lib.stpwl_fit_add_dev(None, None, None, i64(1), i64(4), ci(1), None),
        'stpwl_fit_counts': lambda: lib.stpwl_fit_counts(None, None),
        'stpwl_fit_sums': lambda: lib.stpwl_fit_sums(None, ci(0), None, None, None, None),
        'stpwl_fit_solve': lambda: lib.stpwl_fit_solve(None, dbl(0.0), i64(-1), None, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() + b':' in lib.srh_last_error(), (name, lib.srh_last_error())
