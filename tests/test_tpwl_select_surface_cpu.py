"""CPU: the surface of the TPWL point selection exists -- the stpwl_select_* entry points declared in include/sofacontrol_hip.h and
exported by the built library, stpwl_select_plan answering on the host, tpwl.sysid.points_by_distance with its signature and re-export --
every refusal that is decided before a device call raises without a GPU and names what was wrong, and NULL arguments answer -1 and name
the entry point."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tpwl_select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['stpwl_select_plan', 'stpwl_select_points', 'stpwl_select_points_dev']
W = {'q': 1.0, 'v': 0.5}


def test_symbols_are_declared_and_exported():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    sysid._bind()
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in SYMBOLS:
        decl = re.search(r'^int\s+%s\s*\((.*?)\);' % name, code, flags=re.M | re.S)
        assert decl, name
        assert hasattr(_lib.lib(), name), name
        assert len(getattr(_lib.lib(), name).argtypes) == len(decl.group(1).split(',')), name
    unit = open(os.path.join(ROOT, 'soft-robot-control_amd', 'csrc', 'tpwl_select.hip')).read()
    assert 'atomicAdd' not in unit and 'mfma' not in unit.lower()     # no floating-point atomics, no |a|^2 - 2 a.b + |b|^2
    assert 'fma(e, e, s' in unit and 'hipStreamSynchronize' in unit
    assert len(re.findall(r'hipStreamSynchronize|hipDeviceSynchronize', unit.split('#include', 1)[1])) == 1                 # ONE host wait
    for text in (src, unit.split('#include')[0], open(os.path.join(ROOT, 'INTEGRATION.md')).read(), sysid.__doc__):
        for word in ('threshold', 'separate', 'max_points', 'seed', 'unconditionally', 'EVERY point', 'w_v == 0'):
            assert word in text, word


def test_plan_answers_on_the_host():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    p = sysid.select_plan(30, 4097)
    assert p['chunk'] == sc.C_DEFAULT and p['launches'] == 1 + 2 * 3 and 0 < p['lds_bytes'] <= 64 * 1024
    assert sysid.select_plan(30, sc.LARGE_CALL)['chunk'] == sc.C_DEFAULT
    p = sysid.select_plan(30, 4096 * 1001)                       # the Diamond records of the measurement
    assert p['chunk'] == sc.C_LARGE and p['launches'] == 1 + 2 * -(-4096 * 1001 // sc.C_LARGE)
    assert sysid.select_plan(1, 1) == {'chunk': sc.C_DEFAULT, 'lds_bytes': 256, 'launches': 3}
    with pytest.raises(RuntimeError, match=r'stpwl_select_plan: r = 0, need r >= 1'):
        sysid.select_plan(0, 10)
    with pytest.raises(RuntimeError, match=r'stpwl_select_plan: r = 129 exceeds the limit r <= 128'):
        sysid.select_plan(129, 10)
    with pytest.raises(RuntimeError, match=r'stpwl_select_plan: need candidates >= 1'):
        sysid.select_plan(4, 0)
    out = C.c_int(-5)
    assert _lib.lib().stpwl_select_plan(C.c_int(0), C.c_int64(5), C.byref(out), None, None) == -1 and out.value == 0


def test_python_surface():
    from sofacontrol_amd import tpwl
    from sofacontrol_amd.tpwl import sysid
    for name in ('points_by_distance', 'TPWLPointSelection', 'points_from_records', 'TPWLSysID'):
        assert getattr(tpwl, name) is getattr(sysid, name), name
    par = inspect.signature(sysid.points_by_distance).parameters
    assert list(par) == ['X', 'dist_weights', 'threshold', 'separate', 'stride', 'shape', 'q0', 'v0', 'max_points', 'stream']
    assert [par[k].default for k in list(par)[3:]] == [False, 1, None, None, None, 1024, None]
    sel = sysid.TPWLPointSelection(np.zeros((5, 2)), np.zeros((5, 2)), np.zeros((3, 2), dtype=np.int64), np.zeros(3), True, None, 77, seeded=2)
    assert '5 points' in repr(sel) and '77 candidates' in repr(sel)
    sel = sysid.TPWLPointSelection(np.zeros((5, 2)), np.zeros((5, 2)), np.zeros((3, 2), dtype=np.int64), np.zeros(3), False, (1, 8), 77)
    assert 'stopped at episode 1 row 8' in repr(sel)
    pfr = inspect.signature(sysid.points_from_records).parameters                       # unchanged
    assert list(pfr) == ['X', 'k', 'random_state', 'n_init', 'stride']
    assert 'distance heuristics' not in sysid.__doc__ and "'dynamics' rule" in sysid.__doc__


def test_refusals_on_the_host():
    """Every refusal of the rule comes before any device call: this test has no GPU."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import points_by_distance
    X = np.zeros((2, 9, 4))
    for thr in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(RuntimeError, match='need a finite threshold > 0'):
            points_by_distance(X, W, thr)
    for w, word in (({'q': -1.0, 'v': 0.0}, r"dist_weights\['q'\] = -1.0 is negative or not finite"),
                    ({'q': 1.0, 'v': np.nan}, r"dist_weights\['v'\] = nan is negative or not finite"),
                    ({'q': 1.0, 'v': np.inf}, r"dist_weights\['v'\] = inf is negative or not finite"),
                    ({'q': 0.0, 'v': 0.0}, 'both weights are zero'), ({'q': 1.0}, 'dist_weights must be')):
        with pytest.raises(RuntimeError, match=word):
            points_by_distance(X, w, 1.0)
    with pytest.raises(RuntimeError, match=r'n_x = 5, need n_x = 2 r with r >= 1'):
        points_by_distance(np.zeros((2, 9, 5)), W, 1.0)
    with pytest.raises(RuntimeError, match=r'n_x = 0, need n_x = 2 r with r >= 1'):
        points_by_distance(np.zeros((2, 9, 0)), W, 1.0)
    with pytest.raises(RuntimeError, match=r'X must have shape \(E, T, n_x\) or \(T, n_x\), got \(9,\)'):
        points_by_distance(np.zeros(9), W, 1.0)
    for stride in (0, -3, 1.5):
        with pytest.raises(RuntimeError, match='need an integer stride >= 1'):
            points_by_distance(X, W, 1.0, stride=stride)
    q0 = np.zeros((3, 2))
    bad = q0.copy()
    bad[1, 0] = np.inf
    with pytest.raises(RuntimeError, match='seed point 1 holds a non-finite entry'):
        points_by_distance(X, W, 1.0, q0=q0, v0=bad)
    with pytest.raises(RuntimeError, match='a seed needs both q0 and v0'):
        points_by_distance(X, W, 1.0, q0=q0)
    with pytest.raises(RuntimeError, match=r'must both have shape \(P0, r\) with r = 2, got \(3, 2\) and \(3, 3\)'):
        points_by_distance(X, W, 1.0, q0=q0, v0=np.zeros((3, 3)))
    for mp, P0 in ((0, 0), (1025, 0), (2, 3), (1.5, 0)):
        with pytest.raises(RuntimeError, match=r'max_points = .*, need an integer with max\(P0, 1\) = %d <= max_points <= 1024' % max(P0, 1)):
            points_by_distance(X, W, 1.0, q0=q0[:P0], v0=q0[:P0], max_points=mp)
    Xb = X.copy()
    Xb[1, 4, 3] = np.nan
    Xb[1, 6, 0] = np.inf
    with pytest.raises(RuntimeError, match='episode 1, row 4 of the records is not finite'):
        points_by_distance(Xb, W, 1.0)
    with pytest.raises(RuntimeError, match='episode 1, row 4 of the records is not finite'):
        points_by_distance(Xb, W, 1.0, stride=2)
    with pytest.raises(RuntimeError, match='episode 1, row 6 of the records is not finite'):
        points_by_distance(Xb, W, 1.0, stride=3)                # row 4 is not kept

    class Fake(_lib.DeviceBuffer):
        def __init__(self, nbytes):
            self.ptr, self.nbytes = C.c_void_p(), nbytes

    with pytest.raises(RuntimeError, match=r'DeviceBuffer records need shape = \(E, T\) or \(E, T, n_x\)'):
        points_by_distance(Fake(8 * 72), W, 1.0)
    with pytest.raises(RuntimeError, match='the DeviceBuffer is smaller than'):
        points_by_distance(Fake(8 * 71), W, 1.0, shape=(2, 9, 4))
    with pytest.raises(RuntimeError, match=r'n_x = 3, need n_x = 2 r'):
        points_by_distance(Fake(8 * 54), W, 1.0, shape=(2, 9))


def test_the_c_entry_points_refuse_before_any_device_call():
    """The same refusals at the C ABI (a caller without Python): SRH_EINVAL = -1, the entry point and what was wrong named."""
    from sofacontrol_amd.tpwl import sysid
    lib = sysid._bind()
    i64, ci, dbl = C.c_int64, C.c_int, C.c_double
    X = np.zeros((2, 9, 4))
    X[1, 4, 3] = np.nan
    xp = X.ctypes.data_as(C.POINTER(C.c_double))
    q0 = np.zeros((2, 2))
    q0p = q0.ctypes.data_as(C.POINTER(C.c_double))
    cnt = C.c_int(0)

    def call(r=2, stride=1, w_q=1.0, w_v=0.5, thr=1.0, P0=0, q=None, v=None, mp=16, count=cnt, x=xp, dev=False):
        args = [i64(2), i64(9), ci(r), ci(stride), dbl(w_q), dbl(w_v), dbl(thr), ci(0), ci(P0), q, v, ci(mp), None if count is None else C.byref(count),
                None, None, None, None, None, None]
        if dev:
            return lib.stpwl_select_points_dev(None if x is None else C.cast(x, C.c_void_p), *args, None)
        return lib.stpwl_select_points(x, *args)

    for kw, word in ((dict(x=None), b'null argument (x)'), (dict(count=None), b'null argument (count)'), (dict(r=0), b'r = 0, need r >= 1'),
                     (dict(thr=0.0), b'need a finite threshold > 0'), (dict(thr=float('nan')), b'need a finite threshold > 0'),
                     (dict(w_q=-1.0), b'w_q = -1 is negative or not finite'), (dict(w_v=float('inf')), b'w_v = inf is negative or not finite'),
                     (dict(w_q=0.0, w_v=0.0), b'both weights are zero'), (dict(stride=0), b'need stride >= 1'),
                     (dict(mp=0), b'max_points = 0, need max(P0, 1) = 1 <= max_points <= 1024'), (dict(mp=1025), b'<= max_points <= 1024'),
                     (dict(P0=2, mp=1, q=q0p, v=q0p), b'need max(P0, 1) = 2 <= max_points'), (dict(P0=2), b'needs q0 and v0'),
                     (dict(), b'episode 1, row 4 of the records is not finite')):
        assert call(**kw) == -1, kw
        assert b'stpwl_select_points:' in lib.srh_last_error() and word in lib.srh_last_error(), (kw, lib.srh_last_error())
    for kw, word in ((dict(x=None), b'null argument (x_dev)'), (dict(count=None), b'null argument (count)'), (dict(thr=-2.0), b'threshold')):
        assert call(dev=True, **kw) == -1, kw
        assert b'stpwl_select_points_dev:' in lib.srh_last_error() and word in lib.srh_last_error(), (kw, lib.srh_last_error())
    q0[1, 1] = np.nan
    assert call(P0=2, q=q0p, v=q0p) == -1 and b'seed point 1 holds a non-finite entry' in lib.srh_last_error()
