"""CPU: the surface of the TPWL horizon error exists -- the three stpwl_horizon_* entry points declared in include/sofacontrol_hip.h with
the parameters the ctypes binding gives them and exported by the built library, horizon_plan answering on the host, horizon_error with
its signature and re-export -- and every refusal that is decided before a device call raises without a GPU and names what was wrong."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['stpwl_horizon_plan', 'stpwl_horizon_error', 'stpwl_horizon_error_dev']
CTYPE = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double, 'int *': C.POINTER(C.c_int), 'int64_t *': C.POINTER(C.c_int64),
         'double *': C.POINTER(C.c_double), 'const double *': C.POINTER(C.c_double), 'int32_t *': C.POINTER(C.c_int32), 'void *': C.c_void_p,
         'stpwl_t *': C.c_void_p}


class Model:
    """What horizon_error reads of a model before it touches the device: no GPU behind it."""

    def __init__(self, r=30, m=4, P=64, n_z=3, w_v=0.0, method='nn'):
        self.tpwl_method, self.num_points, self.dist_weights = method, P, {'q': 1.0, 'v': w_v}
        self._n, self._m, self._nz = 2 * r, m, n_z
        self.H = np.zeros((n_z, 2 * r)) if n_z else None
        self.fit_Ts = 0.01

    def get_state_dim(self):
        return self._n

    def get_input_dim(self):
        return self._m

    def get_output_dim(self):
        return self._nz

    def handle_for(self, dt):
        raise AssertionError('the device handle was asked for: the refusal did not come on the host')


def test_header_declarations_equal_the_argtypes_and_the_symbols_are_exported():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl import sysid
    lib = sysid._bind()
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in SYMBOLS:
        decl = re.search(r'^int\s+%s\s*\((.*?)\);' % name, code, flags=re.M | re.S)
        assert decl, name
        assert hasattr(lib, name), name
        params = [re.sub(r'\s+', ' ', p.strip()) for p in decl.group(1).split(',')]
        types = [re.match(r'(.*?)(\w+)$', p).group(1).strip() for p in params]
        got = getattr(lib, name).argtypes
        assert len(got) == len(types), name
        for i, (t, g) in enumerate(zip(types, got)):
            want = CTYPE[t]
            if name.endswith('_dev') and params[i].endswith('_dev'):
                want = C.c_void_p                                # device pointers travel as addresses
            assert g is want or (g is _lib.c_double_p and want is CTYPE['double *']), (name, params[i], g)
    unit = open(os.path.join(ROOT, 'soft-robot-control_amd', 'csrc', 'tpwl_horizon.hip')).read()
    body = unit.split('#include', 1)[1]
    assert 'atomicAdd' not in unit and 'atomicMax' not in unit                      # no floating-point atomics (the flags are integer ORs)
    assert len(re.findall(r'hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy\(', body)) == 1          # exactly ONE host wait in the unit
    for word in ('tpwl::nearest_wave', 'tpwl::panel_load', 'tpwl::step_slices', 'tpwl::step_sum', 'tpwl::step_l2', 'tpwl::wave_first_min'):
        assert word in body, word                                 # the step and the search are called, not restated
    for text in (src, unit.split('#include')[0], open(os.path.join(ROOT, 'INTEGRATION.md')).read(), sysid.__doc__):
        for word in ('every', 'j0 + H <= T\' - 1', 'status', '2 wins over 1', 'lowest window number', 'exactly 0', 'z_ref cancels'):
            assert word in text, word


def test_python_surface():
    from sofacontrol_amd import tpwl
    from sofacontrol_amd.tpwl import sysid
    for name in ('horizon_error', 'horizon_plan', 'TPWLHorizonError', 'one_step_error'):
        assert getattr(tpwl, name) is getattr(sysid, name), name
    par = inspect.signature(sysid.horizon_error).parameters
    assert list(par) == ['model', 'X', 'U', 'horizon', 'dt', 'stride', 'every', 'shape', 'per_window', 'predictions']
    assert [par[k].default for k in list(par)[4:]] == [None, 1, 1, None, False, False]
    assert list(inspect.signature(sysid.one_step_error).parameters) == ['model', 'X', 'U', 'stride', 'worst', 'Ts']       # unchanged
    for word in ('Koopman and SSM analogues', 'weighting-mode models', 'closed-loop (feedback) prediction', "error weights other than the\n  model's H"):
        assert word in sysid.__doc__, word
    res = sysid.TPWLHorizonError(5, 0.01, 10, 1, 2, np.zeros(6), np.ones(6), np.zeros(6), np.zeros((6, 2), dtype=np.int64))
    assert res.windows_ok == 7 and '10 windows (1 diverged, 2 with bad rows)' in repr(res)


def test_plan_answers_on_the_host():
    from sofacontrol_amd.tpwl import sysid
    # the Diamond shape of the measurement: n_x = 60, m = 4, P = 64, T = 1001, H = 50, every 10
    p = sysid.horizon_plan(Model(), 256, 1001, 50, every=10)
    assert p['windows'] == 256 * 96 and p['block'] == 16 and p['blocks'] == 256 * 6 and p['mode'] == 'staged_held' and p['launches'] == 2
    assert p['lds_bytes'] % 2560 == 0 and 8 * (2 * 60 + 4 + 8 * 51 + 2 + 2 * 256 + 60 * 60 + 4 * 60 + 60) <= p['lds_bytes'] <= 160 * 1024 // 4
    assert p['pred_cap_bytes'] == 256 << 20
    p = sysid.horizon_plan(Model(), 4096, 1001, 50, every=10)
    assert p['windows'] == 4096 * 96 and p['block'] == 128 and p['blocks'] == 4096              # more episodes than blocks: one block per episode
    p = sysid.horizon_plan(Model(), 300, 1001, 50, every=1)
    assert p['block'] == 256 and p['blocks'] == 300 * 4 and p['windows'] == 300 * 951
    assert sysid.horizon_plan(Model(w_v=0.5), 1, 52, 50)['mode'] == 'staged' and sysid.horizon_plan(Model(P=65), 1, 52, 50)['mode'] == 'staged'
    assert sysid.horizon_plan(Model(r=33), 1, 52, 50)['mode'] == 'staged'
    # n_x = 128, m = 16: the panel alone is 148 480 bytes; staged while the accumulators fit the 160 KB, the L2-fed step above
    big = Model(r=64, m=16, P=3)
    # (19 346 + 8 (H + 1) doubles against 20 480: H <= 140)
    for H, mode in ((3, 'staged'), (140, 'staged'), (141, 'l2'), (1024, 'l2')):
        p = sysid.horizon_plan(big, 1, H + 1, H)
        assert p['mode'] == mode and p['lds_bytes'] <= 160 * 1024, (H, p)
    assert sysid.horizon_plan(Model(r=42), 1, 2, 1)['mode'] == 'staged'                          # (the rollout's own 64 KB limit is not this unit's)
    # strides and window steps
    assert sysid.horizon_plan(Model(), 2, 38, 4, stride=3)['windows'] == 2 * 9                   # T' = 13
    assert sysid.horizon_plan(Model(), 2, 38, 12, stride=3, every=50)['windows'] == 2


def test_refusals_on_the_host():
    """Every refusal comes before any device call: this test has no GPU (Model.handle_for raises)."""
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import horizon_error, horizon_plan
    X, U = np.zeros((2, 9, 60)), np.zeros((2, 9, 4))
    with pytest.raises(RuntimeError, match=r"tpwl_method = 'weighting': only nearest-point \('nn'\) models are offered, not weighting-mode models"):
        horizon_error(Model(method='weighting'), X, U, 3)
    with pytest.raises(RuntimeError, match=r'stpwl_horizon_plan: n_x = 130 exceeds the limit n_x <= 128'):
        horizon_error(Model(r=65), np.zeros((2, 9, 130)), U, 3)
    with pytest.raises(RuntimeError, match=r'stpwl_horizon_plan: H = 1025, need 1 <= H <= 1024'):
        horizon_error(Model(), np.zeros((1, 1030, 60)), np.zeros((1, 1030, 4)), 1025)
    with pytest.raises(RuntimeError, match=r'stpwl_horizon_plan: m = 17, need 1 <= m <= 16'):
        horizon_plan(Model(m=17), 2, 9, 3)
    with pytest.raises(RuntimeError, match=r"stpwl_horizon_plan: W = 0 windows: T' = 9 kept rows per episode, H = 9 needs T' >= 10"):
        horizon_error(Model(), X, U, 9)
    with pytest.raises(RuntimeError, match=r"W = 0 windows: T' = 3 kept rows"):
        horizon_error(Model(), X, U, 3, stride=4)
    for kw, word in ((dict(stride=0), 'need an integer stride >= 1'), (dict(every=0), 'every = 0, need an integer every >= 1'),
                     (dict(every=1.5), 'every = 1.5, need an integer every >= 1')):
        with pytest.raises(RuntimeError, match=word):
            horizon_error(Model(), X, U, 3, **kw)
    with pytest.raises(RuntimeError, match='horizon = 0, need an integer horizon >= 1'):
        horizon_error(Model(), X, U, 0)
    # predictions over the cap: 4096 x 96 windows x 51 rows x 60 doubles = 9.6 GB
    cap = horizon_plan(Model(), 4096, 1001, 50, every=10)['pred_cap_bytes']

    class Fake(_lib.DeviceBuffer):
        def __init__(self, nbytes):
            self.ptr, self.nbytes = C.c_void_p(), nbytes

    with pytest.raises(RuntimeError, match=r'predictions of 393216 windows x 51 rows x 60 need 9625927680 bytes, above the cap of %d bytes' % cap):
        horizon_error(Model(), Fake(8 * 4096 * 1001 * 60), Fake(8 * 4096 * 1001 * 4), 50, every=10, shape=(4096, 1001), predictions=True)
    with pytest.raises(RuntimeError, match='X and U must both be arrays or both be DeviceBuffers'):
        horizon_error(Model(), X, Fake(8 * 2 * 9 * 4), 3, shape=(2, 9))
    with pytest.raises(RuntimeError, match=r'DeviceBuffer records need shape = \(E, T\)'):
        horizon_error(Model(), Fake(8 * 2 * 9 * 60), Fake(8 * 2 * 9 * 4), 3)
    with pytest.raises(RuntimeError, match='the DeviceBuffers are smaller than'):
        horizon_error(Model(), Fake(8 * 2 * 9 * 60 - 8), Fake(8 * 2 * 9 * 4), 3, shape=(2, 9))
    with pytest.raises(RuntimeError, match=r'X must have shape \(E, T, n_x\) or \(T, n_x\) with n_x = 60'):
        horizon_error(Model(), np.zeros((2, 9, 58)), U, 3)
    m = Model()
    m.fit_Ts = None
    with pytest.raises(RuntimeError, match='the model carries no fit_Ts; give dt'):
        horizon_error(m, X, U, 3)


def test_the_c_entry_points_refuse_before_any_device_call():
    from sofacontrol_amd.tpwl import sysid
    lib = sysid._bind()
    w, b = C.c_int64(-7), C.c_int(-7)
    args = lambda r=30, m=4, H=50, T=1001, stride=1, every=10: [r, m, 64, 3, 0.0, 4, T, H, stride, every]
    for kw, word in ((dict(r=65), b'n_x = 130 exceeds the limit n_x <= 128'), (dict(r=0), b'r = 0, need r >= 1'), (dict(H=1025), b'H = 1025'),
                     (dict(H=0), b'H = 0'), (dict(m=0), b'm = 0'), (dict(T=50), b'W = 0 windows'), (dict(stride=0), b'stride = 0'),
                     (dict(every=0), b'every = 0')):
        assert lib.stpwl_horizon_plan(*args(**kw), C.byref(w), C.byref(b), None, None, None, None, None) == -1, kw
        assert b'stpwl_horizon_plan:' in lib.srh_last_error() and word in lib.srh_last_error(), (kw, lib.srh_last_error())
        assert w.value == 0 and b.value == 0
    assert lib.stpwl_horizon_plan(*args(), None, None, None, None, None, None, None) == 0           # every output may be NULL
    X = np.zeros(8)
    xp = X.ctypes.data_as(C.POINTER(C.c_double))
    cnt = (C.c_int64 * 3)()
    tail = [2, 9, 3, 1, 1, None, None, None, cnt, None, None, None]
    assert lib.stpwl_horizon_error(None, xp, xp, *tail) == -1 and b'stpwl_horizon_error: null handle' in lib.srh_last_error()
    assert lib.stpwl_horizon_error_dev(None, C.cast(xp, C.c_void_p), C.cast(xp, C.c_void_p), *tail, None) == -1
    assert b'stpwl_horizon_error_dev: null handle' in lib.srh_last_error()
