"""ctypes binding of libsofacontrol_hip.so (C ABI: include/sofacontrol_hip.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRH_LIB_PATH: another build of the same library (e.g. a -DSRH_PROFILE build for tools/probes/*); default = the in-tree one
LIB_PATH = os.environ.get('SRH_LIB_PATH') or os.path.join(_HERE, 'libsofacontrol_hip.so')

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class HipError(RuntimeError):
    pass


class SLocpProblem(C.Structure):
    _fields_ = [('N', C.c_int), ('n_x', C.c_int), ('n_u', C.c_int), ('n_z', C.c_int),
                ('H', c_double_p), ('Qz', c_double_p), ('R', c_double_p), ('Qzf', c_double_p),
                ('x_scale', c_double_p),
                ('nU', C.c_int), ('UA', c_double_p), ('Ub', c_double_p),
                ('nX', C.c_int), ('XA', c_double_p), ('Xb', c_double_p),
                ('nXf', C.c_int), ('XfA', c_double_p), ('Xfb', c_double_p),
                ('ndU', C.c_int), ('dUA', c_double_p), ('dUb', c_double_p),
                ('tr_active', C.c_int)]


class SGustoParams(C.Structure):
    _fields_ = [('delta0', C.c_double), ('omega0', C.c_double), ('rho', C.c_double),
                ('beta_fail', C.c_double), ('gamma_fail', C.c_double), ('epsilon', C.c_double),
                ('omega_max', C.c_double), ('convg_thresh', C.c_double), ('max_gusto_iters', C.c_int)]


class SrhKernelInfo(C.Structure):
    """include/sofacontrol_hip.h: srh_kernel_info -- which kernels a LOCP / GuSTO plan launches."""
    _fields_ = [('family', C.c_int32), ('lean_args', C.c_int32 * 6), ('fused_args', C.c_int32 * 3),
                ('handed_over', C.c_int32), ('lds_bytes_lean', C.c_int32), ('lds_bytes_fused', C.c_int32),
                ('threads', C.c_int32)]

    def as_dict(self):
        """{'family': 'lean' | 'fused', 'kernel': the name rocprof shows, 'lean': (n_u, n_x, GX, N, j0, state rows) | None,
        'fused': (split, n_u, n_x), 'handed_over': problems of the last solve the lean kernel passed on (-1: none yet)}."""
        lean = tuple(int(v) for v in self.lean_args) if self.family == 1 else None
        fused = (bool(self.fused_args[0]), int(self.fused_args[1]), int(self.fused_args[2]))
        kern = ('lean<%d, %d, %d, %d, %d, %d>' % lean) if lean else ('fused<%s, %d, %d>' % (str(fused[0]).lower(), fused[1], fused[2]))
        return {'family': 'lean' if self.family == 1 else 'fused', 'kernel': kern, 'lean': lean, 'fused': fused,
                'handed_over': int(self.handed_over), 'lds_bytes_lean': int(self.lds_bytes_lean),
                'lds_bytes_fused': int(self.lds_bytes_fused), 'threads': int(self.threads)}


class SIlqrParams(C.Structure):
    _fields_ = [('max_iter', C.c_int), ('epsilon', C.c_double), ('alpha0', C.c_double),
                ('alpha_scaling', C.c_double), ('improv_lb', C.c_double), ('improv_ub', C.c_double),
                ('alpha_min', C.c_double), ('counter_limit', C.c_int), ('rho0', C.c_double),
                ('drho0', C.c_double), ('rho_scaling', C.c_double), ('rho_increase_fp', C.c_double),
                ('rho_max', C.c_double), ('rho_min', C.c_double), ('include_input_var_constraint', C.c_int),
                ('do_linesearch', C.c_int), ('regularize', C.c_int), ('state_regularization', C.c_int)]


_lib = None


def lib():
    """Load the shared library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise HipError('libsofacontrol_hip.so is missing (%s): run `python -c "import '
                           '__graft_entry__ as g; g.build()"` or `make -C soft-robot-control_amd/csrc`; '
                           'there is no CPU fallback' % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.srh_last_error.restype = C.c_char_p
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().srh_last_error().decode(errors='replace')
        if rc == -1:
            raise RuntimeError('%s: %s' % (what, msg))   # the reference raises RuntimeError on bad args
        raise HipError('%s failed (code %d): %s' % (what, rc, msg))


def dptr(a):
    """double* of a C-contiguous float64 array (or NULL for None)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(c_int32_p)


def f64(a):
    """C-contiguous float64 copy/view of a (None passes through)."""
    if a is None:
        return None
    return np.ascontiguousarray(a, dtype=np.float64)


def device_count():
    n = C.c_int(0)
    rc = lib().srh_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def set_device(i):
    check(lib().srh_set_device(C.c_int(i)), 'srh_set_device')


class DeviceBuffer:
    """A raw HBM allocation made through the C ABI (for callers that want resident inputs)."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib().srh_malloc(C.byref(self.ptr), C.c_size_t(self.nbytes)), 'srh_malloc')

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(lib().srh_memcpy_h2d(b.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)), 'h2d')
        return b

    def to_array(self, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib().srh_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes)), 'd2h')
        return out

    def free(self):
        if self.ptr:
            lib().srh_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sync():
    check(lib().srh_sync(), 'srh_sync')


def gusto_rule_replay(params, N, n_x, script):
    """sgusto_rule_replay: GuSTO's step rule as the kernels run it (csrc/scp_types.h), replayed on the host -- no GPU needed.
    params: dict with SGustoParams' field names; script (T x 5): the QP answers (md, J, rho_k, viol, dsum).  Returns
    (steps (iters x 4): delta, omega of the QP, accepted, J_prev after the step; iters, status, converged)."""
    par = SGustoParams(**params)
    script = np.ascontiguousarray(script, dtype=np.float64).reshape(-1, 5)
    steps = np.zeros((script.shape[0], 4))
    iters, status, converged = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(lib().sgusto_rule_replay(C.byref(par), C.c_int(N), C.c_int(n_x), C.c_int(script.shape[0]), dptr(script), dptr(steps),
                                   C.byref(iters), C.byref(status), C.byref(converged)), 'sgusto_rule_replay')
    return steps[:iters.value], iters.value, status.value, bool(converged.value)


EKF_PATHS = ('refused', 'valu', 'mfma_generic', 'mfma_60', 'wide')


def _ekf_plan_dict(path, lds, gain):
    return {'path': path.value, 'kernel': EKF_PATHS[path.value], 'lds_bytes': int(lds.value), 'gain_form': gain.value}


def ekf_plan(n_x, n_y):
    """sekf_plan: the kernel sekf_create chooses for a filter of n_x states and n_y measurements (csrc/observer.hip), on the host --
    no GPU needed.  {'path': 0 refused | 1 VALU | 2 MFMA generic | 3 MFMA <60> | 4 wide, 'kernel': its name, 'lds_bytes',
    'gain_form': 0 Gauss-Jordan on all waves (paths 2 to 4) | 1 one-wave Cholesky (path 1)}.  Honours SRH_EKF_NO_MFMA."""
    path, lds, gain = C.c_int(0), C.c_size_t(0), C.c_int(0)
    check(lib().sekf_plan(C.c_int(n_x), C.c_int(n_y), C.byref(path), C.byref(lds), C.byref(gain)), 'sekf_plan')
    return _ekf_plan_dict(path, lds, gain)


def ekf_handle_plan(h):
    """sekf_handle_plan: the same for a live filter handle (what sekf_create decided, with the model's own n_u)."""
    path, lds, gain = C.c_int(0), C.c_size_t(0), C.c_int(0)
    check(lib().sekf_handle_plan(h, C.byref(path), C.byref(lds), C.byref(gain)), 'sekf_handle_plan')
    return _ekf_plan_dict(path, lds, gain)


def tpwl_rollout_plan(h, N, batch):
    """stpwl_rollout_plan: the kernel a rollout of the TPWL handle h launches (csrc/tpwl.hip), on the host.  {'staged': region panel in
    LDS | plain kernel, 'held': point table in registers | general nearest-point search, 'lds_bytes'}.  A handle created under
    SRH_TPWL_ROLLOUT_PLAIN=1 stays plain."""
    staged, held, lds = C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(lib().stpwl_rollout_plan(h, C.c_int(N), C.c_int64(batch), C.byref(staged), C.byref(held), C.byref(lds)), 'stpwl_rollout_plan')
    return {'staged': bool(staged.value), 'held': bool(held.value), 'lds_bytes': int(lds.value)}


def gramian_plan(n_s, n_f, cus=0):
    """srom_gramian_plan: the launch srom_gramian_dev makes for an n_s x n_f snapshot matrix (csrc/gramian.hip) on a card of `cus`
    compute units -- cus = 0 asks the current device, cus > 0 is answered on the host, no GPU needed.  {'ntile': 128-row tiles per
    side, 'nfull': tiles computed whole, 'ntail': tiles of the partial last round split along K, 'ksplit': parts per such tile}."""
    ntile, nfull, ntail, ksplit = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().srom_gramian_plan(C.c_int64(n_s), C.c_int64(n_f), C.c_int(cus), C.byref(ntile), C.byref(nfull), C.byref(ntail),
                                  C.byref(ksplit)), 'srom_gramian_plan')
    return {'ntile': ntile.value, 'nfull': nfull.value, 'ntail': ntail.value, 'ksplit': ksplit.value}


IPM_PHASES = ('init', 'cold', 'warm', 'pred', 'corr', 'direction', 'affine', 'advance', 'scales', 'verdict', 'converged')


def ipm_rule_replay(phase, rows, par):
    """sqp_ipm_rule_replay: the interior point's row rule as the seven QP kernels run it (csrc/ipm_rule.h), evaluated on the host -- no
    GPU needed.  phase: a name of IPM_PHASES; rows (n x 8): g, t, lambda, rg, rc, dt, dlambda, a.d (the verdict's script: ok, mu, rd, rp,
    iteration, row count); par: up to 8 numbers (include/sofacontrol_hip.h lists both per phase).  Returns (out (n x 8), scal (8))."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 8)
    p8 = np.zeros(8)
    p8[:len(par)] = par
    out, scal = np.zeros((rows.shape[0], 8)), np.zeros(8)
    check(lib().sqp_ipm_rule_replay(C.c_int(IPM_PHASES.index(phase)), C.c_int(rows.shape[0]), dptr(rows), dptr(p8), dptr(out), dptr(scal)),
          'sqp_ipm_rule_replay')
    return out, scal


ROSTER_EVENTS = ('wait', 'signal', 'read', 'chol', 'panel', 'update', 'front')
ROSTER_COUNTERS = ('trail', 'rinv', 'panel', 'next')


def lean_roster_replay(KT, code, nwk0=1):
    """slean_roster_replay: the tile factorisation of the lean kernels' wave set as each of its four waves runs it under row roster
    `code` (csrc/locp_lean.h: roster_nwk and the targets next to it), listed on the host -- no GPU needed.  Returns (code in effect,
    [events of wave 0, .., of wave 3]); an event is (kind, a, b, c) with kind a name of ROSTER_EVENTS (include/sofacontrol_hip.h)."""
    waves, eff = [], C.c_int32(0)
    for wave in range(4):
        n = C.c_int32(0)
        check(lib().slean_roster_replay(C.c_int(KT), C.c_int(code), C.c_int(nwk0), C.c_int(wave), C.c_int(0),
                                        np.zeros(4, dtype=np.int32).ctypes.data_as(C.c_void_p), C.byref(n), C.byref(eff)), 'slean_roster_replay')
        ev = np.zeros((max(1, n.value), 4), dtype=np.int32)
        check(lib().slean_roster_replay(C.c_int(KT), C.c_int(code), C.c_int(nwk0), C.c_int(wave), C.c_int(n.value),
                                        ev.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(eff)), 'slean_roster_replay')
        waves.append([(ROSTER_EVENTS[k], int(a), int(b), int(c)) for k, a, b, c in ev[:n.value]])
    return int(eff.value), waves


GU_SPARE, GU_STORES = 1, 2


def lean_gu_schedule(NF, M, set_size):
    """slean_gu_schedule: y = G u of the half-size lean kernel by (column, chain) tasks (csrc/locp_lean.h: gu_rounds and the functions
    next to it), listed on the host -- no GPU needed.  Returns {(wave, lane): int32 array (steps x 9)} for the set's waves, a row being
    (round, input, step, column, chain, stage or -1, flags, packed index, toeplitz index) (include/sofacontrol_hip.h)."""
    out = {}
    for wave in range(set_size // 64):
        for lane in range(64):
            n = C.c_int32(0)
            args = (C.c_int(NF), C.c_int(M), C.c_int(set_size), C.c_int(wave), C.c_int(lane))
            check(lib().slean_gu_schedule(*args, C.c_int(0), np.zeros(9, dtype=np.int32).ctypes.data_as(C.c_void_p), C.byref(n)),
                  'slean_gu_schedule')
            st = np.zeros((max(1, n.value), 9), dtype=np.int32)
            check(lib().slean_gu_schedule(*args, C.c_int(n.value), st.ctypes.data_as(C.c_void_p), C.byref(n)), 'slean_gu_schedule')
            out[(wave, lane)] = st[:n.value]
    return out


def gusto_plan_dims(plan):
    """sgusto_plan_dims: the shapes a resident GuSTO plan was created with, {'N', 'n_x', 'n_u', 'n_z', 'batch', 'dt', 'has_Qzf'}."""
    N, n, m, nz, hq = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    B, dt = C.c_int64(0), C.c_double(0.0)
    check(lib().sgusto_plan_dims(plan, C.byref(N), C.byref(n), C.byref(m), C.byref(nz), C.byref(B), C.byref(dt), C.byref(hq)),
          'sgusto_plan_dims')
    return {'N': N.value, 'n_x': n.value, 'n_u': m.value, 'n_z': nz.value, 'batch': B.value, 'dt': dt.value, 'has_Qzf': bool(hq.value)}


def gusto_loop_schedule(N, dt, dt_sim, n_keep, t_start, k):
    """sgusto_loop_schedule: the schedule of period k of a batched closed loop as the library computes it (csrc/gusto_loop.hip), on the
    host -- no GPU needed.  Returns (t_k, idx0, j (n_keep, int32), theta (n_keep)); scp.closed_loop.schedule is the numpy statement."""
    t_k, idx0 = C.c_double(0.0), C.c_int(0)
    j, theta = np.zeros(n_keep, dtype=np.int32), np.zeros(n_keep)
    check(lib().sgusto_loop_schedule(C.c_int(N), C.c_double(dt), C.c_double(dt_sim), C.c_int(n_keep), C.c_double(t_start), C.c_int64(k),
                                     C.byref(t_k), C.byref(idx0), iptr(j), dptr(theta)), 'sgusto_loop_schedule')
    return t_k.value, idx0.value, j, theta


def gusto_loop_end_row(N, dt, dt_sim, n_keep):
    """sgusto_loop_end_row: the end row (j_end, theta_end) of a period's schedule as the library computes it, on the host -- no GPU
    needed; scp.closed_loop.schedule_end is the numpy statement."""
    j, theta = C.c_int32(0), C.c_double(0.0)
    check(lib().sgusto_loop_end_row(C.c_int(N), C.c_double(dt), C.c_double(dt_sim), C.c_int(n_keep), C.byref(j), C.byref(theta)),
          'sgusto_loop_end_row')
    return j.value, theta.value
