"""GPU: koop_lift_kernel (csrc/koopman.hip) in its three zeta modes, with and without W, and its launcher's tile and LDS bookkeeping
(koop_prepare_launch), case by case against tests/koopman_lift_reference.py.

  KoopmanLift.lift_dev         KP_ZETA    ready-made zeta rows
  KoopmanLift.embed_lift_dev   KP_RECORD  raw record, delay embedding and scale_down in the kernel
  KoopmanLift.ring_lift_dev    KP_RING    the per-member device ring filled by push

Without W the device must equal the float64 restatement bit for bit (np.array_equal: an observable is a fixed-order product).  With W:
integer data bit for bit (every partial sum is an integer below 2^20), real data inside w_bound = (P + 4 + degree) 2^-53 |psi| |W|^T
against long double, elementwise.  Every output sits between sentinel guards, every input inside a NaN-filled buffer.  The largest
fraction of w_bound met per mode and tile class is printed (profiles/koopman_lift_exact.log) and not asserted beyond <= 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_lift_cases as kc
import koopman_lift_reference as kr
from test_pod_build_exact_gpu import Guarded, SENTINEL, _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 96                     # NaN doubles on either side of an input
FRACTIONS = {}               # (mode, TR) -> largest |err| / w_bound met


class Padded:
    """A device copy of `a` with PAD NaN doubles before and after it: a read outside the array shows in the output."""

    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        self.buf = _dev(np.concatenate((np.full(PAD, np.nan), a, np.full(PAD, np.nan))))
        self.ptr = C.c_void_p(self.buf.ptr.value + 8 * PAD)


def _lift_handle(name, W=None, batch=1):
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanLift
    c = kc.case(name)
    return KoopmanLift.for_zeta(c['nz'], c['degree'], DMD=c['dmd'], W=W, batch=batch)


def _lift(h, Z):
    from sofacontrol_amd import _lib
    rows = Z.shape[0]
    dz, out = Padded(Z), Guarded(rows * h.n_out)
    h.lift_dev(dz.ptr, rows, out.ptr)
    _lib.sync()
    return out.get((rows, h.n_out))


def _note(mode, TR, frac):
    FRACTIONS[(mode, TR)] = max(FRACTIONS.get((mode, TR), 0.0), frac)


def _check_w(got, ref, bound, kind, mode, TR, what):
    """Integer data: bits.  Real data: elementwise inside the bound; the fraction met is printed and noted."""
    if kind == 'int':
        assert kr.same_bits(got, ref), what
        return
    frac = kr.bound_fraction(got, ref, bound)
    print('%s: |err| / w_bound at most %.4f' % (what, frac))
    _note(mode, TR, frac)
    assert kr.inside(got, ref, bound), (what, frac)


# ------------------------------------------------------------------------------------------------------------- 1. zeta mode, no W
@pytest.mark.parametrize('kind', kc.KINDS)
@pytest.mark.parametrize('name', list(kc.LIFT_CASES))
def test_zeta_mode_psi_bit_exact(name, kind):
    from sofacontrol_amd.baselines.koopman.koopman_utils import num_observables, observable_exponents
    c = kc.case(name)
    h = _lift_handle(name)
    assert (h.nzeta, h.n_psi, h.n_out, h.has_w) == (c['nz'], c['P'], c['P'], False)
    assert num_observables(c['nz'], c['degree'], c['dmd']) == c['P']
    assert np.array_equal(observable_exponents(c['nz'], c['degree'], c['dmd']), kc.exps(c['nz'], c['degree'], c['dmd']))
    Z, ref = kc.zeta(name, kind), kc.psi_of(name, kind, False)
    for rows in kc.rows_of(name):
        got = _lift(h, Z[:rows])
        assert kr.same_bits(got, ref[:rows]), (name, kind, rows, np.argwhere(got != ref[:rows])[:4])


# ---------------------------------------------------------------------------------------------------------------- 2. zeta mode, W
@pytest.mark.parametrize('kind', kc.KINDS)
@pytest.mark.parametrize('name,Nw', [(n, Nw) for n in kc.W_CASES for Nw in kc.nw_of(n)])
def test_zeta_mode_w_exact_or_inside_bound(name, Nw, kind):
    c = kc.case(name)
    h = _lift_handle(name, W=kc.w_of(name, Nw, kind))
    assert (h.n_psi, h.n_out, h.has_w) == (c['P'], Nw, True)
    ref, bound = kc.w_reference(name, Nw, kind)
    Z = kc.zeta(name, kind)
    for rows in kc.w_rows_of(name):
        got = _lift(h, Z[:rows])
        _check_w(got, ref[:rows], None if bound is None else bound[:rows], kind, 'zeta', c['TR'],
                 '%s Nw=%d rows=%d %s' % (name, Nw, rows, kind))


@pytest.mark.parametrize('name', kc.W_CASES)
def test_identity_w_is_not_applied(name):
    c = kc.case(name)
    h, h0 = _lift_handle(name, W=np.eye(c['P'])), _lift_handle(name)
    assert not h.has_w and h.n_out == c['P']
    Z = kc.zeta(name, 'real')[:c['TR'] + 1]
    got = _lift(h, Z)
    assert kr.same_bits(got, _lift(h0, Z)) and kr.same_bits(got, kc.psi_of(name, 'real', False)[:c['TR'] + 1])
    # one entry off the identity and W is applied
    W = np.eye(c['P'])
    W[c['P'] - 1, 0] = 2.0 ** -40
    assert _lift_handle(name, W=W).has_w


# ------------------------------------------------------------------------------------------------------------------- 3. isolation
@pytest.mark.parametrize('with_w', [False, True])
@pytest.mark.parametrize('TR', sorted(kc.FULL_ROWS))
def test_nan_row_stays_in_its_row_and_calls_repeat(TR, with_w):
    name = kc.FULL_ROWS[TR]
    c = kc.case(name)
    rows, Nw = TR + 1, 17
    h = _lift_handle(name, W=kc.w_of(name, Nw, 'real') if with_w else None)
    Z = kc.zeta(name, 'real')[:rows]
    clean = _lift(h, Z)
    assert kr.same_bits(clean, _lift(h, Z)), 'two identical calls differ'
    if with_w:
        ref, bound = kc.w_reference(name, Nw, 'real')
    for bad in (0, TR - 1, TR):
        Zb = Z.copy()
        Zb[bad] = np.nan
        got = _lift(h, Zb)
        others = np.arange(rows) != bad
        assert kr.same_bits(got[others], clean[others]), (name, bad)
        if with_w:
            assert np.isnan(got[bad]).all()
            _check_w(got[others], ref[:rows][others], bound[:rows][others], 'real', 'zeta', TR, '%s NaN row %d' % (name, bad))
        else:
            ncol = c['P'] - (0 if c['dmd'] else 1)
            assert np.isnan(got[bad, :ncol]).all() and (c['dmd'] or got[bad, -1] == 1.0)
            assert kr.same_bits(got[others], kc.psi_of(name, 'real', False)[:rows][others])


# ----------------------------------------------------------------------------------------------------------------- 4. record mode
def _embed(h, y, u, T, delays):
    """embed_lift_dev of the first T samples; the record sits inside NaN, the output between guards (one row of room when T <= delays)."""
    from sofacontrol_amd import _lib
    rows = max(T - delays, 0)
    dy, du, out = Padded(y[:T]), Padded(u[:T]), Guarded(max(rows, 1) * h.n_out)
    h.embed_lift_dev(dy.ptr, du.ptr, T, out.ptr)
    _lib.sync()
    got = out.get((max(rows, 1), h.n_out))
    if rows == 0:
        assert np.all(got == SENTINEL), 'T <= delays wrote into the output'
    return got[:rows]


@pytest.mark.parametrize('kind', kc.KINDS)
@pytest.mark.parametrize('name', list(kc.RECORD_CASES))
def test_record_mode_exact(name, kind):
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanLift
    d = kc.record_dims(name)
    ny, m, dl, P = d['n_y'], d['m'], d['delays'], d['P']
    sc = kc.scales(ny, m, kind, name)
    lengths = kc.record_lengths(name)
    y, u = kc.samples(lengths[-1], ny, m, dl, kind, sc, name)
    E = kc.exps(d['nz'], d['degree'], d['dmd'])
    Nw = min(17, P)
    W = kc.make_w(Nw, P, kind, 'record ' + name)
    h0 = KoopmanLift(ny, m, dl, d['degree'], DMD=d['dmd'], y_offset=sc[0], y_factor=sc[1], u_offset=sc[2], u_factor=sc[3])
    hw = KoopmanLift(ny, m, dl, d['degree'], DMD=d['dmd'], y_offset=sc[0], y_factor=sc[1], u_offset=sc[2], u_factor=sc[3], W=W)
    assert (h0.nzeta, h0.n_psi, h0.has_w, hw.has_w, hw.n_out) == (d['nz'], P, False, True, Nw)
    Z64 = kr.zeta_record(y, u, dl, sc, np.float64)
    p64 = kr.psi(Z64, E, np.float64)
    if kind == 'int':
        assert np.array_equal(Z64, np.round(Z64)) and np.abs(Z64).max() <= 3
        ref, bound = kr.project(p64, W, np.float64), None
    else:
        # the scaled zeta is the float64 one (the kernel's two operations); from there on long double
        pl = kr.psi(Z64, E, np.longdouble)
        ref, bound = kr.project(pl, W, np.longdouble), kr.w_bound(pl, W, P, d['degree'])
    for T in lengths:
        rows = max(T - dl, 0)
        got = _embed(h0, y, u, T, dl)
        assert kr.same_bits(got, p64[:rows]), (name, kind, T)
        got = _embed(hw, y, u, T, dl)
        _check_w(got, ref[:rows], None if bound is None else bound[:rows], kind, 'record', d['TR'], 'record %s T=%d %s' % (name, T, kind))
    for T in range(dl):                 # every length short of delays + 1, not only T = delays
        assert _embed(h0, y, u, T, dl).shape == (0, P)


# ------------------------------------------------------------------------------------------------------------------- 5. ring mode
def _ring_state(h):
    """(ring (batch, slots, n_y + m), head, count) as the handle holds them."""
    from sofacontrol_amd import _lib
    _lib.sync()
    p, slots, head, count, _ = h.state()
    ring = np.empty((h.batch, slots, h.n_y + h.m))
    _lib.check(_lib.lib().srh_memcpy_d2h(ring.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(ring.nbytes)), 'd2h')
    return ring, head, count


def _ring_lift(h):
    from sofacontrol_amd import _lib
    out = Guarded(h.batch * h.n_out)
    h.ring_lift_dev(out.ptr)
    _lib.sync()
    return out.get((h.batch, h.n_out))


@pytest.mark.parametrize('kind', kc.KINDS)
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('name', list(kc.RING_CASES))
def test_ring_mode_exact(name, wide, kind):
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanLift
    d = kc.ring_dims(name)
    ny, m, dl, P, TR = d['n_y'], d['m'], d['delays'], d['P'], d['TR']
    batch = TR + 1 if wide else 1
    sc = kc.scales(ny, m, kind, name)
    E = kc.exps(d['nz'], d['degree'], d['dmd'])
    Nw = min(17, P)
    W = kc.make_w(Nw, P, kind, 'ring ' + name) if d['with_w'] else None
    h = KoopmanLift(ny, m, dl, d['degree'], DMD=d['dmd'], y_offset=sc[0], y_factor=sc[1], u_offset=sc[2], u_factor=sc[3], W=W, batch=batch)
    assert (h.nzeta, h.n_psi, h.has_w) == (d['nz'], P, d['with_w'])
    npush = 2 * (dl + 1) + 1

    def fresh(tag):
        out = []
        for k in range(npush):
            y, u = kc.samples(batch, ny, m, dl, kind, sc, '%s %s push %d' % (name, tag, k))
            out.append((y, u))
        return out

    def check(pushed, what):
        Z64 = kr.zeta_ring(pushed, dl, sc, np.float64)
        got = _ring_lift(h)
        if W is None:
            assert kr.same_bits(got, kr.psi(Z64, E, np.float64)), what
        elif kind == 'int':
            assert kr.same_bits(got, kr.project(kr.psi(Z64, E, np.float64), W, np.float64)), what
        else:
            pl = kr.psi(Z64, E, np.longdouble)
            _check_w(got, kr.project(pl, W, np.longdouble), kr.w_bound(pl, W, P, d['degree']), kind, 'ring', TR, what)
        assert not np.isnan(got).any()
        # the ring itself: sample t - j, scaled down, in the slot j behind the newest; count and head as pushed
        ring, head, count = _ring_state(h)
        assert count == len(pushed) and ring.shape[1] == dl + 1 and 0 <= head <= dl
        for j in range(min(len(pushed), dl + 1)):
            y, u = pushed[-1 - j]
            want = np.concatenate((kr.scale_down(y, sc[0], sc[1], np.float64), kr.scale_down(u, sc[2], sc[3], np.float64)), axis=1)
            assert kr.same_bits(ring[:, (head - j) % (dl + 1)], want), (what, j)

    pushes, heads = fresh('a'), set()
    for k in range(npush):
        h.push(*pushes[k])
        if k + 1 < dl + 1:
            with pytest.raises(RuntimeError):
                h.ring_lift_dev(Guarded(batch * h.n_out).ptr)
            continue
        check(pushes[:k + 1], '%s batch %d %s push %d' % (name, batch, kind, k + 1))
        heads.add(h.state()[2])
    assert heads == set(range(dl + 1))                    # the newest sample has sat in every slot, and wrapped
    # stale NaN in every slot, reset, refill: refused until the ring is full again, and nothing stale is read then
    nan = (np.full((batch, ny), np.nan), np.full((batch, m), np.nan))
    for _ in range(dl + 1):
        h.push(*nan)
    assert np.isnan(_ring_lift(h)).any()
    h.reset()
    again = fresh('b')[:dl + 1]
    for k in range(dl + 1):
        with pytest.raises(RuntimeError):
            h.ring_lift_dev(Guarded(batch * h.n_out).ptr)
        h.push(*again[k])
    check(again, '%s batch %d %s after reset' % (name, batch, kind))


# -------------------------------------------------------------------------------------------------------------- 6. LDS grant order
GRANT_ORDER = [('shipped', None), ('widest_near_cap', None), ('first_over_64k', None), ('most_observables', None), ('most_observables', 17),
               ('most_observables_dmd', 33), ('shipped', None), ('shipped', 16)]


def grant_order_sequence():
    """Create and launch, in a process that has made no lift handle yet: 40 960 B, the largest request (133 120 B), the first over 64 KiB
    (66 560 B, below what is granted by then), a large W handle after a large W-less one (another `granted` slot), and the small ones
    again.  Each handle is created only when its turn comes, and every lift is compared bit for bit (integer data)."""
    done = 0
    for name, Nw in GRANT_ORDER:
        c = kc.case(name)
        h = _lift_handle(name, W=None if Nw is None else kc.w_of(name, Nw, 'int'))
        rows = c['TR'] + 1
        got = _lift(h, kc.zeta(name, 'int')[:rows])
        ref = kc.psi_of(name, 'int', False)[:rows] if Nw is None else kc.w_reference(name, Nw, 'int')[0][:rows]
        assert kr.same_bits(got, ref), (name, Nw)
        print('grant order: %s (%d B of LDS, %s) bit-exact' % (name, c['lds'], 'W %d x %d' % (Nw, c['P']) if Nw else 'no W'))
        done += 1
    print('grant order: %d lifts bit-exact' % done)


def test_lds_grant_order_in_a_fresh_process():
    assert [kc.case(n)['lds'] for n, _ in GRANT_ORDER[:3]] == [40960, 133120, 66560]
    code = ('import sys; sys.path[:0] = %r; import test_koopman_lift_exact_gpu as t; t.grant_order_sequence()'
            % [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'soft-robot-control_amd'), ROOT])
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'grant order: %d lifts bit-exact' % len(GRANT_ORDER) in r.stdout
    # and in this process, whatever handles the tests before have made: the same sequence
    grant_order_sequence()


# ----------------------------------------------------------------------------------------------------------------------- 7. limits
def test_limits():
    from sofacontrol_amd.baselines.koopman.koopman_utils import KoopmanLift, num_observables, observable_exponents
    for nz, degree in kc.REFUSED:
        assert num_observables(nz, degree) > 1024
        with pytest.raises(RuntimeError):
            KoopmanLift.for_zeta(nz, degree)
        with pytest.raises(RuntimeError):
            KoopmanLift.for_zeta(nz, degree, DMD=True)      # both are over the limit without the constant too
        with pytest.raises(RuntimeError):
            observable_exponents(nz, degree)
    with pytest.raises(RuntimeError):
        KoopmanLift.for_zeta(kr.KP_MAX_NZ + 1, 1)
    with pytest.raises(RuntimeError):
        KoopmanLift.for_zeta(3, kr.KP_MAX_DEG + 1)
    c = kc.case('small_dmd')
    with pytest.raises(RuntimeError):
        KoopmanLift.for_zeta(c['nz'], c['degree'], DMD=True, W=np.ones((c['P'] + 1, c['P'])))
    h = _lift_handle('small_dmd')
    with pytest.raises(RuntimeError):
        h.lift(np.ones((2, c['nz'] + 1)))
    with pytest.raises(RuntimeError):
        h.lift(np.ones((2, c['nz'] - 1)))
    # rows = 0: nothing is launched, nothing written
    from sofacontrol_amd import _lib
    out = Guarded(c['P'])
    h.lift_dev(Padded(np.ones(c['nz'])).ptr, 0, out.ptr)
    _lib.sync()
    assert np.all(out.get((c['P'],)) == SENTINEL)
    assert h.lift(np.zeros((0, c['nz']))).shape == (0, c['P'])


def test_zz_report_fractions():
    """The largest |err| / w_bound met per mode and tile class by the tests above (printed, not asserted beyond <= 1)."""
    for (mode, TR), frac in sorted(FRACTIONS.items()):
        print('worst %-6s TR=%2d: |err| / w_bound = %.4f' % (mode, TR, frac))
        assert frac <= 1.0
