"""GPU: the batched filter (sekf_batch_*, tpwl.observer.DiscreteEKFObserverBatch) -- the three filter kernels of csrc/observer.hip
launched with one workgroup per filter -- on the seeded members of tests/ekf_batch_cases.py, one shape per kernel path.

  - member against one-filter handle: member b of a batch equals, bit for bit in x and Sigma after every call of the schedule (fused,
    predict-only, update-only), a DiscreteEKFObserver driven by member b's numbers.  B = 3: every member; B = 260 (more workgroups than
    CUs): members 0, 1, 255, 256, 259;
  - against long double: every member of the B = 3 batches within ekf_cases.tolerance(e_oracle of that member), x and Sigma, and
    takes the table point the reference takes at every predictor;
  - failure isolation: one member with a covariance whose innovation covariance loses its last pivot reports status 1 and keeps its x
    and Sigma bit for bit, sekf_batch_step returns the numeric error, the other members equal the same batch with a healthy covariance
    in that slot bit for bit;
  - refusals, each with a message naming the limit.
Every figure is printed before it is asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import ekf_batch_cases as bc
import ekf_cases as ec

pytestmark = pytest.mark.gpu

NOT_PD = 'innovation covariance S is not positive definite'
SHAPE_IDS = ['%s-%dx%d-m%d' % s for s in bc.SHAPES]


def make_batch(c, tp, batch):
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    return DiscreteEKFObserverBatch(tp, batch, Sigma0=c['Sigma0'], W=c['W'], V=c['V'])


def batch_state(obs):
    """(x, Sigma) read from the device; the estimate a step hands back is the resident one."""
    from sofacontrol_amd import _lib
    x, S = np.empty((obs.batch, obs.state_dim)), np.empty((obs.batch, obs.state_dim, obs.state_dim))
    _lib.check(_lib.lib().sekf_batch_get_state(obs._h, _lib.dptr(x), _lib.dptr(S), None), 'sekf_batch_get_state')
    if obs.x is not None:
        np.testing.assert_array_equal(x, obs.x)
    return x, S


def apply(obs, op):
    if op[0] == 'reset':
        obs.initialize(op[2])
    elif op[2] is not None and op[3] is not None:
        obs.update(op[2], op[3], ec.DT)
    elif op[2] is not None:
        obs.predict_state(op[2], ec.DT)
    else:
        obs.update_state(op[3])


def run_batch(obs, ops, points=None):
    """States (x (B x n), Sigma (B x n x n)) after every compute call; points: a list that receives obs.points after every predictor."""
    out = []
    for op in ops:
        apply(obs, op)
        if op[0] == 'step':
            out.append(batch_state(obs))
            if points is not None and op[2] is not None:
                points.append(obs.points)
    return out


class SingleFilter:
    """One DiscreteEKFObserver on the same model object, with the set_x / step / state interface of ekf_cases.run."""

    def __init__(self, c, tp):
        from sofacontrol_amd import _lib
        from sofacontrol_amd.tpwl.observer import DiscreteEKFObserver
        self.lib, self.n = _lib, c['n']
        self.ekf = DiscreteEKFObserver(tp, Sigma0=c['Sigma0'], W=c['W'], V=c['V'])

    def set_x(self, x):
        x = self.lib.f64(x)
        self.lib.check(self.lib.lib().sekf_set_state(self.ekf._h, self.lib.dptr(x), None), 'sekf_set_state')
        self.ekf.x = x.copy()

    def step(self, u, y, explicit):
        assert explicit is None
        if u is not None and y is not None:
            self.ekf.update(u, y, ec.DT)
        elif u is not None:
            self.ekf.predict_state(u, ec.DT)
        else:
            self.ekf.update_state(y)

    def state(self):
        x, S = np.empty(self.n), np.empty((self.n, self.n))
        self.lib.check(self.lib.lib().sekf_get_state(self.ekf._h, self.lib.dptr(x), self.lib.dptr(S)), 'sekf_get_state')
        return x, S


def check_plan(obs, shape, batch):
    from sofacontrol_amd import _lib
    got, want = obs.kernel_plan(), _lib.ekf_plan(shape[1], shape[2])
    assert got['path'] == want['path'] == ec.PATH_CODE[shape[0]], (shape, got, want)
    assert got['gain_form'] == want['gain_form'] and got['batch'] == batch and 0 < got['lds_bytes'] <= want['lds_bytes']


@pytest.mark.parametrize('batch,members', [(bc.SMALL, tuple(range(bc.SMALL))), (bc.LARGE, bc.LARGE_MEMBERS)], ids=['B3', 'B260'])
@pytest.mark.parametrize('shape', bc.SHAPES, ids=SHAPE_IDS)
def test_member_equals_one_filter_handle(shape, batch, members, monkeypatch):
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    c = ec.case(ec.spec(shape))
    tp, _ = ec.product_filter(c)
    obs = make_batch(c, tp, batch)
    check_plan(obs, shape, batch)
    got = run_batch(obs, bc.batch_operations(shape, range(batch)))
    check_plan(obs, shape, batch)                                  # the first predictor re-creates the filters on the dt handle
    assert (obs.status == 0).all()
    for b in members:
        cm = bc.member(shape, b)
        single = SingleFilter(cm, tp)
        want = ec.run(cm, single)
        assert single.ekf.kernel_plan()['path'] == ec.PATH_CODE[shape[0]]
        assert len(want) == len(got) == len(ec.call_steps(cm))
        for call, ((xb, Sb), (x1, S1)) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(xb[b], x1, err_msg='x of member %d after call %d' % (b, call))
            np.testing.assert_array_equal(Sb[b], S1, err_msg='Sigma of member %d after call %d' % (b, call))
    print('ekf_batch %s B = %d: members %s equal their one-filter handles over %d calls' % (shape, batch, list(members), len(got)))


@pytest.mark.parametrize('shape', bc.SHAPES, ids=SHAPE_IDS)
def test_members_against_long_double(shape, monkeypatch):
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    c = ec.case(ec.spec(shape))
    tp, _ = ec.product_filter(c)
    obs = make_batch(c, tp, bc.SMALL)
    assert obs.points.tolist() == [-1] * bc.SMALL
    points = []
    got = run_batch(obs, bc.batch_operations(shape, range(bc.SMALL)), points)
    for b in range(bc.SMALL):
        ref, flt, e_oracle = bc.reference(shape, b)
        assert [int(p[b]) for p in points] == flt.picks, (shape, b)           # each filter selects its region at its own estimate
        tol = ec.tolerance(e_oracle)
        errs = ec.errors([(x[b], S[b]) for x, S in got], ref)
        ex, eS = max(e[0] for e in errs), max(e[1] for e in errs)
        print('ekf_batch %s member %d: worst err x %.2e Sigma %.2e over %d calls, points %s | e_oracle %.2e tol %.2e'
              % (shape, b, ex, eS, len(errs), sorted(set(flt.picks)), e_oracle, tol))
        bad = [(k, e) for k, e in zip(ec.call_steps(c), errs) if max(e) > tol]
        assert not bad, (shape, b, tol, bad[:4])


@pytest.mark.parametrize('shape', bc.SHAPES, ids=SHAPE_IDS)
def test_failure_stays_in_its_filter(shape, monkeypatch):
    """A numerical status, not a device fault: the kernel finds a non-positive pivot and leaves through its failure exit."""
    from sofacontrol_amd import _lib
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    c = ec.case(ec.spec(shape))
    tp, _ = ec.product_filter(c)
    B, f = bc.SMALL, bc.FAILING
    ops = bc.batch_operations(shape, range(B))
    reset, fused = ops[0], ops[1]
    assert reset[0] == 'reset' and fused[0] == 'step' and fused[2] is not None and fused[3] is not None
    (name, bad_sigma, pivot), = [t for t in ec.indefinite_sigmas(c) if t[0] == 'last_pivot']
    assert pivot == c['ny'] - 1

    healthy = make_batch(c, tp, B)
    apply(healthy, reset)
    healthy.update_state(fused[3])
    hx, hS = batch_state(healthy)
    healthy.update_state(fused[3])
    hx2, hS2 = batch_state(healthy)

    obs = make_batch(c, tp, B)
    apply(obs, reset)
    Sig = np.repeat(c['Sigma0'][None], B, axis=0)
    Sig[f] = bad_sigma
    obs.Sigma = Sig
    x_out = np.empty((B, c['n']))
    y = _lib.f64(fused[3])
    rc = _lib.lib().sekf_batch_step(obs._h, None, _lib.dptr(y), _lib.dptr(x_out))        # update-only: S is formed from the installed Sigma
    msg = _lib.lib().srh_last_error().decode()
    print('ekf_batch %s failure isolation: rc %d, status %s, message %r' % (shape, rc, obs.status.tolist(), msg))
    assert rc == -4 and NOT_PD in msg and '1 of %d filters (first: filter %d)' % (B, f) in msg
    assert obs.status.tolist() == [1 if b == f else 0 for b in range(B)]
    x, S = np.empty((B, c['n'])), np.empty((B, c['n'], c['n']))
    _lib.check(_lib.lib().sekf_batch_get_state(obs._h, _lib.dptr(x), _lib.dptr(S), None), 'sekf_batch_get_state')
    np.testing.assert_array_equal(x, x_out)
    np.testing.assert_array_equal(x[f], reset[2][f])
    np.testing.assert_array_equal(S[f], bad_sigma)
    others = [b for b in range(B) if b != f]
    np.testing.assert_array_equal(x[others], hx[others])
    np.testing.assert_array_equal(S[others], hS[others])
    # the Python call raises as the single observer does, with x refreshed; the other members have taken their second update
    with pytest.raises(RuntimeError, match=NOT_PD):
        obs.update_state(fused[3])
    assert obs.status.tolist() == [1 if b == f else 0 for b in range(B)]
    x, S = batch_state(obs)
    np.testing.assert_array_equal(x[f], reset[2][f])
    np.testing.assert_array_equal(S[f], bad_sigma)
    np.testing.assert_array_equal(x[others], hx2[others])
    np.testing.assert_array_equal(S[others], hS2[others])
    # a healthy covariance back in the slot: the member steps again and its status clears
    Sig[f] = c['Sigma0']
    obs.Sigma = Sig
    apply(obs, fused)
    assert (obs.status == 0).all()


def test_refusals():
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch
    shape = bc.SHAPES[0]
    c = ec.case(ec.spec(shape))
    tp, _ = ec.product_filter(c)
    kw = dict(Sigma0=c['Sigma0'], W=c['W'], V=c['V'])
    with pytest.raises(RuntimeError, match='batch must be an integer >= 1'):
        DiscreteEKFObserverBatch(tp, 0, **kw)
    method = tp.tpwl_method
    try:
        tp.tpwl_method = 'weighting'
        with pytest.raises(RuntimeError, match='weighting-mode models .* are not batched'):
            DiscreteEKFObserverBatch(tp, 2, **kw)
    finally:
        tp.tpwl_method = method
    with pytest.raises(RuntimeError, match=r'Sigma0 must have shape \(8, 8\)'):
        DiscreteEKFObserverBatch(tp, 2, Sigma0=np.eye(7), W=c['W'], V=c['V'])
    obs = DiscreteEKFObserverBatch(tp, 2, **kw)
    with pytest.raises(RuntimeError, match=r'x must have shape \(2, 8\)'):
        obs.initialize(np.zeros(8))
    with pytest.raises(RuntimeError, match=r'u must have shape \(2, 4\)'):
        obs.update(np.zeros((3, 4)), np.zeros((2, 6)), ec.DT)
    with pytest.raises(RuntimeError, match=r'y must have shape \(2, 6\)'):
        obs.update_state(np.zeros((2, 5)))
    with pytest.raises(RuntimeError, match=r'Sigma must have shape \(2, 8, 8\)'):
        obs.Sigma = np.eye(8)
    # the C ABI: batch < 1, a shape ekf_plan refuses (n_x = 128: past the 160 KB LDS), null arguments, a model without discrete tables
    lib, h = _lib.lib(), C.c_void_p()
    mh = tp.handle_for(ec.DT)
    args = (_lib.dptr(_lib.f64(c['C'])), None, C.c_int(c['ny']), _lib.dptr(c['Sigma0']), _lib.dptr(c['W']), _lib.dptr(c['V']))
    assert lib.sekf_batch_create(C.byref(h), mh, *args, C.c_int64(0)) == -1 and b'need batch >= 1' in lib.srh_last_error()
    assert lib.sekf_batch_create(C.byref(h), mh, *args[:2], C.c_int(9), *args[3:], C.c_int64(2)) == -1 and b'n_y <= n_x' in lib.srh_last_error()
    assert lib.sekf_batch_step(None, None, None, None) == -1 and b'null argument' in lib.srh_last_error()
    assert lib.sekf_batch_step(obs._h, None, None, None) == -1 and b'need inputs' in lib.srh_last_error()
    assert _lib.ekf_plan(128, 30)['path'] == 0
    from helpers import small_rom, tip_selector, product_tpwl
    from oracle import tpwl as otpwl
    tpb = product_tpwl(otpwl.synthetic_model(64, 4, 2, seed=3), *small_rom(70, 64, 3), tip_selector(15, 70))
    tpb.C, tpb.y_ref, tpb.meas_dim = np.eye(30, 128), np.zeros(30), 30
    with pytest.raises(RuntimeError, match='no filter kernel takes n_x = 128, n_y = 30'):
        DiscreteEKFObserverBatch(tpb, 2)
    bargs = (_lib.dptr(_lib.f64(tpb.C)), None, C.c_int(30), _lib.dptr(np.eye(128)), _lib.dptr(np.eye(128)), _lib.dptr(np.eye(30)))
    assert lib.sekf_batch_create(C.byref(h), tpb.handle_for(None), *bargs, C.c_int64(2)) == -1 and b'does not fit the 160 KB LDS' in lib.srh_last_error()
    # a predictor on the continuous handle (no discrete tables)
    cont = C.c_void_p()
    _lib.check(lib.sekf_batch_create(C.byref(cont), tp.handle_for(None), *args, C.c_int64(2)), 'sekf_batch_create')
    try:
        u = np.zeros((2, 4))
        assert lib.sekf_batch_step(cont, _lib.dptr(u), None, None) == -1 and b'has not been pre-discretised' in lib.srh_last_error()
    finally:
        lib.sekf_batch_destroy(cont)
