"""GPU: the TPWL point selection (csrc/tpwl_select.hip, tpwl.sysid.points_by_distance) against the long-double sequential scan
(tests/tpwl_select_reference.py) on the cases of tests/tpwl_select_cases.py, every one of which is certified there: ALL comparisons of
its scan are decided, so count, index, status and stopped_at must be equal as integers, q and v must be the record's rows bit for bit,
and dmin must lie within 32 (r + 4) eps relative (+inf exactly).  The chunk of the device's split comes from stpwl_select_plan; the
cases place taken points on both sides of its edges.  Then: streamed records, device records, a rerun, and the hand-over to the fit.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import tpwl_select_cases as sc
import tpwl_select_reference as sr

pytestmark = pytest.mark.gpu


def plan_chunk():
    from sofacontrol_amd.tpwl import sysid
    return sysid.select_plan(2, 1)['chunk']


try:
    C = plan_chunk()
except Exception:                        # collected where the library is not built: the test below reports it
    C = sc.C_DEFAULT
NAMES = sorted(sc.build(C))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def select(c, X=None, q0=None, v0=None, device=None):
    from sofacontrol_amd import _lib
    from sofacontrol_amd.tpwl.sysid import points_by_distance
    X = c['X'] if X is None else X
    kw = dict(separate=c['separate'], stride=c['stride'], q0=c['q0'] if q0 is None else q0, v0=c['v0'] if v0 is None else v0,
              max_points=c['max_points'])
    w = {'q': c['w'][0], 'v': c['w'][1]}
    if device:
        buf = _lib.DeviceBuffer.from_array(X)
        try:
            return points_by_distance(buf, w, c['thr'], shape=X.shape[:device], **kw)
        finally:
            buf.free()
    return points_by_distance(X, w, c['thr'], **kw)


def same_bits(a, b):
    assert np.array_equal(a.index, b.index) and a.complete == b.complete and a.stopped_at == b.stopped_at
    assert np.array_equal(bits(a.q), bits(b.q)) and np.array_equal(bits(a.v), bits(b.v)) and np.array_equal(bits(a.dmin), bits(b.dmin))


def against_reference(sel, ref, c, X=None, what=''):
    X = c['X'] if X is None else X
    r = X.shape[2] // 2
    print('%s: %d points (%d seeded) from %d candidates, complete %s, stopped_at %s; reference %d points, complete %s, stopped_at %s'
          % (what, len(sel.q), sel.seeded, sel.candidates, sel.complete, sel.stopped_at, len(ref['q']), ref['complete'], ref['stopped_at']))
    assert len(sel.q) == len(ref['q']) and sel.candidates == ref['candidates'] and sel.seeded == ref['P0']
    assert sel.index.dtype == np.int64 and np.array_equal(sel.index, ref['index'])
    assert sel.complete == ref['complete'] and sel.stopped_at == ref['stopped_at']
    assert np.array_equal(bits(sel.q), bits(ref['q'])) and np.array_equal(bits(sel.v), bits(ref['v']))
    rows = X[sel.index[:, 0], sel.index[:, 1]]                  # index names UNstrided rows: the points are those rows bit for bit
    assert np.array_equal(bits(sel.q[sel.seeded:]), bits(rows[:, r:])) and np.array_equal(bits(sel.v[sel.seeded:]), bits(rows[:, :r]))
    want, got = ref['dmin'], np.asarray(sel.dmin, dtype=np.longdouble)
    assert got.shape == want.shape
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isnan(got).any()
    fin = np.isfinite(want) & (want != 0)
    share = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]), initial=0.0) / sr.bound(r))
    print('%s: dmin worst share of 32 (r + 4) eps: %.3g; zeros equal: %s' % (what, share, np.array_equal(got[want == 0], want[want == 0])))
    assert share <= 1.0 and np.array_equal(got[want == 0], want[want == 0])


def test_the_cases_are_built_around_the_plans_chunk():
    from sofacontrol_amd.tpwl import sysid
    assert C == plan_chunk()
    for name, c in sc.build(C).items():
        E, T, nx = c['X'].shape
        n = E * ((T - 1) // c['stride'] + 1)
        assert sysid.select_plan(nx // 2, n)['chunk'] == (sc.C_LARGE if name == 'large_call' else C), name
    counts = sorted(c['X'].shape[1] for n, c in sc.build(C).items() if n.startswith('edge_n'))
    assert counts == [C - 1, C, C + 1, 2 * C + 1]


@pytest.mark.parametrize('name', NAMES)
def test_selection_equals_the_sequential_scan(name):
    c, ref = sc.build(C)[name], sc.reference(name, C)
    ok, bad = sr.certified(ref, c['thr'], c['X'].shape[2] // 2, c['exact'])
    assert ok, bad[:5]
    sel = select(c)
    against_reference(sel, ref, c, what=name)
    sc.check_expect(c, dict(q=sel.q, index=sel.index, complete=sel.complete, stopped_at=sel.stopped_at))
    assert repr(sel).startswith('TPWLPointSelection(%d points' % len(ref['q']))


def test_wild_velocities_change_nothing_without_a_velocity_weight():
    a, b = select(sc.build(C)['wv0_wild']), select(sc.build(C)['wv0_calm'])
    print('wv0: %d and %d points' % (len(a.q), len(b.q)))
    assert np.array_equal(a.index, b.index) and np.array_equal(bits(a.q), bits(b.q)) and np.array_equal(bits(a.dmin), bits(b.dmin))


@pytest.mark.parametrize('name,split', [('two_episodes', 'episode'), ('edge_n3', 1000), ('sep_walk', 'episode'), ('line_65', 100)])
def test_streamed_records_give_the_bits_of_the_concatenation(name, split):
    """X1 then X2 with the first result as the seed, device against device: split at an episode edge and inside a chunk."""
    c = sc.build(C)[name]
    X = c['X']
    X1, X2 = (X[:1], X[1:]) if split == 'episode' else (np.ascontiguousarray(X[:, :split]), np.ascontiguousarray(X[:, split:]))
    whole, a = select(c), select(c, X=X1)
    b = select(c, X=X2, q0=a.q, v0=a.v)
    print('%s: %d points in one call; %d then %d more when streamed' % (name, len(whole.q), len(a.q), len(b.index)))
    assert b.seeded == len(a.q) and b.complete and whole.complete
    assert np.array_equal(bits(b.q), bits(whole.q)) and np.array_equal(bits(b.v), bits(whole.v))
    assert np.array_equal(bits(np.concatenate([a.dmin, b.dmin])), bits(whole.dmin))
    off = (1, 0) if split == 'episode' else (0, split)
    assert np.array_equal(np.vstack([a.index, b.index + np.array(off)]), whole.index)
    against_reference(whole, sc.reference(name, C), c, what=name)


@pytest.mark.parametrize('name,dims', [('episodes_stride', 2), ('dim_r30', 3), ('edge_last_taken', 2), ('sep_walk', 3), ('all_far_cap', 2)])
def test_device_records_give_the_bits_of_host_records(name, dims):
    c = sc.build(C)[name]
    same_bits(select(c, device=dims), select(c))


@pytest.mark.parametrize('name', ['edge_n3', 'dim_r17', 'sep_walk', 'all_far_1024'])
def test_the_same_call_twice_gives_the_same_bits(name):
    c = sc.build(C)[name]
    same_bits(select(c), select(c))


def test_a_device_record_that_is_not_finite_is_refused_with_its_episode_and_row():
    c = dict(sc.build(C)['episodes_stride'])
    X = c['X'].copy()
    X[2, 4, 1], X[2, 5, 0], X[1, 9, 0] = np.inf, np.nan, np.nan                 # rows 5 and 9 are not kept (stride 4)
    with pytest.raises(RuntimeError, match='stpwl_select_points_dev: episode 2, row 4 of the records is not finite; nothing was selected'):
        select(c, X=X, device=2)
    X[2, 4, 1] = 0.0
    sel = select(c, X=X, device=2)                                              # what is not kept is not read
    assert sel.complete and len(sel.q) >= 2


@pytest.mark.parametrize('name', ['dim_r30', 'episodes_stride', 'two_episodes', 'range_1e200'])
def test_the_selection_goes_into_the_fit_and_covers_the_records(name):
    """TPWLSysID takes sel.q, sel.v unchanged; every taken point that is a sample has a sample; every kept row lies within the threshold
    of some point (long-double distances; the case is certified, so a rejected row's distance is below threshold (1 - 32 (r + 4) eps))."""
    from sofacontrol_amd.tpwl.sysid import TPWLSysID
    c, ref = sc.build(C)[name], sc.reference(name, C)
    X, s = c['X'], c['stride']
    E, T, nx = X.shape
    sel = select(c)
    assert sel.complete
    m = 2
    U = np.random.default_rng(5).standard_normal((E, T, m))
    if name == 'range_1e200':                                                   # the fit's targets must stay finite: the far state moves in
        X = X.copy()
        X[0, 100, 2] = 1e3
        sel = select(c, X=X)
        ref = sc.run(sr.scan, c, X=X)
        assert sr.certified(ref, c['thr'], nx // 2)[0] and np.array_equal(sel.index, ref['index'])
    sid = TPWLSysID(sel.q, sel.v, {'q': c['w'][0], 'v': c['w'][1]}, m, 0.01)
    assert sid.add(X, U, stride=s) == E * ((T - 1) // s)
    counts = sid.counts()
    last = ((T - 1) // s) * s
    is_sample = sel.index[:, 1] != last
    print('%s: %d points, %d of them samples, fewest samples of one %d' % (name, len(sel.q), int(is_sample.sum()),
                                                                            int(counts[sel.seeded:][is_sample].min())))
    assert np.all(counts[sel.seeded:][is_sample] > 0)
    cov = sr.coverage(dict(q=sel.q, v=sel.v), X, c['w'][0], c['w'][1], stride=s)
    print('%s: the farthest kept row is %.6g from its nearest point, threshold %.6g' % (name, float(cov), c['thr']))
    assert cov < c['thr'] * (1 - sr.bound(nx // 2))
