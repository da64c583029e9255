"""The cases of the TPWL point selection's tests (tests/test_tpwl_select_reference_cpu.py, tests/test_tpwl_select_gpu.py): seeded random
records plus constructed ones, each with what it is built to show (`expect`), and the long-double scan of every case computed once.

A case: {'X' (E, T, 2 r), 'w' = (w_q, w_v), 'thr', 'separate', 'stride', 'q0', 'v0', 'max_points', 'exact' (integer coordinates and unit
weights: tpwl_select_reference's second certificate clause), 'expect'}.  expect: 'count' (points of the table at the end), 'taken' /
'not_taken' (lists of (episode, row)), 'index' (the whole list), 'complete', 'stopped_at'.
C is the chunk of the device's split (stpwl_select_plan); the chunk-edge cases are placed around it."""
import functools

import numpy as np

import tpwl_select_reference as sr

C_DEFAULT = 2048                         # stpwl_select_plan's chunk for calls of at most LARGE_CALL candidates
C_LARGE = 16384                          # .. and of larger calls
LARGE_CALL = 65536


def cloud(seed, n, r, scale=1.0, E=1):
    return scale * np.random.default_rng(seed).uniform(-1.0, 1.0, (E, n, 2 * r))


def walk(seed, E, T, r, step=0.05):
    return np.cumsum(step * np.random.default_rng(seed).standard_normal((E, T, 2 * r)), axis=1)


def state(q, v=None):
    q = np.asarray(q, dtype=np.float64)
    return np.concatenate([np.zeros_like(q) if v is None else np.asarray(v, dtype=np.float64), q])


def _case(X, w=(1.0, 0.5), thr=0.6, separate=False, stride=1, q0=None, v0=None, max_points=1024, exact=False, **expect):
    return dict(X=np.ascontiguousarray(X, dtype=np.float64), w=w, thr=thr, separate=separate, stride=stride, q0=q0, v0=v0,
                max_points=max_points, exact=exact, expect=expect)


@functools.lru_cache(maxsize=None)
def build(C=C_DEFAULT):
    cases = {}
    # chunk edges: candidate counts around C, and taken points placed at the edge
    for i, n in enumerate((C - 1, C, C + 1, 2 * C + 1)):
        cases['edge_n%d' % i] = _case(cloud(10 + i, n, 2))
    X = cloud(20, 2 * C + 1, 2)
    X[0, C - 1], X[0, C] = state([50.0, 50.0]), state([50.1, 50.0])          # the last of a chunk is taken; its neighbour across the edge is not
    cases['edge_last_taken'] = _case(X, taken=[(0, C - 1)], not_taken=[(0, C)])
    X = cloud(21, 2 * C + 1, 2)
    X[0, C], X[0, C + 1], X[0, 2 * C] = state([50.0, 50.0]), state([50.1, 50.0]), state([-50.0, 50.0])
    cases['edge_first_taken'] = _case(X, taken=[(0, C), (0, 2 * C)], not_taken=[(0, C + 1)])
    # inside a chunk: far candidates near each other, all passing against the old table; only the first may be taken
    X = cloud(22, 1500, 2)
    X[0, 700], X[0, 701], X[0, 1400] = state([50.0, 50.0]), state([50.1, 50.0]), state([50.0, 50.2])
    cases['inside_pair'] = _case(X, taken=[(0, 700)], not_taken=[(0, 701), (0, 1400)])
    # dimensions: the unroll edge and the Diamond size
    for r in (1, 16, 17, 30):
        cases['dim_r%d' % r] = _case(walk(30 + r, 2, 150, r), w=(1.0, 0.3), thr=0.2 * np.sqrt(r))
    # table growth past the LDS point tile (16) and a wave (64): N points on a line, each followed by two states near it
    for N in (15, 16, 17, 63, 64, 65, 130):
        X = np.zeros((1, 3 * N, 4))
        for i in range(N):
            X[0, 3 * i], X[0, 3 * i + 1], X[0, 3 * i + 2] = state([3.0 * i, 0.0]), state([3.0 * i + 0.5, 0.0]), state([3.0 * i, 0.5])
        cases['line_%d' % N] = _case(X, w=(1.0, 1.0), thr=2.0, count=N, index=[(0, 3 * i) for i in range(N)], complete=True)
    # weights and mode
    X = cloud(40, 600, 3)
    calm = X.copy()
    calm[..., :3] = 0.0
    X[..., :3] *= 1e150                                                      # wild but finite velocities
    cases['wv0_wild'] = _case(X, w=(1.0, 0.0))
    cases['wv0_calm'] = _case(calm, w=(1.0, 0.0))
    cases['wq0'] = _case(cloud(41, 600, 3), w=(0.0, 1.0))
    rows = [state([0, 0]), state([5, 0]), state([0.1, 0], [7, 0]), state([0.2, 0], [7.1, 0]), state([5.2, 0], [0.3, 0]), state([9, 9], [7, 0])]
    cases['sep_built'] = _case(np.array(rows)[None], w=(1.0, 1.0), thr=1.0, separate=True, index=[(0, 0), (0, 1), (0, 2), (0, 5)])
    cases['sep_walk'] = _case(walk(50, 2, 200, 4), w=(1.0, 0.5), thr=0.45, separate=True)
    cases['sep_wv0'] = _case(cloud(51, 500, 2), w=(1.0, 0.0), separate=True)
    # equality: 3-4-5 offsets, unit weights, threshold 5 -- and a threshold one ulp above the distance
    pts = [(0, 0), (3, 4), (3, 0), (6, 8), (6, 0), (9, 4), (7, 4)]
    X = np.array([state(p, [1.0, 2.0]) for p in pts])[None]
    cases['eq_345'] = _case(X, w=(1.0, 1.0), thr=5.0, exact=True, index=[(0, 0), (0, 1), (0, 3), (0, 4), (0, 5)])
    cases['below_345'] = _case(X, w=(1.0, 1.0), thr=float(np.nextafter(5.0, np.inf)), exact=True, not_taken=[(0, 1)], taken=[(0, 3)])
    # degenerate scans
    cases['all_near'] = _case(cloud(60, 700, 2, scale=0.1), w=(1.0, 1.0), thr=1.0, count=1, index=[(0, 0)], complete=True)
    X = np.array([state([10.0 * i, 0.0]) for i in range(40)])[None]
    cases['all_far_cap'] = _case(X, thr=1.0, max_points=32, count=32, complete=False, stopped_at=(0, 32))
    X = np.array([state([3.0 * i]) for i in range(1100)])[None]
    cases['all_far_1024'] = _case(X, thr=1.0, count=1024, complete=False, stopped_at=(0, 1024))
    seed3 = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    X = np.array([state([0.1, 0.0]), state([0.2, 0.0]), state([50.0, 50.0]), state([90.0, 0.0])])[None]
    cases['cap_at_seed'] = _case(X, thr=1.0, q0=seed3, v0=np.zeros((3, 2)), max_points=3, count=3, index=[], complete=False, stopped_at=(0, 2))
    X = cloud(61, 300, 2)
    X[0, 100, 2] = 1e200                                                     # RANGE: the squared norm overflows, the distance is +inf
    cases['range_1e200'] = _case(X, taken=[(0, 100)])
    # seed
    X = cloud(62, 400, 2)
    X[0, 0] = state([0.1, 0.1], [0.1, 0.1])
    cases['seed_compared'] = _case(X, q0=np.zeros((1, 2)), v0=np.zeros((1, 2)), not_taken=[(0, 0)])
    g = np.array([(a, b) for a in np.linspace(-1, 1, 5) for b in np.linspace(-1, 1, 5)])
    cases['seed_covers'] = _case(cloud(63, 500, 2), w=(1.0, 0.0), thr=0.8, q0=g, v0=np.zeros((25, 2)), count=25, index=[], complete=True)
    # episodes and stride: T - 1 no multiple of the stride; the last kept row of an episode taken; a far row that is not kept
    X = cloud(64, 11, 2, E=3)
    X[1, 8], X[1, 9] = state([30.0, 30.0]), state([-30.0, -30.0])
    cases['episodes_stride'] = _case(X, stride=4, taken=[(1, 8)], not_taken=[(1, 9)])
    cases['two_episodes'] = _case(cloud(70, 1300, 2, E=2))
    # a call above LARGE_CALL candidates: the large chunk, with taken points at its edges
    X = cloud(80, LARGE_CALL + 300, 1)
    X[0, C_LARGE - 1], X[0, C_LARGE], X[0, 2 * C_LARGE] = state([50.0]), state([50.1]), state([-50.0])
    cases['large_call'] = _case(X, thr=0.4, taken=[(0, C_LARGE - 1), (0, 2 * C_LARGE)], not_taken=[(0, C_LARGE)])
    return cases


def run(ref_scan, c, X=None, q0=None, v0=None):
    """A scan function of tpwl_select_reference on case c (optionally on other records / another seed)."""
    return ref_scan(c['X'] if X is None else X, c['w'][0], c['w'][1], c['thr'], separate=c['separate'], stride=c['stride'],
                    q0=c['q0'] if q0 is None else q0, v0=c['v0'] if v0 is None else v0, max_points=c['max_points'])


@functools.lru_cache(maxsize=None)
def reference(name, C=C_DEFAULT):
    """The long-double scan of a case, computed once and shared (read-only)."""
    return run(sr.scan, build(C)[name])


def check_expect(c, res):
    """What the case was built to show, on a result {'q', 'index', 'complete', 'stopped_at'}."""
    e = c['expect']
    idx = [tuple(int(a) for a in row) for row in res['index']]
    if 'count' in e:
        assert len(res['q']) == e['count'], (len(res['q']), e['count'])
    if 'index' in e:
        assert idx == list(e['index']), idx
    for t in e.get('taken', []):
        assert t in idx, t
    for t in e.get('not_taken', []):
        assert t not in idx, t
    if 'complete' in e:
        assert bool(res['complete']) == e['complete']
    if 'stopped_at' in e:
        assert tuple(res['stopped_at']) == tuple(e['stopped_at']), res['stopped_at']
    assert all(row % c['stride'] == 0 for _, row in idx)
