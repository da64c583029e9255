"""Seeded cases of the Koopman fit shared by tests/test_koopman_fit_reference_cpu.py (the oracle's own error, without a GPU) and
tests/test_koopman_fit_gpu.py (the kernels of csrc/koopman_fit.hip on the same numbers).

Records are iid uniform in [-1, 1] (well conditioned), scaled by seeded offsets near 0 and factors near 1 so that the scaling's two
operations round.  A case is a list of `adds` -- (Y (E, T, n_y), U (E, T, m)) per add call -- with a stride and a u_lag.  TR is the
accumulate kernel's pairs per chunk (skoop_fit_plan's rows_per_chunk, 64; tests/test_koopman_fit_surface_cpu.py pins it)."""
import numpy as np

import koopman_fit_reference as kr

TR = 64

# (n_y, m, delays, degree, dmd) -> n, each the smallest shape that reaches what it names
SHAPES = {
    (1, 1, 0, 1, True): 2,        # the smallest
    (4, 1, 0, 2, True): 15,       # one below a tile
    (4, 1, 0, 2, False): 16,      # one tile
    (4, 2, 0, 2, False): 17,      # one above a tile
    (1, 1, 1, 3, False): 21,      # degree 3, delays
    (1, 2, 2, 2, False): 38,      # two delays
    (3, 4, 1, 2, False): 70,      # the Diamond, above 64
    (14, 8, 0, 2, False): 128,    # the limit
}
REFUSED = (14, 9, 0, 2, False)    # n = 129


def layouts(d, n):
    """name -> ([(E, T) per add], stride, u_lag).  T' = pairs + d + 1 rows give `pairs` pairs."""
    T = lambda pairs: pairs + d + 1
    out = {
        'one-pair': ([(1, T(1))], 1, 0),
        'TR-1': ([(1, T(TR - 1))], 1, 1),
        'TR': ([(1, T(TR))], 1, 0),
        'TR+1': ([(1, T(TR + 1))], 1, 1),
        '2TR+1': ([(1, T(2 * TR + 1))], 1, 0),
        'E3-aligned': ([(3, T(TR))], 1, 1),               # every episode is one whole chunk
        'E3-unaligned': ([(3, T(TR + 5))], 1, 0),         # two chunks per episode, the second of 5 pairs
        # an episode of T' = d + 1, and (where one exists) one of T' = d, between two ordinary ones: they contribute nothing
        'empty-between': ([(1, T(20)), (1, d + 1)] + ([(1, d)] if d >= 1 else []) + [(1, T(30))], 1, 0),
        'stride3-lag1': ([(2, 3 * (T(20) - 1) + 2)], 3, 1),   # T = 3 k + 2: no multiple of the stride, T' = k + 1
        'stride3-lag0': ([(1, 3 * (T(9) - 1) + 1)], 3, 0),    # T = 3 k + 1, T' = k + 1: the last row is kept
        'two-adds': ([(2, T(40)), (1, T(40))], 1, 1),
        'one-add': ([(3, T(40))], 1, 1),                  # the same episodes as 'two-adds' in one call
        'solve': ([(3, T(2 * n))], 1, 0),                 # 6 n pairs: the forward comparison of A and B
    }
    return out


CASES = [(shape, name) for shape in SHAPES for name in layouts(shape[2], SHAPES[shape])]
_cache = {}


def case_id(case):
    return '%d-%d-%d-%d-%s-%s' % (case[0][:4] + ('dmd' if case[0][4] else 'const', case[1]))


def scale_of(shape):
    ny, m = shape[0], shape[1]
    rng = np.random.default_rng(4100 + 7 * ny + m)
    return dict(y_offset=rng.uniform(-0.1, 0.1, ny), y_factor=rng.uniform(0.9, 1.1, ny), u_offset=rng.uniform(-0.1, 0.1, m),
                u_factor=rng.uniform(0.9, 1.1, m))


def records(case):
    """dict adds [(Y, U)], stride, u_lag, scale, and the shape's fields."""
    if ('rec', case) in _cache:
        return _cache[('rec', case)]
    shape, name = case
    ny, m, d, degree, dmd = shape
    spec, stride, u_lag = layouts(d, SHAPES[shape])[name]
    # 'one-add' holds the episodes of 'two-adds': the same seed, drawn episode by episode
    seed = 4000 + 97 * list(SHAPES).index(shape) + (10 if name in ('two-adds', 'one-add') else sorted(layouts(d, 1)).index(name))
    rng = np.random.default_rng(seed)
    eps = [(rng.uniform(-1.0, 1.0, (T, ny)), rng.uniform(-1.0, 1.0, (T, m))) for E, T in spec for _ in range(E)]
    adds, at = [], 0
    for E, T in spec:
        adds.append((np.stack([e[0] for e in eps[at:at + E]]).reshape(E, T, ny), np.stack([e[1] for e in eps[at:at + E]]).reshape(E, T, m)))
        at += E
    c = dict(adds=adds, stride=stride, u_lag=u_lag, scale=scale_of(shape), n_y=ny, m=m, delays=d, degree=degree, dmd=dmd, n=SHAPES[shape])
    _cache[('rec', case)] = c
    return c


def expected_pairs(case):
    c = records(case)
    return sum(Y.shape[0] * max(0, (Y.shape[1] - 1) // c['stride'] + 1 - 1 - c['delays']) for Y, _ in c['adds'])


def reference(case, dtype):
    """The sums of a case in `dtype`, cached (and left unchanged by the tests)."""
    if ('sums', case, dtype) not in _cache:
        c = records(case)
        _cache[('sums', case, dtype)] = kr.sums(c['adds'], c['scale'], c['delays'], c['degree'], c['dmd'], c['stride'], c['u_lag'], dtype)
    return _cache[('sums', case, dtype)]


def model_reference(case, dtype, ridge=0.0):
    """(A, B) of a case in `dtype` from that dtype's own sums."""
    if ('fit', case, dtype, ridge) not in _cache:
        s = reference(case, dtype)
        X = kr.solve(s['G'], s['R'], ridge, dtype)
        P = s['R'].shape[0]
        _cache[('fit', case, dtype, ridge)] = (X[:, :P], X[:, P:])
    return _cache[('fit', case, dtype, ridge)]


def e_oracle(case):
    """The float64 statement's distance from long double on A and B of a 'solve' case."""
    A, B = model_reference(case, kr.LD)
    a, b = model_reference(case, np.float64)
    return max(kr.err(a, A), kr.err(b, B))


def smooth_case():
    """The Diamond shape on one smooth trajectory: y_k = 0.97 y_{k-1} + 0.03 xi_k + 0.02 sum u_{k-1}; G is ill conditioned (no forward
    comparison is made on it, the certificate alone)."""
    if 'smooth' in _cache:
        return _cache['smooth']
    rng = np.random.default_rng(4900)
    T, ny, m = 602, 3, 4
    U = rng.uniform(-1.0, 1.0, (1, T, m))
    Y = np.zeros((1, T, ny))
    for k in range(1, T):
        Y[0, k] = 0.97 * Y[0, k - 1] + 0.03 * rng.uniform(-1.0, 1.0, ny) + 0.02 * U[0, k - 1].sum()
    _cache['smooth'] = dict(adds=[(Y, U)], stride=1, u_lag=0, scale=None, n_y=ny, m=m, delays=1, degree=2, dmd=False, n=70)
    return _cache['smooth']


def linear_case(dmd):
    """Records of y_{k+1} = A0 y_k + B0 u_k (d = 0, degree 1, identity scaling): the fit returns A0, B0 and the constant's row."""
    rng = np.random.default_rng(4950)
    ny, m, E, T = 3, 2, 2, 60
    A0 = rng.standard_normal((ny, ny))
    A0 *= 0.8 / np.abs(np.linalg.eigvals(A0)).max()
    B0 = rng.standard_normal((ny, m))
    U = rng.uniform(-1.0, 1.0, (E, T, m))
    Y = np.zeros((E, T, ny))
    Y[:, 0] = rng.uniform(-1.0, 1.0, (E, ny))
    for k in range(T - 1):
        Y[:, k + 1] = Y[:, k] @ A0.T + U[:, k] @ B0.T
    scale = dict(y_offset=np.zeros(ny), y_factor=np.ones(ny), u_offset=np.zeros(m), u_factor=np.ones(m))
    return dict(adds=[(Y, U)], stride=1, u_lag=0, scale=scale, n_y=ny, m=m, delays=0, degree=1, dmd=dmd, A0=A0, B0=B0)
