"""Seeded TPWL tables and query states for the exact tests of the table kernels (tests/test_tpwl_table_reference_cpu.py without a
GPU, tests/test_tpwl_table_exact_gpu.py on one).  Built on oracle.tpwl.synthetic_model; every table and query list is built once.

A spec is (P, r, w_q, w_v).  For a spec there are several tables ("kinds"), each with its list of queries:
  'rand'  the synthetic model.  Queries, interleaved so that every batch mixes them: random states; states next to the points 0, 63,
          64, P - 1, 255, 256 (the minimum placed on a lane / round / thread-stride boundary); non-finite states (NaN, +inf, -inf or
          +-1e200 in one position coordinate; NaN in one velocity coordinate).
  'dupK'  the pairs of group K made identical rows (q and v): the query at the duplicated point (d = 0 twice) and one off it.
  'mirK'  the pairs of group K made mirror images s_a = c + delta, s_b = c - delta of a dyadic centre (both parts of the state, far
          outside the cloud of the other points): the query at c.
  'equi'  every point at +-2^-3 e_j (both parts): the query at 0, all points equidistant, the expected index 0.
The pairs: both in one lane's stride of tpwl::nearest_wave (5, 69) and one thread's stride of weights_kernel (7, 263); in different
lanes (3, 70), (70, 131); adjacent across the lane / round boundary (62, 63), (63, 64), (64, 65); first and last (0, P - 1) -- those that
fit P, packed into groups of disjoint pairs.  The A/B/d tables of the two points of a pair stay different: a wrong choice shows.

Each query carries `want`: the index the design fixes (the first of a pair, the placed point, 0 for a state that is not a number), or
-1 where only the reference decides (random states)."""
import numpy as np

from oracle import tpwl as otpwl
import tpwl_table_reference as tr

M = 2                                     # inputs of every table model here
SHAPES = [(1, 1), (2, 2), (63, 15), (64, 16), (64, 32), (65, 17), (64, 33), (128, 31), (129, 5), (257, 3), (300, 5), (7, 48)]
SPECS = [(P, r, 1.0, w_v) for P, r in SHAPES for w_v in (0.0, 0.5)] + [(64, 16, 0.0, 1.0), (129, 5, 0.0, 0.0)]
N_RANDOM = 24


def spec_id(s):
    return 'P%d-r%d-wq%g-wv%g' % s


def pair_groups(P):
    """The placed pairs that fit P, greedily packed into groups of disjoint pairs."""
    pairs = []
    for i, j in [(5, 69), (7, 263), (3, 70), (70, 131), (62, 63), (63, 64), (64, 65), (0, P - 1)]:
        if i < j < P and (i, j) not in pairs:
            pairs.append((i, j))
    groups = []
    for p in pairs:
        for g in groups:
            if not {p[0], p[1]} & {i for q in g for i in q}:
                g.append(p)
                break
        else:
            groups.append([p])
    return groups


def kinds(s):
    n = len(pair_groups(s[0]))
    return ['rand'] + ['dup%d' % k for k in range(n)] + ['mir%d' % k for k in range(n)] + ['equi']


def _seed(s, salt):
    P, r, w_q, w_v = s
    return 100000 * salt + 100 * P + r + (7 if w_v else 0) + (13 if not w_q else 0)


_base, _tables, _queries = {}, {}, {}


def table(s, kind):
    """The model dict (oracle/tpwl.py) of the spec and kind, with discrete tables under 'A_d', 'B_d', 'd_d' (forward Euler at
    dt = 0.01, A_d = I + dt A_c, ...: they only have to differ from point to point and from the continuous ones)."""
    key = (s, kind)
    if key in _tables:
        return _tables[key]
    P, r, w_q, w_v = s
    if (P, r) not in _base:                            # the A/B/d tables of a shape are shared by its kinds and weights (read only)
        b = otpwl.synthetic_model(r, M, P, seed=1000 + 100 * P + r)
        b['A_d'] = np.eye(2 * r) + 0.01 * b['A_c']
        b['B_d'], b['d_d'] = 0.01 * b['B_c'], 0.01 * b['d_c']
        _base[(P, r)] = b
    b = _base[(P, r)]
    m = dict(b, q=b['q'].copy(), v=b['v'].copy(), w_q=w_q, w_v=w_v)
    rng = np.random.default_rng(_seed(s, 2) + sum(map(ord, kind)))
    if kind.startswith('dup'):
        for i, j in pair_groups(P)[int(kind[3:])]:
            m['q'][j], m['v'][j] = m['q'][i], m['v'][i]
    elif kind.startswith('mir'):
        for k, (a, b) in enumerate(pair_groups(P)[int(kind[3:])]):
            c = 32.0 * (k + 1) + rng.integers(-8, 9, 2 * r) / 8.0
            delta = rng.choice([-0.25, -0.125, 0.125, 0.25], 2 * r)
            m['v'][a], m['q'][a] = (c + delta)[:r], (c + delta)[r:]
            m['v'][b], m['q'][b] = (c - delta)[:r], (c - delta)[r:]
    elif kind == 'equi':
        for i in range(P):
            e = np.zeros(r)
            e[i % r] = 0.125 * (-1.0) ** (i // r)
            m['q'][i], m['v'][i] = e, e
    _tables[key] = m
    return m


def points(m):
    return np.concatenate((m['v'], m['q']), axis=1)


def _random_states(rng, count, r):
    return np.concatenate((0.3 * rng.standard_normal((count, r)), 3.0 * rng.standard_normal((count, r))), axis=1)


def queries(s, kind):
    """(X (Q, n_x), want (Q,), family (Q,) of str) for the table of the spec and kind."""
    key = (s, kind)
    if key in _queries:
        return _queries[key]
    P, r, w_q, w_v = s
    m = table(s, kind)
    pts = points(m)
    rng = np.random.default_rng(_seed(s, 3) + sum(map(ord, kind)))
    none = w_q == 0 and w_v == 0                       # every distance is 0: the first point
    out = []
    if kind == 'rand':
        rand = [(x, -1, 'random') for x in _random_states(rng, N_RANDOM, r)]
        placed = [(pts[t] + 1e-3 * rng.standard_normal(2 * r), t, 'placed')
                  for t in sorted({t for t in (0, 63, 64, P - 1, 255, 256) if t < P})]
        bad = []
        base = _random_states(rng, 8, r)
        for k, (off, val, fam) in enumerate([(r, np.nan, 'nan-q'), (r, np.inf, '+inf'), (r, -np.inf, '-inf'), (r, 1e200, '+big'),
                                             (r, -1e200, '-big'), (0, np.nan, 'nan-v'), (r, np.nan, 'nan-q'), (0, np.nan, 'nan-v')]):
            x = base[k].copy()
            x[off + (r - 1 if k >= 6 else 0)] = val                      # the first coordinate, then the last one (the tail of the sums)
            want = 0
            if fam == 'nan-v' and w_v == 0:                              # not read: the index of the finite state
                want = int(tr.first_min(tr.distances(m, base[k])))
            bad.append((x, want, fam))
        lists = [rand, placed, bad]
        while any(lists):                                                # interleave
            for l in lists:
                if l:
                    out.append(l.pop(0))
    elif kind.startswith('dup'):
        for i, j in pair_groups(P)[int(kind[3:])]:
            out.append((pts[i].copy(), i, 'dup-on'))
            out.append((pts[i] + 1e-3 * rng.standard_normal(2 * r), i, 'dup-off'))
    elif kind.startswith('mir'):
        for a, b in pair_groups(P)[int(kind[3:])]:
            out.append(((pts[a] + pts[b]) / 2, a, 'mirror'))
    else:
        out.append((np.zeros(2 * r), 0, 'equi'))
    X = np.stack([o[0] for o in out])
    want = np.array([0 if (none and o[1] >= 0) else o[1] for o in out], dtype=np.int32)
    fam = np.array([o[2] for o in out])
    _queries[key] = (X, want, fam)
    return _queries[key]


_ref = {}


def reference(s, kind):
    """(idx (Q,), D (Q, P) long double) of the long-double reference for queries(s, kind)."""
    key = (s, kind)
    if key not in _ref:
        X = queries(s, kind)[0]
        D = np.stack([tr.distances(table(s, kind), x) for x in X])
        _ref[key] = (np.array([tr.first_min(d) for d in D], dtype=np.int32), D)
    return _ref[key]


def finite(X):
    return np.isfinite(X).all(axis=1) & (np.abs(X).max(axis=1) < 1e100)


# ------------------------------------------------------------------------------------ weights
BETAS = (0.0, 3.0, 50.0)


def weight_queries(s):
    """{kind: (X, family)} for stpwl_weights: random states and states 1e-9 (relative to the table's scale) next to a point on 'rand';
    the duplicated points themselves on 'dup0' (one-hot at the first duplicate)."""
    P, r, w_q, w_v = s
    rng = np.random.default_rng(_seed(s, 4))
    pts = points(table(s, 'rand'))
    near = [pts[t] + 1e-9 * rng.standard_normal(2 * r) for t in sorted({0, P // 2, P - 1})]
    out = {'rand': (np.concatenate((_random_states(rng, 6, r), np.stack(near))), np.array(['random'] * 6 + ['near'] * len(near)))}
    if pair_groups(P):
        d = points(table(s, 'dup0'))
        on = [d[i] for i, _ in pair_groups(P)[0]]
        out['dup0'] = (np.stack(on), np.array(['dup-on'] * len(on)))
    return out


def weight_bound(W_ref, D, beta, P):
    """The componentwise bound: 16 eps (1 + beta d_i / d_min) w_i + P eps w_i.  The first term covers the error of the
    exponent's argument (each d carries a few eps; exp turns an absolute error of its argument into a relative one), the second the
    sum of P terms.  Under it lies the floor of the number format: the kernel, like numpy, forms e_i = exp(-beta d_i / d_min) in
    float64 and divides by S = sum_j e_j (S >= exp(-beta): the nearest point's term).  Below its smallest normal number, 2.2e-308,
    float64 has no relative precision (and reaches 0 long before the 80-bit reference does), so e_i carries an absolute error of up to
    that number and w_i one of up to 2.2e-308 / S."""
    with np.errstate(all='ignore'):
        ratio = np.where(D.min() > 0, D / D.min(), 0.0)
        S = np.exp(-tr.LD(beta) * ratio).sum()
    return (16 * tr.EPS * (1 + beta * ratio) + P * tr.EPS) * W_ref + F64_TINY / S


F64_TINY = float(np.finfo(np.float64).tiny)


# (r, m, P): n^2 + n m + n next to multiples of 256 (blend_kernel tiles the elements in grid.y blocks of 256)
BLEND_SHAPES = [(1, 1, 5),        # n_x = 2: 8 elements
                (7, 3, 9),        # 252 = 256 - 4
                (5, 15, 6),       # 260 = 256 + 4
                (8, 15, 7),       # 512 = 2 * 256
                (8, 16, 7),       # 528 = 2 * 256 + 16
                (36, 8, 3)]       # n_x = 72, m = 8: 5832 = 22 * 256 + 200


def blend_case(r, m, P):
    model = otpwl.synthetic_model(r, m, P, seed=31 * r + m, w_v=0.5)
    rng = np.random.default_rng(17 * r + m)
    X = _random_states(rng, 3, r)
    return model, X


# ------------------------------------------------------------------------------------ rollouts that land on ties
def tie_rollout(r, P, w_v, N=9, seed=5):
    """Tables of the test's own: A_d = B_d = 0, so x_{k+1} = d_d[i_k] exactly, and d_d sends the state onto a tie: from the home point h
    (in no pair) to pair 0, from the FIRST point of pair k to pair k + 1 (cyclic), from the second point of any pair and from every
    other point back to h -- a wrong choice at a tie shows in the next state.  Pairs alternate between duplicated rows (the state lands
    on the point) and mirror images (the state lands on their midpoint).  All entries are dyadic with a few bits: every distance
    comparison and the output z = H x + z_ref (integer H, z_ref) are exact in float64 and in the reference alike.
    Returns model, Ad, Bd, dd, H, z_ref, x0 (2, n), u (2, N, m), idx (N,) expected for the first rollout."""
    rng = np.random.default_rng(seed + r + P)
    n, m = 2 * r, 3
    model = otpwl.synthetic_model(r, m, P, seed=seed, w_v=w_v)
    S = rng.integers(-64, 65, (P, n)).astype(float)                      # integer points, a few units apart at least (asserted on the CPU)
    groups = pair_groups(P)
    pairs = groups[0] if P > 9 else [(1, 2), (3, 4), (5, 6), (7, 8)]
    used = {i for p in pairs for i in p}
    h = next(i for i in range(P) if i not in used)
    target = []
    for k, (a, b) in enumerate(pairs):
        if k % 2 == 0:
            S[b] = S[a]
            target.append(S[a].copy())
        else:
            delta = rng.choice([-0.25, 0.25], n)
            c = S[a].copy()
            S[a], S[b] = c + delta, c - delta
            target.append(c)
    model['v'], model['q'] = S[:, :r].copy(), S[:, r:].copy()
    dd = np.tile(S[h], (P, 1))
    dd[h] = target[0]
    for k, (a, b) in enumerate(pairs):
        dd[a] = target[(k + 1) % len(pairs)]
    Ad, Bd = np.zeros((P, n, n)), np.zeros((P, n, m))
    H = rng.integers(-2, 3, (6, n)).astype(float)
    z_ref = rng.integers(-4, 5, 6).astype(float)
    x0 = np.stack((S[h], target[1 % len(target)]))                       # the second rollout starts on a tie
    u = rng.uniform(1.0, 800.0, (2, N, m))
    idx = np.array([h] + [pairs[k % len(pairs)][0] for k in range(N - 1)], dtype=np.int32)
    return model, Ad, Bd, dd, H, z_ref, x0, u, idx
