"""CPU: keeps the long-double statement of tests/tpwl_table_reference.py honest and enforces the input conditions under which
tests/test_tpwl_table_exact_gpu.py may ask the kernels of csrc/tpwl.hip / csrc/tpwl_dev.h for EQUAL indices:
  - every finite query of every case is `decided` (the undecided share is exactly 0), so float64 rounding cannot move a minimum;
  - every designed tie, placed minimum and non-finite state resolves to the index the design fixes;
  - on the finite queries the float64 oracle (oracle/tpwl.py: np.argmin, np.exp, np.einsum) gives the reference's indices, and its
    weights and blends stay within the bounds the GPU tests use -- the numpy oracle alone would pass them;
  - the tie rollouts visit the designed sequence of points, on ties at every stage."""
import numpy as np
import pytest

from oracle import tpwl as otpwl
import tpwl_table_cases as tc
import tpwl_table_reference as tr


def test_first_min_rules():
    inf, nan = np.inf, np.nan
    assert tr.first_min([3.0, 1.0, 1.0, 2.0]) == 1
    assert tr.first_min([inf, inf, inf]) == 0 and tr.first_min([nan, nan]) == 0 and tr.first_min([inf, nan]) == 0
    assert tr.first_min([inf, 2.0, inf]) == 1
    assert tr.first_min([0.0]) == 0
    for d in ([inf, inf], [nan, nan, nan]):
        assert tr.first_min(d) == int(np.argmin(d))                      # what np.argmin gives where there is no minimum
    assert tr.decided([1.0, 1.0, 1.0], 5) and tr.decided([inf, inf], 5) and tr.decided([0.0, 1.0], 5)
    assert not tr.decided([1.0, 1.0 + 8 * tr.EPS], 5) and tr.decided([1.0, 1.0 + 1e-12, 1.0], 5)
    m = dict(q=np.array([[1.0], [2.0]]), v=np.array([[0.0], [0.0]]), w_q=1.0, w_v=0.0)
    assert tr.nearest(m, [[np.nan, 1.9]]).tolist() == [1]               # w_v == 0: the velocity is not read
    assert tr.nearest(dict(m, w_v=0.5), [[np.nan, 1.9]]).tolist() == [0]
    assert tr.nearest(m, [[0.0, 1e200]]).tolist() == [0] and np.isinf(tr.distances(m, [0.0, 1e200])).all()       # RANGE
    assert tr.nearest(dict(m, w_q=0.0), [[0.0, np.nan]]).tolist() == [0] and np.isnan(tr.distances(dict(m, w_q=0.0), [0.0, np.inf])).all()


def test_pair_groups_place_every_pair():
    assert tc.pair_groups(1) == [] and tc.pair_groups(2) == [[(0, 1)]]
    flat = sorted(p for g in tc.pair_groups(300) for p in g)
    assert flat == sorted([(5, 69), (7, 263), (3, 70), (70, 131), (62, 63), (63, 64), (64, 65), (0, 299)])
    for P, _ in tc.SHAPES:
        for g in tc.pair_groups(P):
            idx = [i for p in g for i in p]
            assert len(idx) == len(set(idx)) and max(idx) < P


@pytest.mark.parametrize('s', tc.SPECS, ids=tc.spec_id)
def test_every_query_is_decided_and_designed(s):
    P, r, w_q, w_v = s
    undecided = total = 0
    fams = set()
    for kind in tc.kinds(s):
        X, want, fam = tc.queries(s, kind)
        idx, D = tc.reference(s, kind)
        fams |= set(fam.tolist())
        ok = tc.finite(X)
        for k in range(len(X)):
            total += 1
            undecided += not tr.decided(D[k], r)
            if want[k] >= 0:
                assert idx[k] == want[k], (kind, fam[k], k, int(idx[k]), int(want[k]))
        # the float64 oracle on the finite queries
        assert np.array_equal(otpwl.nearest_points(tc.table(s, kind), X[ok]), idx[ok]), kind
        # the ties are ties: the first two of the sorted distances are equal, and at a duplicated point both are 0
        for k in np.flatnonzero(np.isin(fam, ['dup-on', 'dup-off', 'mirror', 'equi'])):
            d = np.sort(D[k])
            if P > 1:
                assert d[0] == d[1], (kind, fam[k])
            if fam[k] == 'dup-on':
                assert d[0] == 0
            if fam[k] == 'equi' and (w_q or w_v):
                assert d[0] == d[-1] > 0
    print('%s: %d queries, undecided share %d / %d, families %s' % (tc.spec_id(s), total, undecided, total, sorted(fams)))
    assert undecided == 0
    assert {'random', 'placed', 'nan-q', '+inf', '-inf', '+big', '-big', 'nan-v', 'equi'} <= fams
    if P > 1:
        assert {'dup-on', 'dup-off', 'mirror'} <= fams


@pytest.mark.parametrize('s', tc.SPECS, ids=tc.spec_id)
def test_oracle_weights_within_the_bound(s):
    P, r, w_q, w_v = s
    worst = 0.0
    for kind, (X, fam) in tc.weight_queries(s).items():
        m = tc.table(s, kind)
        for beta in tc.BETAS:
            for x, f in zip(X, fam):
                D = tr.distances(m, x)
                assert tr.decided(D, r)
                Wr = tr.weights(m, x, beta)
                Wo = otpwl.weighting_factors(m, x, beta)
                assert abs(float(Wr.sum()) - 1.0) <= 1e-17 * P + 1e-18
                err, bound = np.abs(Wo - Wr), tc.weight_bound(Wr, D, beta, P)
                assert (err <= bound).all(), (kind, beta, f, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                if f == 'dup-on':
                    assert Wr[tr.first_min(D)] == 1 and Wr.sum() == 1 and np.array_equal(Wo, Wr.astype(float))
                if beta == 0 and D.min() > 0:
                    assert np.array_equal(Wr, np.full(P, tr.LD(1) / P))
                if f == 'near' and beta > 0 and P > 1 and (w_q or w_v):
                    assert (Wr == 0).sum() >= P // 2 and Wr.max() > 0.99
    print('%s: numpy weights use %.3f of the bound at most' % (tc.spec_id(s), worst))


@pytest.mark.parametrize('shape', tc.BLEND_SHAPES, ids=lambda t: '-'.join(map(str, t)))
def test_oracle_blend_within_the_bound(shape):
    r, m, P = shape
    n = 2 * r
    tot = n * n + n * m + n
    model, X = tc.blend_case(*shape)
    for x in X:
        W = otpwl.weighting_factors(model, x, 3.0)
        A, B, d = otpwl.weighted_jacobians(model, x, 3.0)
        for got, T in ((A, model['A_c']), (B, model['B_c']), (d, model['d_c'])):
            assert (np.abs(got - tr.blend(W, T)) <= (P + 2) * tr.EPS * tr.blend_abs(W, T)).all()
    print('n_x %d, m %d: %d elements = %d * 256 %+d' % (n, m, tot, round(tot / 256), tot - 256 * round(tot / 256)))
    assert {(1, 1, 5): 8, (7, 3, 9): 252, (5, 15, 6): 260, (8, 15, 7): 512, (8, 16, 7): 528, (36, 8, 3): 5832}[shape] == tot


@pytest.mark.parametrize('r,P,w_v', [(5, 9, 0.0), (33, 9, 0.0), (5, 70, 0.0), (5, 9, 0.5)])
def test_tie_rollouts_visit_the_designed_points(r, P, w_v):
    model, Ad, Bd, dd, H, z_ref, x0, u, want = tc.tie_rollout(r, P, w_v)
    for b in range(2):
        X, idx = tr.rollout(model, Ad, Bd, dd, x0[b], u[b])
        if b == 0:
            assert idx.tolist() == want.tolist()
        assert len(set(idx.tolist())) >= 3
        for k in range(len(idx)):
            D = tr.distances(model, X[k])
            assert tr.decided(D, r)
            d = np.sort(D)
            if k > 0 or b == 1:
                assert d[0] == d[1] < d[2], (b, k)                       # a two-way tie at every stage after the home point
        Xo = otpwl.rollout(model, Ad, Bd, dd, x0[b], u[b])
        assert np.array_equal(Xo, X.astype(float)) and np.array_equal(X, X.astype(float).astype(tr.LD))          # exact in float64
        Z = tr.ld(H) @ X.T
        assert np.array_equal(Z, Z.astype(float).astype(tr.LD))
    # the two candidates of a tie send the state to different places
    for a, b_ in (tc.pair_groups(P)[0] if P > 9 else [(1, 2), (3, 4), (5, 6), (7, 8)]):
        assert not np.array_equal(dd[a], dd[b_])
