"""CPU: the references, the input conditions and the Gramian launch plan behind tests/test_pod_build_exact_gpu.py.

  - the float64 references of the integer data equal Python int arithmetic on sampled entries, and the data meet the conditions
    tests/pod_build_cases.py promises (integer entries of at most 8, the last column and last row of magnitude 8, distinct rows);
  - the long-double reference and float64 numpy agree inside the derived bound (tests/pod_build_reference.py);
  - srom_gramian_plan (a host function for cus > 0) at 256 compute units: the edges of every condition of the tail rule."""
import numpy as np
import pytest

import pod_build_cases as pc
import pod_build_reference as pr

CUS = 256
SLOTS = 2 * CUS


def _sample(rng, n, count=12):
    return sorted({0, n - 1} | set(int(i) for i in rng.integers(0, n, count)))


def test_integer_data_conditions():
    shapes = {(n_s, n_f) for n_s, n_f, _ in pc.GRAMIAN_WHOLE} | {(n_s, n_f) for _, n_s, n_f, _ in pc.MODES}
    shapes |= {(n_s, n_f) for n_s, _, n_f, _ in pc.SQDIST} | {(pc.tail_n_s(32), pc.TAIL_N_F), (pc.tail_n_s(34), pc.TAIL_N_F)}
    for n_s, n_f in sorted(shapes):
        S = pc.int_matrix(n_s, n_f, 0)
        assert S.shape == (n_s, n_f) and np.array_equal(S, np.round(S)) and np.abs(S).max() <= 8
        assert (np.abs(S[:, -1]) == 8).all() and (np.abs(S[-1]) == 8).all()
        if n_f >= 4:
            assert len(np.unique(S, axis=0)) == n_s, (n_s, n_f)
        assert 64 * n_f < 2 ** 53                                          # every partial sum of every product is exact


def test_integer_references_equal_python_int_arithmetic():
    rng = np.random.default_rng(0)
    for n_s, n_f, _ in pc.GRAMIAN_WHOLE + [(pc.tail_n_s(32), pc.TAIL_N_F, 0)]:
        S = pc.int_matrix(n_s, n_f, 0)
        G = pr.gramian(S)
        assert np.array_equal(G, G.T)
        for i in _sample(rng, n_s):
            for j in _sample(rng, n_s, 4):
                assert G[i, j] == pr.gramian_entry_pyint(S, i, j)
    for k, n_s, n_f, _ in pc.MODES:
        S, W = pc.int_matrix(n_s, n_f, 0), pc.int_matrix(n_s, k, 1)
        U = pr.modes(S, W)
        for i in _sample(rng, n_f, 6):
            for j in _sample(rng, k, 4):
                assert U[i, j] == pr.modes_entry_pyint(S, W, i, j)
    for n_s, nc, n_f, _ in pc.SQDIST:
        S, Y = pc.int_matrix(n_s, n_f, 0), pc.int_matrix(nc, n_f, 2)
        D = pr.sqdist_rows(S, Y)
        assert D.shape == (nc, n_s)
        for c in _sample(rng, nc, 4):
            for i in _sample(rng, n_s, 6):
                assert D[c, i] == pr.sqdist_entry_pyint(S, Y, c, i)


def test_long_double_reference_agrees_with_float64_inside_the_bound():
    n_s, nc, n_f, _ = pc.SQDIST_REAL
    S, Y = pc.real_matrix(n_s, n_f, 0), pc.real_matrix(nc, n_f, 2)
    col = np.abs(S).max(axis=0)
    assert col.max() / col.min() >= 1e4                                     # the columns really span decades
    P, bound = pr.abt_ld(S, Y), pr.abt_bound(S, Y)
    assert (bound > 0).all() and np.all(np.abs(S @ Y.T - P) <= bound)
    xn = pr.row_sqnorms_ld(S)
    assert np.all(np.abs(pr.row_sqnorms(S) - xn) <= pr.dot_bound(xn.astype(np.float64), n_f))
    D, dbound = pr.sqdist_rows_ld(S, Y)
    assert np.all(np.abs(pr.sqdist_rows(S, Y) - np.maximum(D, 0)) <= dbound)
    # the bound is not idle: it sits within a factor (K + 67) of one rounding of the terms, far below the values it guards
    assert np.median(dbound / np.abs(D).astype(np.float64)) < 1e-10


def test_mode_selection_reference_and_host_rule():
    """scaled_modes states the rule of csrc/mode_rule.h; modes_from_gramian (the host route of the sharded build) follows it."""
    from sofacontrol_amd.mor.pod import modes_from_gramian
    V, w = pc.select_inputs(5)
    w = np.array([-1e-3, 0.0, 0.5 * pr.mode_floor(5) * w[-1], w[3], w[4]])
    Wk = pr.scaled_modes(V, w, 5)
    assert np.array_equal(Wk[:, 2:], np.zeros((5, 3))) and np.array_equal(Wk[:, 0], V[4] / np.sqrt(w[4]))
    S = pc.rank_snapshots()
    G = S @ S.T
    assert np.linalg.matrix_rank(S) == pc.RANK
    Wh, k, Sigma = modes_from_gramian(S, G, 1e-4, rom_dim=pc.RANK_K, eigh=lambda A: np.linalg.eigh(A))
    assert k == pc.RANK_K and np.isfinite(Wh).all() and np.isfinite(Sigma).all()
    assert np.array_equal(Wh[:, pc.RANK:], np.zeros((pc.RANK_N, pc.RANK_K - pc.RANK))) and np.abs(Wh[:, :pc.RANK]).max(axis=0).min() > 0
    sv = np.linalg.svd(S, compute_uv=False)
    np.testing.assert_allclose(Sigma[:pc.RANK], sv[:pc.RANK], rtol=1e-12)
    # input conditions of the rank-edge GPU test: sigma_0 / sigma_2 <= 30 and relative gaps >= 0.2 (see its docstring)
    assert sv[0] / sv[2] <= 30 and min(1 - sv[1] / sv[0], 1 - sv[2] / sv[1]) >= 0.2


def test_leading_eigenpair_matrices_meet_their_conditions():
    for n, k, ov in pc.TOPK:
        G, lam = pc.topk_matrix(n, k, ov)
        b = pc.topk_block(n, k, ov)
        assert np.array_equal(G, G.T) and k <= b <= 128
        if b < n:
            assert lam[b - 1] / lam[b] >= 1e6 > 10
        np.testing.assert_allclose(np.linalg.eigvalsh(G)[::-1][:b], lam[:b], rtol=1e-12)
    assert {pc.topk_block(*c) for c in pc.TOPK} == {5, 20, 16, 128}
    n, k, ov = pc.TOPK_REFUSED
    assert (k + ov + 15) & ~15 > 128


# --------------------------------------------------------------------------------------------------------- the plan
def _plan(n_s, n_f, cus=CUS):
    from sofacontrol_amd import _lib
    p = _lib.gramian_plan(n_s, n_f, cus)
    assert (p['ntile'], p['nfull'], p['ntail'], p['ksplit']) == pc.plan_model(n_s, n_f, cus), (n_s, n_f, cus)
    nblk = p['ntile'] * (p['ntile'] + 1) // 2
    assert p['nfull'] + p['ntail'] == nblk and 1 <= p['ksplit'] <= 8 and (p['ksplit'] == 1 or p['ntail'] > 0)
    return p, nblk


def test_gramian_plan_is_declared_and_needs_no_gpu():
    import ctypes as C
    from test_abi_cpu import declared_symbols
    from sofacontrol_amd import _lib
    assert 'srom_gramian_plan' in declared_symbols()
    nt = C.c_int(-1)
    L = _lib.lib()
    assert L.srom_gramian_plan(C.c_int64(300), C.c_int64(1000), C.c_int(CUS), C.byref(nt), None, None, None) == 0 and nt.value == 3
    assert L.srom_gramian_plan(C.c_int64(300), C.c_int64(1000), C.c_int(CUS), None, None, None, None) == 0
    assert L.srom_gramian_plan(C.c_int64(0), C.c_int64(1000), C.c_int(CUS), None, None, None, None) != 0
    assert b'srom_gramian_plan' in L.srh_last_error()
    assert L.srom_gramian_plan(C.c_int64(5), C.c_int64(0), C.c_int(CUS), None, None, None, None) != 0


def test_gramian_plan_edges_at_256_cus():
    n_f = pc.TAIL_N_F                                     # 67 chunks
    # nblk == slots and nblk == slots + 1.  nblk is a triangular number and neither 512 nor 513 is one, so at 256 CUs the nearest are
    # 496 (ntile = 31: one round, not full) and 528 (ntile = 32, below); the equalities themselves are met on cards of 248 CUs
    # (496 = slots: a full round and nothing behind it) and of 7 CUs (ntile = 5: 15 = slots + 1, a tail of one tile)
    p, nblk = _plan(128 * 31, n_f)
    assert nblk == 496 <= SLOTS and p['ntail'] == 0 and p['ksplit'] == 1
    p, nblk = _plan(128 * 31, n_f, cus=248)
    assert nblk == 2 * 248 and p['ntail'] == 0 and p['ksplit'] == 1
    p, nblk = _plan(128 * 5, n_f, cus=7)
    assert nblk == 2 * 7 + 1 and (p['nfull'], p['ntail'], p['ksplit']) == (14, 1, 8)
    # 2 * rem == slots against 2 * rem == slots + 2, at 256 CUs: rem = 256 and rem = 257
    found = {}
    for ntile in range(32, 600):
        rem = (ntile * (ntile + 1) // 2) % SLOTS
        if rem in (256, 257) and rem not in found:
            found[rem] = ntile
    assert set(found) == {256, 257}, found
    p, _ = _plan(128 * found[256], n_f)
    assert p['ntail'] == 256 and p['ksplit'] == 2
    p, _ = _plan(128 * found[257], n_f)
    assert p['ntail'] == 0 and p['ksplit'] == 1
    # nchunk 63 against 64 (n_f = 1008 / 1009), on a shape whose tail is otherwise taken
    p, _ = _plan(pc.tail_n_s(32), 63 * 16)
    assert p['ntail'] == 0
    p, _ = _plan(pc.tail_n_s(32), 63 * 16 + 1)
    assert p['ntail'] == 16 and p['ksplit'] == 8
    # the cap of 8 (slots / rem = 32) and a split of 4 (512 / 118)
    p, nblk = _plan(pc.tail_n_s(32), n_f)
    assert nblk == 528 and (p['nfull'], p['ntail'], p['ksplit']) == (512, 16, 8)
    p, nblk = _plan(pc.tail_n_s(35), n_f)
    assert nblk == 630 and (p['nfull'], p['ntail'], p['ksplit']) == (512, 118, 4)
    # what the GPU test searches for on the card it runs on, here for 256 CUs: ntile = 34 (nblk = 595, rem = 83) is split 6 ways
    assert pc.tail_ntiles(lambda n_s, nf: _plan(n_s, nf)[0]) == (32, 34)
    p, nblk = _plan(pc.tail_n_s(34), n_f)
    assert nblk == 595 and (p['nfull'], p['ntail'], p['ksplit']) == (512, 83, 6)
    # one tile, and every ntile up to 150: the restated rule and nfull + ntail == nblk (checked inside _plan)
    for ntile in range(1, 151):
        _plan(128 * ntile - 5, n_f)
