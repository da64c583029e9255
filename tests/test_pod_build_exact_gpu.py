"""GPU: the kernels of the POD build chain, path by path, against tests/pod_build_reference.py.

  srom_gramian_dev        gramian_kernel (whole tiles) and its K-split tail (gramian_tail_kernel)
  srom_modes_dev          modes_kernel
  srom_row_sqnorms_dev / srom_sqdist_rows_dev     row_sqnorm_kernel, abt_dev.h (split-K A B^T), sqdist_kernel
  srom_select_modes_dev   select_modes_kernel
  srom_eigh_topk_dev      the edges of its block rule, its refusal, its optional outputs, its "not settled" return
  compute_POD with rom_dim beyond the rank of the snapshots

Integer-valued inputs are compared bit for bit (np.array_equal: the products are exact in any order of accumulation); real inputs
inside the derived bound (K + 64) 2^-53 |A| |B|^T; a divide by a square root to 2 ulp.  Every output sits between sentinel guards
and every pitched input carries NaN in its padding."""
import ctypes as C

import numpy as np
import pytest

import pod_build_cases as pc
import pod_build_reference as pr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25e300


class Guarded:
    """A device buffer of `count` doubles with GUARD sentinels on either side."""

    def __init__(self, count):
        from sofacontrol_amd import _lib
        self.count = int(count)
        self.buf = _lib.DeviceBuffer.from_array(np.full(self.count + 2 * GUARD, SENTINEL))
        self.ptr = C.c_void_p(self.buf.ptr.value + 8 * GUARD)

    def get(self, shape):
        """The payload, after checking that both guards are untouched."""
        a = self.buf.to_array((self.count + 2 * GUARD,))
        assert np.array_equal(a[:GUARD], np.full(GUARD, SENTINEL)) and np.array_equal(a[-GUARD:], np.full(GUARD, SENTINEL)), 'guard overwritten'
        return a[GUARD:-GUARD].reshape(shape).copy()


def _dev(a):
    from sofacontrol_amd import _lib
    return _lib.DeviceBuffer.from_array(np.ascontiguousarray(a, dtype=np.float64))


def _gramian(S, lds):
    from sofacontrol_amd import _lib
    n_s, n_f = S.shape
    dS, G = _dev(pc.pitched(S, lds)), Guarded(n_s * n_s)
    _lib.check(_lib.lib().srom_gramian_dev(dS.ptr, C.c_int64(n_s), C.c_int64(n_f), C.c_int64(lds), G.ptr, None), 'srom_gramian_dev')
    _lib.sync()
    return G.get((n_s, n_s))


# ----------------------------------------------------------------------------------------------------------- Gramian
@pytest.mark.parametrize('n_s,n_f,lds', pc.GRAMIAN_WHOLE)
def test_gramian_whole_tiles_bit_exact(n_s, n_f, lds):
    from sofacontrol_amd import _lib
    p = _lib.gramian_plan(n_s, n_f)
    assert p['ntail'] == 0 and p['ksplit'] == 1 and p['nfull'] == p['ntile'] * (p['ntile'] + 1) // 2
    S = pc.int_matrix(n_s, n_f, 0)
    G = _gramian(S, lds)
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, pr.gramian(S))


@pytest.fixture(scope='module')
def tail_ntiles():
    from sofacontrol_amd import _lib
    return pc.tail_ntiles(_lib.gramian_plan)


@pytest.mark.parametrize('which', ['ksplit_cap_8', 'ksplit_below_cap'])
def test_gramian_k_split_tail_bit_exact(which, tail_ntiles):
    """The partial last round, split along K into scratch and summed by gramian_tail_kernel: the smallest launch on this card with a
    tail split 8 ways, and the smallest with a tail split k ways, 1 < k < 8 (ntile = 32 and 34 on 256 compute units).  n_f = 1062 is
    67 chunks: parts start at odd chunks (the LDS buffer parity) and the last chunk is ragged; the last tile row is ragged."""
    from sofacontrol_amd import _lib
    ntile = tail_ntiles[0 if which == 'ksplit_cap_8' else 1]
    assert ntile is not None, 'no launch with such a tail up to ntile = 200 on this card'
    n_s, n_f = pc.tail_n_s(ntile), pc.TAIL_N_F
    p = _lib.gramian_plan(n_s, n_f)
    print('tail case %s: ntile %d, plan %r' % (which, ntile, p))
    assert p['ntile'] == ntile and p['ntail'] > 0 and p['nfull'] + p['ntail'] == ntile * (ntile + 1) // 2
    assert p['ksplit'] == 8 if which == 'ksplit_cap_8' else 1 < p['ksplit'] < 8
    nchunk = -(-n_f // pc.KC)
    assert any((nchunk * part // p['ksplit']) & 1 for part in range(p['ksplit'])) and n_f % pc.KC != 0 and n_s % pc.TB != 0
    S = pc.int_matrix(n_s, n_f, 0)
    G = _gramian(S, n_f + pc.TAIL_PAD)
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, pr.gramian(S))


# ------------------------------------------------------------------------------------------------------------- modes
def _modes(S, W, lds):
    from sofacontrol_amd import _lib
    n_s, n_f = S.shape
    k = W.shape[1]
    dS, dW, U = _dev(pc.pitched(S, lds)), _dev(W), Guarded(n_f * k)
    _lib.check(_lib.lib().srom_modes_dev(dS.ptr, C.c_int64(n_s), C.c_int64(n_f), C.c_int64(lds), dW.ptr, C.c_int(k), U.ptr, None),
               'srom_modes_dev')
    _lib.sync()
    return U.get((n_f, k))


@pytest.mark.parametrize('k,n_s,n_f,lds', pc.MODES)
def test_modes_bit_exact(k, n_s, n_f, lds):
    S, W = pc.int_matrix(n_s, n_f, 0), pc.int_matrix(n_s, k, 1)
    assert np.array_equal(_modes(S, W, lds), pr.modes(S, W))


def test_modes_argument_checks():
    from sofacontrol_amd import _lib
    L = _lib.lib()
    dS, dW, U = _dev(np.zeros((4, 8))), _dev(np.zeros((4, 65))), Guarded(8 * 65)

    def call(n_s, n_f, lds, k):
        return L.srom_modes_dev(dS.ptr, C.c_int64(n_s), C.c_int64(n_f), C.c_int64(lds), dW.ptr, C.c_int(k), U.ptr, None)
    for bad in ((4, 8, 8, 0), (4, 8, 8, 65), (0, 8, 8, 2), (4, 0, 8, 2), (4, 8, 7, 2), (4, 8, 8, -1)):
        assert call(*bad) == -1 and b'srom_modes_dev' in L.srh_last_error(), bad
    assert call(4, 8, 8, 2) == 0
    _lib.sync()
    assert np.array_equal(U.get((8 * 65,))[:16], np.zeros(16))                  # only the accepted call wrote, inside its extent


# ------------------------------------------------------------------------------------- squared distances (abt_dev.h)
def _sqdist(S, Y, lds):
    """(row norms of S, D (nc x n_s)) through srom_row_sqnorms_dev and srom_sqdist_rows_dev."""
    from sofacontrol_amd import _lib
    L = _lib.lib()
    n_s, n_f = S.shape
    nc = Y.shape[0]
    dS, dY, xn, D = _dev(pc.pitched(S, lds)), _dev(Y), Guarded(n_s), Guarded(nc * n_s)
    dims = (C.c_int64(n_s), C.c_int64(n_f), C.c_int64(lds))
    _lib.check(L.srom_row_sqnorms_dev(dS.ptr, *dims, xn.ptr, None), 'srom_row_sqnorms_dev')
    _lib.check(L.srom_sqdist_rows_dev(dS.ptr, *dims, dY.ptr, C.c_int(nc), xn.ptr, D.ptr, None), 'srom_sqdist_rows_dev')
    _lib.sync()
    return xn.get((n_s,)), D.get((nc, n_s))


@pytest.mark.parametrize('n_s,nc,n_f,lds', pc.SQDIST)
def test_sqdist_rows_bit_exact(n_s, nc, n_f, lds):
    S, Y = pc.int_matrix(n_s, n_f, 0), pc.int_matrix(nc, n_f, 2)
    xn, D = _sqdist(S, Y, lds)
    assert np.array_equal(xn, pr.row_sqnorms(S))
    assert np.array_equal(D, pr.sqdist_rows(S, Y))


def test_sqdist_rows_real_data_inside_the_bound():
    n_s, nc, n_f, lds = pc.SQDIST_REAL
    S, Y = pc.real_matrix(n_s, n_f, 0), pc.real_matrix(nc, n_f, 2)
    xn, D = _sqdist(S, Y, lds)
    xref = pr.row_sqnorms_ld(S)
    exn = np.abs(xn - xref).astype(np.float64)
    bxn = pr.dot_bound(xref.astype(np.float64), n_f)
    print('row norms: worst error / bound %.3f' % float((exn / bxn).max()))
    assert np.all(exn <= bxn)
    Dref, bound = pr.sqdist_rows_ld(S, Y)
    eD = np.abs(D - np.maximum(Dref, 0)).astype(np.float64)
    print('distances: worst error / bound %.3f' % float((eD / bound).max()))
    assert np.all(eD <= bound)


# ---------------------------------------------------------------------------------------------------- mode selection
def _select(V, w, k):
    from sofacontrol_amd import _lib
    n = w.shape[0]
    dV, dw, Wk = _dev(V), _dev(w), Guarded(n * k)
    _lib.check(_lib.lib().srom_select_modes_dev(dV.ptr, dw.ptr, C.c_int64(n), C.c_int(k), Wk.ptr, None), 'srom_select_modes_dev')
    _lib.sync()
    return Wk.get((n, k))


@pytest.mark.parametrize('n,k', pc.select_cases())
def test_select_modes_to_two_ulp(n, k):
    V, w = pc.select_inputs(n)
    got, ref = _select(V, w, k), pr.scaled_modes(V, w, k)
    assert np.array_equal(ref, V[::-1][:k].T / np.sqrt(w[::-1][:k]))              # every mode of these inputs is live
    assert pr.within_ulps(got, ref, 2)


def test_select_modes_zero_columns_for_vanished_eigenvalues():
    """csrc/mode_rule.h: w_i <= max(1e-28, n eps) w_max or w_i <= 0 gives a zero column, exactly; a w_i just above the threshold is
    divided by."""
    V, w = pc.select_inputs(5)
    w = np.array([-1e-3, 0.0, 0.5 * pr.mode_floor(5) * w[-1], 2.0 * pr.mode_floor(5) * w[-1], w[-1]])
    got, ref = _select(V, w, 5), pr.scaled_modes(V, w, 5)
    assert np.array_equal(got[:, 2:], np.zeros((5, 3)))
    assert np.isfinite(got).all() and pr.within_ulps(got, ref, 2) and np.abs(got[:, 1]).min() > 0


# --------------------------------------------------------------------------------------------------------- rank edge
def _topk(G, k, oversample, want_Wk=True, want_Vt=True):
    """(rc, w, Wk, Vt, trace, iters) of srom_eigh_topk_dev."""
    from sofacontrol_amd import _lib
    n = G.shape[0]
    dG, w = _dev(G), Guarded(k)
    Wk, Vt = Guarded(n * k), Guarded(k * n)
    tr, it = C.c_double(), C.c_int(-1)
    rc = _lib.lib().srom_eigh_topk_dev(dG.ptr, C.c_int64(n), C.c_int(k), C.c_int(oversample), w.ptr, Wk.ptr if want_Wk else None,
                                       Vt.ptr if want_Vt else None, C.byref(tr), C.byref(it), None)
    _lib.sync()
    return rc, w.get((k,)), Wk.get((n, k)), Vt.get((k, n)), tr.value, it.value


def _rank_reference():
    S = pc.rank_snapshots()
    Ur, sr, _ = np.linalg.svd(S.T, full_matrices=False)                 # modes of the snapshot matrix (n_f x n_s)
    return S, Ur[:, :pc.RANK], sr[:pc.RANK]


def test_rank_edge_compute_pod_beyond_the_rank():
    """40 snapshots of rank 3, rom_dim = 6: every output finite, the modes beyond the rank exactly zero, the first three against
    numpy's SVD.  Tolerance of the three modes: the eigenvectors of G = S S^T computed to a backward error of n eps |G| have an
    angle error of at most n eps (sigma_0 / sigma_i)^2 / relgap_i; with sigma_0 / sigma_2 <= 30 and relative gaps >= 0.2 (checked
    on the CPU) that is 40 * 1.1e-16 * 900 / 0.2 = 2e-11, held here with a factor 50 for the two further products: 1e-9.
    Before the two repairs of DESIGN.md section 32 this case did not get as far as a non-finite mode: srom_eigh_dev gave up on
    the Gramian ("Jacobi sweeps did not converge"); with that repaired, the null eigenvalues come out at +-1e-16 w_max and the
    modes beyond the rank are zero by the rule of csrc/mode_rule.h."""
    from sofacontrol_amd.mor.pod import compute_POD
    S, Uref, sref = _rank_reference()
    _, U, k, Sigma = compute_POD(S.T, 1e-4, rom_dim=pc.RANK_K)
    assert k == pc.RANK_K and U.shape == (pc.RANK_NF, pc.RANK_K)
    print('Sigma', Sigma[:8], 'max |U| beyond the rank', np.abs(U[:, pc.RANK:]).max())
    assert np.isfinite(U).all() and np.isfinite(Sigma).all()
    assert np.array_equal(U[:, pc.RANK:], np.zeros((pc.RANK_NF, pc.RANK_K - pc.RANK)))
    np.testing.assert_allclose(Sigma[:pc.RANK], sref, rtol=1e-9)
    np.testing.assert_allclose(np.abs(U[:, :pc.RANK]), np.abs(Uref), rtol=0, atol=1e-9)


def test_rank_edge_leading_eigenpairs_beyond_the_rank():
    """The same Gramian through srom_eigh_topk_dev with k = 6 (block 32)."""
    S, Uref, sref = _rank_reference()
    G = pr.gramian(S)
    rc, w, Wk, Vt, tr, it = _topk(G, pc.RANK_K, -1)
    print('w', w, 'iterations', it, 'max |Wk| beyond the rank', np.abs(Wk[:, pc.RANK:]).max())
    assert rc == 0 and np.isfinite(w).all() and np.isfinite(Wk).all() and np.isfinite(Vt).all()
    assert np.array_equal(Wk[:, pc.RANK:], np.zeros((pc.RANK_N, pc.RANK_K - pc.RANK)))
    np.testing.assert_allclose(w[:pc.RANK], sref ** 2, rtol=0, atol=1e-10 * sref[0] ** 2)
    U = S.T @ Wk
    np.testing.assert_allclose(np.abs(U[:, :pc.RANK]), np.abs(Uref), rtol=0, atol=1e-9)
    assert np.array_equal(U[:, pc.RANK:], np.zeros((pc.RANK_NF, pc.RANK_K - pc.RANK)))


# ------------------------------------------------------------------------------------------ leading eigenpairs, edges
@pytest.mark.parametrize('n,k,oversample', pc.TOPK)
def test_leading_eigenpairs_block_edges(n, k, oversample):
    """Eigenvalues to 1e-10 w_0, residual to 1e-9 w_0, orthonormality to 1e-10 and the trace to 1e-12 (the tolerances of
    tests/test_pod_gpu.py::test_leading_eigenpairs_vs_numpy); Wk against Vt^T / sqrt(w) of the same call to 2 ulp."""
    G, _ = pc.topk_matrix(n, k, oversample)
    rc, w, Wk, Vt, tr, it = _topk(G, k, oversample)
    assert rc == 0
    wref = np.linalg.eigvalsh(G)[::-1][:k]
    res = np.abs(G @ Vt.T - Vt.T * w).max()
    print('n %d k %d block %d: iterations %d, eigenvalue error %.2e w0, residual %.2e w0, orthonormality %.2e' %
          (n, k, pc.topk_block(n, k, oversample), it, np.abs(w - wref).max() / wref[0], res / wref[0], np.abs(Vt @ Vt.T - np.eye(k)).max()))
    assert np.abs(w - wref).max() <= 1e-10 * wref[0]
    assert abs(tr - np.trace(G)) <= 1e-12 * np.trace(G)
    assert np.abs(Vt @ Vt.T - np.eye(k)).max() <= 1e-10
    assert res <= 1e-9 * wref[0]
    assert pr.within_ulps(Wk, Vt.T / np.sqrt(w), 2)
    assert 1 <= it <= 30


def test_leading_eigenpairs_refusal_and_optional_outputs():
    from sofacontrol_amd import _lib
    n, k, ov = pc.TOPK_REFUSED
    G, _ = pc.topk_matrix(n, k, ov - 1)
    rc = _topk(G, k, ov)[0]
    msg = _lib.lib().srh_last_error()
    assert rc == -1 and b'srom_eigh_dev' in msg and b'128' in msg, msg
    # NULL Wk with Vt, NULL Vt with Wk: the other outputs as in the full call (the solve is deterministic), the NULL one untouched
    G, _ = pc.topk_matrix(20, 4, -1)
    rc, w, Wk, Vt, tr, it = _topk(G, 4, -1)
    rc1, w1, Wk1, Vt1, tr1, it1 = _topk(G, 4, -1, want_Wk=False)
    rc2, w2, Wk2, Vt2, tr2, it2 = _topk(G, 4, -1, want_Vt=False)
    assert rc == rc1 == rc2 == 0 and it == it1 == it2 and tr == tr1 == tr2
    assert np.array_equal(w, w1) and np.array_equal(w, w2) and np.array_equal(Vt, Vt1) and np.array_equal(Wk, Wk2)
    assert np.array_equal(Wk1, np.full(Wk.shape, SENTINEL)) and np.array_equal(Vt2, np.full(Vt.shape, SENTINEL))


def test_leading_eigenpairs_flat_tail_reports_not_settled():
    """lam_i = 1 - 1e-4 i: the block cannot settle; the call still succeeds, says 31, and returns finite Ritz values that do not
    exceed the eigenvalues they stand for (Cauchy interlacing for a Rayleigh-Ritz step -- no claim of accuracy)."""
    G, lam = pc.flat_matrix()
    rc, w, Wk, Vt, tr, it = _topk(G, 4, -1)
    print('flat tail: iterations %d, w %r' % (it, w))
    assert rc == 0 and it == 31
    assert np.isfinite(w).all() and np.isfinite(Wk).all() and np.isfinite(Vt).all()
    assert np.all(w <= lam[:4] * (1 + 1e-12))
