"""CPU: keeps the long-double filter of tests/ekf_reference.py honest and enforces the input conditions under which
tests/test_ekf_exact_gpu.py may hold the kernels of csrc/observer.hip to a tolerance near round-off:
  - on every case the float64 oracle (oracle/observer.py) agrees with the long-double reference to 1e-11;
  - at every table-path predictor the two nearest table points are more than 1e-6 (relative) apart, so the device and the
    reference pick the same point; every table case visits at least three points;
  - every case carries the label of the kernel that sekf_plan (the dispatch of sekf_create, a host function) gives it;
  - every shape on an MFMA or wide path has the Gauss-Jordan gain (ekf_mfma_kernel once had a one-wave Cholesky branch no shape
    could reach; the elimination's precondition is now part of the dispatch) and the LDS carve of its layout."""
import numpy as np
import pytest

import ekf_cases as ec
import ekf_reference as er

ALL_SPECS = ec.SPECS + ec.LONG_SPECS


def test_chol_solve_against_float64_and_failing_pivot():
    rng = np.random.default_rng(0)
    for m in (1, 2, 5, 16, 17, 33):
        G = rng.standard_normal((m, m))
        S = G @ G.T + m * np.eye(m)
        B = rng.standard_normal((m, 3))
        X = er.chol_solve(S, B)
        assert X.dtype == np.longdouble
        assert er.err(np.linalg.solve(S, B), X) <= 1e-13
        assert float(np.abs(er.ld(S) @ X - B).max()) <= 1e-16 * m * float(np.abs(S).max())      # residual at 80-bit level
        assert er.chol_solve(S, B[:, 0]).shape == (m,)
    for pivot in (0, 1, 4):
        D = np.ones(5); D[pivot] = -1.0
        with pytest.raises(np.linalg.LinAlgError) as info:
            er.chol_solve(np.diag(D), np.ones(5))
        assert info.value.pivot == pivot


def test_update_is_the_joseph_free_textbook_step():
    """The long-double update against the information form (Sigma^-1 + C^T V^-1 C)^-1, an independent statement."""
    rng = np.random.default_rng(1)
    n, ny = 7, 3
    C = rng.standard_normal((ny, n))
    Sg, V = ec.spd(n, 2.0, rng), ec.spd(ny, 0.5, rng)
    x, y, y_ref = rng.standard_normal(n), rng.standard_normal(ny), rng.standard_normal(ny)
    xn, Sn = er.update(C, y_ref, x, Sg, y, V)
    info = np.linalg.inv(Sg) + C.T @ np.linalg.inv(V) @ C
    Sw = np.linalg.inv(info)
    xw = Sw @ (np.linalg.inv(Sg) @ x + C.T @ np.linalg.inv(V) @ (y - y_ref))
    assert er.err(Sw, Sn) <= 1e-12 and er.err(xw, xn) <= 1e-12


@pytest.mark.parametrize('s', ALL_SPECS, ids=ec.spec_id)
def test_oracle_error_margin_and_points(s):
    c = ec.case(s)
    traj, ref, e_oracle = ec.reference(s)
    print('%s: e_oracle %.2e, %d calls, points %s, least margin %.2e' %
          (ec.spec_id(s), e_oracle, len(traj), sorted(set(ref.picks)), min(ref.margins) if ref.margins else float('inf')))
    assert len(traj) == c['steps'] + c['steps'] // 2
    assert e_oracle <= ec.E_ORACLE_MAX, (s, e_oracle)
    if c['form'] == 'table':
        assert len(ref.margins) == c['steps'] and min(ref.margins) > ec.MARGIN, (s, min(ref.margins))
        assert len(set(ref.picks)) >= 3, (s, ref.picks)
    else:
        assert not ref.picks
    for W in (c['W'], c['V'], c['Sigma0']):          # dense, symmetric bit for bit, not a multiple of I
        np.testing.assert_array_equal(W, W.T)
        assert W.shape[0] == 1 or np.abs(W - np.diag(np.diag(W))).max() > 1e-4 * np.abs(W).max()


@pytest.mark.parametrize('shape', ec.INDEFINITE, ids=str)
def test_reference_raises_at_the_expected_pivot(shape):
    c = ec.case(ec.spec(shape))
    assert c['ny'] > 1
    x = c['resets'][0]
    for name, Sigma, pivot in ec.indefinite_sigmas(c):
        np.testing.assert_array_equal(Sigma, Sigma.T)
        assert pivot == 0 or pivot >= c['ny'] / 2
        with pytest.raises(np.linalg.LinAlgError) as info:
            er.update(c['C'], c['y_ref'], x, Sigma, c['y'][0], c['V'])
        assert info.value.pivot == pivot, (name, info.value.pivot, pivot)


def plan(n, ny):
    from sofacontrol_amd import _lib
    return _lib.ekf_plan(n, ny)


def test_every_case_is_labelled_with_the_kernel_it_gets(monkeypatch):
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    shapes = ec.SHAPES + ec.EXPLICIT + ec.LONG + ec.NO_MFMA + ec.INDEFINITE
    for path, n, ny, m in shapes:
        p = plan(n, ny)
        assert p['path'] == ec.PATH_CODE[path], ((path, n, ny), p)
        assert 0 < p['lds_bytes'] <= 160 * 1024 and p['lds_bytes'] % 2560 == 0
        assert p['gain_form'] == (1 if path == 'valu' else 0)
    assert {s[0] for s in ec.SPECS} == {'valu', 'mfma0', 'mfma60', 'wide'}
    monkeypatch.setenv('SRH_EKF_NO_MFMA', '1')
    for path, n, ny, m in ec.NO_MFMA:
        assert plan(n, ny)['path'] == ec.PATH_CODE['valu'], (n, ny)
    for path, n, ny, m in shapes:                              # (72, 32) and (80, 16) do not fit the VALU layout
        assert plan(n, ny)['path'] in (ec.PATH_CODE['valu'], ec.PATH_CODE['refused']), (n, ny)


def test_plan_edges_and_refusals(monkeypatch):
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    code = ec.PATH_CODE
    assert plan(16, 1)['path'] == code['valu'] and plan(17, 1)['path'] == code['mfma0']           # 2 ceil16(n_y) <= ceil16(n_x)
    assert plan(48, 16)['path'] == code['mfma0'] and plan(48, 17)['path'] == code['valu']
    assert plan(64, 32)['path'] == code['mfma0'] and plan(64, 33)['path'] == code['valu']
    assert plan(65, 32)['path'] == code['wide'] and plan(72, 33)['path'] == code['valu']
    assert plan(80, 32)['path'] != code['wide'] and plan(80, 16)['path'] == code['wide']
    assert plan(0, 0)['path'] == plan(8, 9)['path'] == plan(8, 0)['path'] == code['refused']
    assert plan(200, 4)['path'] == code['refused']
    # the VALU layout: 3 n (n | 1) + n_y (n | 1) + n_y (n_y | 1) + 4 max(n, n_y, 16) + 8 doubles, in whole 2560-byte units
    for n, ny in ((8, 6), (30, 30), (4, 3)):
        want = 8 * (3 * n * (n | 1) + ny * (n | 1) + ny * (ny | 1) + 4 * max(n, ny, 16) + 8)
        assert plan(n, ny)['lds_bytes'] == -(-want // 2560) * 2560
    # the MFMA and wide layouts on every shape of paths 2 to 4 (doubles, in whole 2560-byte units), and on each of them the
    # precondition of the elimination ekf_gain_gj<4, 2> that both kernels run: nw = 8 waves of four rows each, two register chunks
    # of 64 columns, a double buffer of 2 (n_y + n_x + 4 nw) + 128 doubles inside the two ny16 x ldy panels carved for it
    nw, seen = 512 // 64, {2: 0, 3: 0, 4: 0}
    for n in range(1, 130):
        for ny in range(1, n + 1):
            p = plan(n, ny)
            if p['path'] not in seen:
                continue
            seen[p['path']] += 1
            n16, ny16, NK = -(-n // 16) * 16, -(-ny // 16) * 16, -(-n // 4) * 4
            ld, ldy = n16 + 1, ny16 + 1
            if p['path'] == code['wide']:
                want = 2 * NK * ld + ny16 * ld + NK * ldy + 3 * ny16 * ldy + 4 * n16 + 8
            else:
                want = 3 * n16 * ld + ny16 * ld + 3 * ny16 * ldy + 4 * max(n16, ny16) + 8
            assert p['lds_bytes'] == -(-8 * want // 2560) * 2560, (n, ny, p)
            assert ny <= 4 * nw and ny <= 64 and ny + n <= 128 and 2 * (ny + n + 4 * nw) + 128 <= 2 * ny16 * ldy, (n, ny, p)
    assert seen == {2: 992, 3: 32, 4: 384}, seen
    assert plan(60, 30)['lds_bytes'] == 145920 and plan(72, 30)['lds_bytes'] == 161280


def test_mfma_cholesky_fallback_is_unreachable(monkeypatch):
    """Every (n_x, n_y) with n_y <= n_x < 130 that the dispatch puts on an MFMA kernel takes the Gauss-Jordan gain.  This
    showed the one-wave Cholesky / triangular-inverse branch ekf_mfma_kernel once had to be dead code; the branch is gone,
    and the count of shapes per path pins that removing it moved no shape to another kernel."""
    monkeypatch.delenv('SRH_EKF_NO_MFMA', raising=False)
    seen = {2: 0, 3: 0, 4: 0}
    for n in range(1, 130):
        for ny in range(1, n + 1):
            p = plan(n, ny)
            if p['path'] in seen:
                seen[p['path']] += 1
                assert p['gain_form'] == 0, (n, ny, p)
            elif p['path'] == 1:
                assert p['gain_form'] == 1
    assert seen == {2: 992, 3: 32, 4: 384}, seen
