"""The half-size lean workgroup's Gram fill stages the packed rows of G in the dead K-tile area and keeps the accumulators of all its
tiles in registers until every wave is through with the staged rows (ql::gram_t<.., STAGE = true>).  A wrong or racy K
does not fail loudly -- the interior point corrects an inexact Hessian and converges anyway -- so these cases ask for EQUALITY: BASELINE
C2, instantiation <4, 60, 4, 50, 50, 4> (SRH_LEAN_HALF=1), solves capped at 5 SCP iterations.  (Both equalities also hold on the build
before the staged fill.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B_BIG, B_SMALL = 600, 8          # 600 > 256 CUs: pairs of rollouts share a CU


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def test_half_size_gram_fill_is_reproducible_and_independent_of_its_neighbours(monkeypatch):
    """(i) 600 rollouts solved three times from the same inputs: xopt, uopt and the SCP iteration counts are identical arrays.
    (ii) the first 8 of them solved alone as a batch of 8 equal their rows of the 600-rollout solve bit for bit (no dependence on
    neighbours, residency or which wave pulled which tile task).  (iii) the same 8 on the full-size kernel (SRH_LEAN_HALF=0): equal
    iteration counts, trajectories within 1e-8 (the bound of this pair in test_gusto_bench_shapes_gpu.py).  (iv) the layout still
    fits two workgroups per CU."""
    import workloads as wl
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2()
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B_BIG, 2, 1354)
    kw = dict(U=Polyhedron(w['UA'], w['Ub']), X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, max_trace=0,
              max_gusto_iters=5, first_solve_cap=5)
    monkeypatch.setenv('SRH_LEAN_HALF', '1')
    g = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0, u_init, x_init, z=z, batch=B_BIG, **kw)
    assert g.kernel_info['lean'] == (4, 60, 4, 50, 50, 4), g.kernel_info
    assert g.kernel_info['lds_bytes_lean'] <= 80 * 1024, g.kernel_info                                   # (iv)
    runs = []
    for _ in range(3):
        g.solve_batch(x0, u_init, x_init, z=z)
        assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0
        runs.append((g.xopt.copy(), g.uopt.copy(), g.iters.copy()))
    for k in (1, 2):                                                                                      # (i)
        d = [float(np.abs(runs[k][j] - runs[0][j]).max()) for j in range(3)]
        print('solve %d vs solve 0: max |dx| %g |du| %g |diters| %g' % (k, d[0], d[1], d[2]))
    for k in (1, 2):
        for j in range(3):
            assert np.array_equal(runs[k][j], runs[0][j]), (k, j)
    S = B_SMALL
    gs = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0[:S], u_init[:S], x_init[:S], z=z[:S], batch=S, **kw)
    assert gs.kernel_info['lean'] == (4, 60, 4, 50, 50, 4), gs.kernel_info
    gs.solve_batch(x0[:S], u_init[:S], x_init[:S], z=z[:S])
    print('batch of 8 vs its rows of the batch of 600: max |dx| %g |du| %g' %
          (np.abs(gs.xopt - runs[0][0][:S]).max(), np.abs(gs.uopt - runs[0][1][:S]).max()))
    assert np.array_equal(gs.iters, runs[0][2][:S])                                                       # (ii)
    assert np.array_equal(gs.xopt, runs[0][0][:S]) and np.array_equal(gs.uopt, runs[0][1][:S])
    monkeypatch.setenv('SRH_LEAN_HALF', '0')
    gf = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0[:S], u_init[:S], x_init[:S], z=z[:S], batch=S, **kw)
    assert gf.kernel_info['lean'] == (4, 60, 4, 50, 7, 4), gf.kernel_info
    gf.solve_batch(x0[:S], u_init[:S], x_init[:S], z=z[:S])
    print('half-size vs full-size: rel x %.2e u %.2e' % (rel(gs.xopt, gf.xopt), rel(gs.uopt, gf.uopt)))
    assert np.array_equal(gf.iters, gs.iters)                                                             # (iii)
    assert rel(gs.xopt, gf.xopt) <= 1e-8 and rel(gs.uopt, gf.uopt) <= 1e-8
