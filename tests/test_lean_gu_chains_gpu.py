"""y = G u of the half-size lean kernel by (column, chain) tasks (ql::g_times_tasks in csrc/locp_lean.h; the schedule itself is checked on
the host in tests/test_lean_gu_schedule_cpu.py).  A lane owns one of the four accumulation chains of a column and sees that chain's
operands in that chain's order, the quad forms (a0 + a1) + (a2 + a3): the mapping moves no bit of the result, so the cases ask for
EQUALITY wherever two runs of the half-size kernel meet -- the Toeplitz generators against the packed rows (the two load paths of the
mapping: a plan created under SRH_LEAN_NO_TOEPLITZ=1 condenses every QP by the general recursion), a solve against its repetition, a batch
against its first rows alone -- for oracle.gusto at the suite's 1e-7 with equal SCP iteration counts, and for the full-size kernel (which
keeps the thread-per-column loop) at the 1e-8 of tests/test_lean_half_newton_gpu.py.  Fixed-horizon instantiations exist at N = 50 only
(lean.hip: SRH_LEAN_VARIANTS), so BASELINE C2 at N = 50 is the smallest shape that reaches the code: NP = 100 columns in rounds of
8, 16 x 5 and 12 columns, 1 to 13 steps, on the Newton front's two waves (all four inputs per wave) and on the whole workgroup (two
inputs per wave) inside every interior-point iteration.  Solves capped at 5 SCP iterations."""
import numpy as np
import pytest

from test_gusto_bench_shapes_gpu import problem, rel
from test_lean_half_newton_gpu import FULL, HALF
from test_lean_products_gpu import FIELDS, assert_identical, assert_oracle, both_paths, box_kernel, make, shape, solve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('points', [1, 64])
def test_generators_against_packed_rows_and_the_oracle(points, monkeypatch):
    """8 C2 rollouts on the half-size kernel (asserted through kernel_info['kernel'] in both_paths -> box_kernel).  One-point table: every
    QP is single-region, every product reads the generators at the immediate offsets of the steps.  64-point table: both kinds of QP in
    one solve.  The default plan equals the SRH_LEAN_NO_TOEPLITZ=1 plan, which walks the packed rows, array for array; all 8 rollouts
    against oracle.gusto at 1e-7 with equal SCP iteration counts."""
    res = both_paths(monkeypatch, 'c2', 50, points, 1, HALF)
    assert_identical(res[False][0], res[True][0], 'half-size, %d points' % points)
    assert res[True][1] == 0 and res[False][1] >= 8, (res[True][1], res[False][1])
    assert_oracle(res[False][0], shape('c2', 50, points), range(8), 'half-size, %d points' % points)


def test_600_rollouts_twice_and_their_first_8_alone(monkeypatch):
    """600 C2 rollouts (above the CU count: two half-size workgroups per CU) twice: identical arrays.  Their first 8 on a plan of their
    own on the same kernel equal those rows bit for bit: no task reads another rollout's rows, generators or partial sums."""
    import workloads as wl
    w = wl.diamond_c2()
    prob = (w,) + tuple(problem(w, 600, 2, 1354))
    g = make(monkeypatch, prob, 600)
    box_kernel(g.kernel_info, HALF)
    runs = [solve(g, prob, 600) for _ in range(2)]
    assert (runs[0]['status'] == 0).all() and g.kernel_info['handed_over'] == 0, g.kernel_info
    assert_identical(runs[1], runs[0], 'solve 1 against solve 0')
    g8 = make(monkeypatch, prob, 8, half=1)
    box_kernel(g8.kernel_info, HALF)
    first = solve(g8, prob, 8)
    for f in FIELDS:
        assert np.array_equal(first[f], runs[0][f][:8]), f


def test_half_size_against_full_size(monkeypatch):
    """The same 64 C2 rollouts on the half-size kernel (tasks) and on the full-size one (a thread per column, unchanged): equal SCP
    iteration counts, trajectories within 1e-8 (the two kernels differ in the rounding of their Gram fills, measured 8.7e-15)."""
    import workloads as wl
    w = wl.diamond_c2()
    prob = (w,) + tuple(problem(w, 64, 2, 1354))
    res = {}
    for half, lean in ((1, HALF), (0, FULL)):
        g = make(monkeypatch, prob, 64, half=half)
        box_kernel(g.kernel_info, lean)
        res[half] = solve(g, prob, 64)
        assert (res[half]['status'] == 0).all() and g.kernel_info['handed_over'] == 0, g.kernel_info
    ex, eu = rel(res[1]['xopt'], res[0]['xopt']), rel(res[1]['uopt'], res[0]['uopt'])
    print('half-size against full-size, 64 rollouts: rel x %.2e u %.2e' % (ex, eu))
    assert np.array_equal(res[1]['iters'], res[0]['iters'])
    assert ex <= 1e-8 and eu <= 1e-8, (ex, eu)
