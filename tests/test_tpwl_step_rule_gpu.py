"""GPU: the TPWL plant step is ONE rule across the kernels that use it (csrc/tpwl_dev.h, "THE STEP RULE").

The advance kernels of the two closed loops on a TPWL plant -- loop_advance_kernel (csrc/gusto_loop.hip) and rompc_loop_advance_kernel
(csrc/rompc_loop.hip) -- step the plant for n_keep sub-steps under their own feedback laws.  Fed the inputs U they recorded, a rollout of
the same plant tables at dt_sim from the same state must give their plant states bit for bit: on the staged path (rollout_staged_kernel,
the plant's own handle) and on the plain path (rollout_kernel, a handle of the same tables created under SRH_TPWL_ROLLOUT_PLAIN=1).
No disturbance (W = None): x' is the step rule's sum and nothing else.

Cases are the suites' own smallest (tests/cl_cases.py, tests/rompc_loop_cases.py, B = 3) with the disturbance taken out: g6 (n_x = 8, 32
slices), m8 (n_x = 12: 21 slices, 252 of the 256 threads live), r36 (n_x = 72: 3 slices, the wave search).  The plant's point sequence
comes from the float64 reference on the CPU and is asserted before anything runs on the device: whether a member changes region inside
the sub-steps (the panel is reloaded) or stays in one (it is loaded once) is stated per case."""
import os

import numpy as np
import pytest

import cl_cases as cc
import cl_reference as cr
import rompc_loop_cases as rc
from helpers import product_tpwl

pytestmark = pytest.mark.gpu

_plain = {}


def plain_twin(mname, dt_sim):
    """The model once more with its dt_sim handle created under SRH_TPWL_ROLLOUT_PLAIN=1 (same CPU tables as the plant's)."""
    if (mname, dt_sim) not in _plain:
        m = cc.model(mname)
        tp = product_tpwl(m['model'], m['U'], m['q_ref'], m['v_ref'], m['Hf'])
        old = os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
        try:
            os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = '1'
            tp.handle_for(dt_sim, tables=cc.tables(mname, dt_sim))
        finally:
            os.environ.pop('SRH_TPWL_ROLLOUT_PLAIN', None)
            if old is not None:
                os.environ['SRH_TPWL_ROLLOUT_PLAIN'] = old
        _plain[(mname, dt_sim)] = tp
    return _plain[(mname, dt_sim)]


def check_sequence(name, picks, margin, want):
    """picks (B, n_keep) of the CPU reference: members that change region inside the sub-steps / that stay in one, as the case states."""
    changing = [b for b in range(picks.shape[0]) if len(set(picks[b].tolist())) > 1]
    staying = [b for b in range(picks.shape[0]) if b not in changing]
    print('%s: CPU point sequences %s, least margin %.3e; members that change region %s, that stay %s' % (name, picks.tolist(), margin, changing,
                                                                                                         staying))
    assert margin >= cr.MARGIN
    assert (changing, staying) == want, (changing, staying)


def check_rollouts(name, plant, mname, dt_sim, x_in, U, X_loop, held):
    """rollout of the plant's dt_sim handle (staged) and of the plain twin's from x_in under U against the loop's plant states."""
    from sofacontrol_amd import _lib
    B, nk = U.shape[0], U.shape[1]
    twin = plain_twin(mname, dt_sim)
    ps, pp = _lib.tpwl_rollout_plan(plant.handle_for(dt_sim), nk, B), _lib.tpwl_rollout_plan(twin.handle_for(dt_sim), nk, B)
    assert (ps['staged'], ps['held']) == (True, held) and (pp['staged'], pp['held']) == (False, False), (ps, pp)
    assert np.isfinite(X_loop).all() and len({X_loop[b].tobytes() for b in range(B)}) == B and U.any()
    for what, model in (('staged', plant), ('plain', twin)):
        X, _ = model.rollout(x_in, U, dt_sim)
        assert X.shape == (B, nk + 1, x_in.shape[1])
        assert np.array_equal(X[:, 0], x_in), what
        assert np.array_equal(X[:, 1:], X_loop), '%s: %s rollout differs from the loop\'s plant states' % (name, what)


# (entry of cl_cases.ADVANCE, (members that change region, members that stay in one), held point table on the staged path)
GUSTO = [('g6-frac-10', ([0, 1, 2], []), True), ('m8-frac-10', ([0, 1, 2], []), True), ('r36-5-10', ([0], [1, 2]), False)]


@pytest.mark.parametrize('entry,want,held', GUSTO, ids=[g[0] for g in GUSTO])
def test_loop_advance_steps_the_plant_as_rollout_does(entry, want, held):
    import test_gusto_loop_gpu as tl
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    case = [c for c in cc.ADVANCE if c[0] == entry][0]
    name, mname, B, dt_sim, n_keep, gains, dist, seed = case
    case = (name, mname, B, dt_sim, n_keep, gains, False, seed)             # the case without its disturbance
    c = cc.advance_case(case)
    assert c['W'] is None
    tp, gm = tl.planner(mname)
    ref = cc.advance_reference(case, np.float64, H=np.asarray(tp.H))
    check_sequence(name, ref[3], ref[5], want)
    cl = ClosedLoopBatch(tl.plain_gusto(mname, B), tp, dt_sim, n_keep, K=c['K'])
    X, Z, U, ip, ig = cl._advance(c['xopt'], c['uopt'], c['x'], None)
    np.testing.assert_array_equal(ip, ref[3])
    check_rollouts(name, tp, mname, dt_sim, c['x'], U, X, held)


# (entry of rompc_loop_cases.ADVANCE, ...)
ROMPC = [('r36-5-10', ([], [0, 1, 2]), False), ('g6-frac-10', ([0, 1, 2], []), True), ('m8-frac-10', ([0, 1, 2], []), True)]


@pytest.mark.parametrize('entry,want,held', ROMPC, ids=[g[0] for g in ROMPC])
def test_rompc_advance_steps_the_plant_as_rollout_does(entry, want, held):
    import test_rompc_loop_gpu as trl
    case = [c for c in rc.ADVANCE if c[0] == entry][0]
    name, mname, B, ny, dt_sim, nk, dist, noise, with_H, mode, seed = case
    assert mode == 'sim'                                                    # the plant is set: X is the stepped plant's
    case = (name + '-step', mname, B, ny, dt_sim, nk, False, noise, with_H, mode, seed)         # without its disturbance, under a name of its own
    c = rc.advance_case(case)
    assert c['W'] is None and c['X_plant'] is None
    ref = rc.advance_reference(case, np.float64)
    check_sequence(name, ref['picks'], ref['margin'], want)
    cl = trl.advance_loop(case)
    got = cl._advance(c['xopt'], c['uopt'], c['x'], c['x_hat'], W=None, V=c['V'])
    check_rollouts(name, trl.plant(mname, mode), mname, dt_sim, c['x'], got['U'], got['X'], held)
