"""CPU: the input conditions of the closed-loop iLQR cases (tests/ilqr_loop_cases.py) under the statement of tests/ilqr_loop_reference.py
-- for every case the float64 statement stays within E_ORACLE_MAX of the long-double one, picks the same points, and no point search
comes within MARGIN of a second point -- and the statement's own properties: the row table, the held input, the idle tail."""
import numpy as np
import pytest

import cl_cases as cc
import ilqr_loop_cases as ic
import ilqr_loop_reference as ir


@pytest.mark.parametrize('case', ic.ADVANCE, ids=ic.IDS)
def test_advance_cases_meet_their_input_conditions(case):
    ref, e_oracle = ic.advance_measured(case)
    print('%s: e_oracle %.3e, least margin %.3e' % (case[0], e_oracle, ref[4]))
    assert e_oracle <= ir.E_ORACLE_MAX
    assert ref[4] >= ir.MARGIN
    assert np.isfinite(np.asarray(ref[0], dtype=np.float64)).all()


@pytest.mark.parametrize('cs', ic.OBSERVED, ids=ic.OBS_IDS)
def test_observed_cases_meet_their_input_conditions(cs):
    ref, e_oracle = ic.observed_measured(cs)
    print('%s: e_oracle %.3e, least margin %.3e' % (cs[0], e_oracle, ref['margin']))
    assert e_oracle <= ir.E_ORACLE_MAX
    assert ref['margin'] >= ir.MARGIN


@pytest.mark.parametrize('tag', ['full', 'ekf'])
def test_statement_reproduces_the_references_traces(tag):
    """tests/golden/g25_ilqr_loop.npz: the reference's tpwl.controllers.ilqr closed on its own TPWL model through evaluate, with the
    FullStateObserver and with a DiscreteEKFObserver.  The float64 statement fed the golden's policy gives the golden's u, plant states
    and beliefs within tolerance(e_oracle)."""
    g = ic.g25()
    ref, e_oracle = ic.g25_measured(tag)
    f64, gold = ic.g25_statement(tag, np.float64), ic.g25_golden(tag)
    print('g25 %s: e_oracle %.3e, least margin %.3e, tolerance %.3e' % (tag, e_oracle, ref['margin'], ir.tolerance(e_oracle)))
    assert e_oracle <= ir.E_ORACLE_MAX and ref['margin'] >= ir.MARGIN
    for k in ('U', 'X', 'Xhat'):
        e = ir.err(f64[k], gold[k])
        print('g25 %s %s: float64 statement against the golden %.3e' % (tag, k, e))
        assert gold[k].shape == f64[k].shape
        assert e <= ir.tolerance(e_oracle), k
    # what the trace covers: rows 3, 6, 7 read 2, 5, 6; controller step 13 (t_step = 0.65 > final_time) is idle with a non-zero u0
    rows = g['rows']
    assert [int(rows[j]) for j in (3, 6, 7, 12, 13)] == [2, 5, 6, 11, -1]
    assert g['u0'].any() and (g[tag + '_u'][65:] == g['u0']).all() and not (g[tag + '_u'][64] == g['u0']).all()
    if tag == 'full':
        np.testing.assert_array_equal(g['full_x_hat'], g['full_x'][:-1])
    else:
        assert np.abs(g['ekf_x_hat'] - g['ekf_x'][:-1]).max() > 1e-6


def test_members_of_a_case_are_distinct_and_visit_more_than_one_region():
    c = ic.advance_case(ic.ADVANCE[4])
    for k in ('xbar', 'ubar', 'K', 'x'):
        flat = c[k].reshape(c[k].shape[0], -1)
        assert len(np.unique(flat, axis=0)) == flat.shape[0], k
    picks = ic.advance_measured(ic.ADVANCE[1])[0][3]
    assert len(np.unique(picks)) >= 2


def test_row_quirk_held_input_and_idle_tail_of_the_statement():
    """g6-r5-tail: controller steps 3, 6, 7 read rows 2, 5, 6; the input changes only where a controller step fires; from controller step
    13 on (row 13 >= N = 12) the input is the non-zero u0."""
    case = ic.ADVANCE[1]
    c = ic.advance_case(case)
    rows = c['rows']
    assert [int(rows[j]) for j in (3, 6, 7)] == [2, 5, 6] and rows[12] == 11 and rows[13] == -1
    U = np.asarray(ic.advance_measured(case)[0][1], dtype=np.float64)
    for s in range(case[5]):
        if s % 5:
            np.testing.assert_array_equal(U[:, s], U[:, s - 1])
    assert c['u0'].any()
    np.testing.assert_array_equal(U[:, 65:], np.broadcast_to(c['u0'], U[:, 65:].shape))
    assert not np.array_equal(U[0, 60], c['u0'])
    # a row read twice: the law at another state
    assert not np.array_equal(U[:, 10], U[:, 15])


def test_split_advance_of_the_statement_equals_the_whole():
    case = ic.ADVANCE[1]
    c = ic.advance_case(case)
    plant, H = cc.table_dict('g6', 0.01), cc.model('g6')['H']
    b = 1
    args = (plant, H, c['xbar'][b], c['ubar'][b], c['K'][b], c['rows'], 5, c['u0'])
    X, U, Z, ip, _ = ir.advance(*args, c['x'][b], c['u0'], 20, 0, c['W'][:20, b], np.float64)
    X1, U1, _, _, _ = ir.advance(*args, c['x'][b], c['u0'], 7, 0, c['W'][:7, b], np.float64)
    X2, U2, _, _, _ = ir.advance(*args, X1[-1], U1[-1], 13, 7, c['W'][7:20, b], np.float64)
    np.testing.assert_array_equal(np.concatenate((X1, X2)), X)
    np.testing.assert_array_equal(np.concatenate((U1, U2)), U)
