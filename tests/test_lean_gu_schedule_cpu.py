"""CPU: the (column, chain) schedule of y = G u in the half-size lean kernel (csrc/locp_lean.h: gu_rounds and the functions next to it,
ql::g_times_tasks), listed on the host by slean_gu_schedule from the functions the device code calls.  The product is bit-identical to the
thread-per-column loop only if every chain of every column receives exactly its own terms in its own order -- chain c of column i the
stages c, c + 4, .. <= i / 2 of the inputs in turn -- and the four chains of a column meet in one quad of lanes; a wrong table there is a
wrong number in every interior-point iteration, or a read outside the packed block.  The definitions the checks use (the triangle, the
packed offsets, the generators' layout) are stated here on their own."""
import functools

import numpy as np
import pytest

NF, M = 50, 4
NP = 2 * NF
ROUND, INPUT, STEP, COLUMN, CHAIN, STAGE, FLAGS, PACKED, TOEPLITZ = range(9)
SPARE, STORES = 1, 2
SETS = (128, 256)            # the Newton front's two waves, the whole half-size workgroup


@functools.lru_cache(maxsize=None)
def listing(set_size):
    """{(wave, lane): steps x 9} from the library; asked once per set size and never changed"""
    from sofacontrol_amd import _lib
    assert (_lib.GU_SPARE, _lib.GU_STORES) == (SPARE, STORES)
    return _lib.lean_gu_schedule(NF, M, set_size)


def goff(j):
    """start of stage j in the packed G^T: the stages before it hold M rows of NP - 2 j' entries each"""
    return sum(M * (NP - 2 * jj) for jj in range(j))


def packed_index(j, b, i):
    """element i >= 2 j of row (j, b)"""
    return goff(j) + b * (NP - 2 * j) + (i - 2 * j)


def verify(sched, set_size):
    """every property the kernel's bit-identity and its bounds rest on; raises AssertionError"""
    nw, GR = set_size // 64, set_size // 128
    tasks, stores = {}, {}
    for wave in range(nw):
        inputs = list(range(wave // 2, M, GR))
        shape0 = None
        for lane in range(64):
            st = np.asarray(sched[(wave, lane)])
            # the lanes of a wave walk in lockstep: same rounds, inputs and steps, in the same order
            shape = st[:, [ROUND, INPUT, STEP]].tolist()
            shape0 = shape if shape0 is None else shape0
            assert shape == shape0, (wave, lane)
            rounds = list(dict.fromkeys(st[:, ROUND].tolist()))
            for r in rounds:
                rs = st[st[:, ROUND] == r]
                nsteps = int(rs[:, STEP].max()) + 1
                # inside a round: the inputs of the wave's class in turn, the steps 0 .. nsteps - 1 inside each
                assert rs[:, [INPUT, STEP]].tolist() == [[b, s] for b in inputs for s in range(nsteps)], (wave, lane, r)
                assert len(set(rs[:, COLUMN].tolist())) == 1 and len(set(rs[:, CHAIN].tolist())) == 1 and len(set(rs[:, FLAGS].tolist())) == 1
                i, c, flags = int(rs[0, COLUMN]), int(rs[0, CHAIN]), int(rs[0, FLAGS])
                assert 0 <= i < NP and 0 <= c < 4
                for b in inputs:
                    bs = rs[rs[:, INPUT] == b]
                    live = bs[bs[:, STAGE] >= 0]
                    # the unmasked steps are exactly the chain's stages, ascending
                    assert live[:, STAGE].tolist() == list(range(c, i // 2 + 1, 4)), (wave, lane, r, b)
                    # no step before the round's last two is masked
                    assert (bs[bs[:, STAGE] < 0][:, STEP] >= nsteps - 2).all(), (wave, lane, r, b)
                    for e in bs:
                        j = int(e[STAGE])
                        # no read leaves the packed block / the generators, masked and spare lanes included
                        assert 0 <= e[PACKED] < goff(NF) and 0 <= e[TOEPLITZ] < M * NP, (wave, lane, e.tolist())
                        if j >= 0:
                            assert e[PACKED] == packed_index(j, b, i) and e[TOEPLITZ] == b * NP + i - 2 * j, (wave, lane, e.tolist())
                    if not flags & SPARE:
                        assert (i, c, b) not in tasks, 'task (column %d, chain %d, input %d) occurs twice' % (i, c, b)
                        tasks[(i, c, b)] = (wave, r, lane >> 2)
                    if flags & STORES:
                        assert not flags & SPARE and (i, b) not in stores
                        stores[(i, b)] = (wave, r, lane >> 2)
    # every (column < NP, chain) task occurs (exactly once: above), for every input
    assert set(tasks) == {(i, c, b) for i in range(NP) for c in range(4) for b in range(M)}
    for i in range(NP):
        for b in range(M):
            # the four tasks of a column share a quad, and one of its lanes stores the column's sum
            quads = {tasks[(i, c, b)] for c in range(4)}
            assert len(quads) == 1 and stores.get((i, b)) in quads, (i, b, quads)


@pytest.mark.parametrize('set_size', SETS)
def test_schedule(set_size):
    verify(listing(set_size), set_size)


@pytest.mark.parametrize('set_size', SETS)
def test_rounds_and_their_waves(set_size):
    """NP = 100: rounds of 8, 16 x 5 and 12 columns in 1, 3, .. 13 steps (49 per input), dealt longest first to the two waves of an input
    class: 25 and 24 steps per input, against the 50 and 32 stage slots of a thread per column.  A wave runs its rounds longest first,
    the inputs of its class in turn inside a round"""
    sched = listing(set_size)
    for wave in range(set_size // 64):
        st = sched[(wave, 0)]
        inputs = list(range(wave // 2, M, set_size // 128))
        first = st[st[:, INPUT] == st[0, INPUT]]
        rounds = {}
        for r in first[:, ROUND].tolist():
            rounds[r] = rounds.get(r, 0) + 1
        assert rounds == ({6: 13, 3: 7, 2: 5} if wave % 2 == 0 else {5: 11, 4: 9, 1: 3, 0: 1}), (wave, rounds)
        blocks = list(dict.fromkeys(map(tuple, st[:, [ROUND, INPUT]].tolist())))
        assert blocks == [(r, b) for r in sorted(rounds, reverse=True) for b in inputs], (wave, blocks)
        cols = {r: sorted({int(sched[(wave, lane)][sched[(wave, lane)][:, ROUND] == r][0, COLUMN]) for lane in range(64)}) for r in rounds}
        for r, cs in cols.items():
            lo = 0 if r == 0 else 16 * r - 8
            assert cs == list(range(lo, min(NP, 16 * r + 8))), (r, cs)


def test_the_checks_see_a_dropped_first_step():
    """the checks above can fail: the same schedule without the first step of one lane"""
    sched = dict(listing(128))
    sched[(0, 5)] = sched[(0, 5)][1:]
    with pytest.raises(AssertionError):
        verify(sched, 128)
    # ... and with a lane's first step given to the stage behind it (the lockstep shape intact)
    sched = dict(listing(128))
    st = sched[(1, 9)].copy()
    st[0, STAGE] += 4
    sched[(1, 9)] = st
    with pytest.raises(AssertionError):
        verify(sched, 128)
