"""CPU: the counter protocol of the lean kernels' tile factorisation under every row roster (csrc/locp_lean.h: tile_cholesky_set, roster_nwk
and the targets next to it), replayed on the host before it runs on a GPU -- a wrong target there is a workgroup that
spins for good, not a wrong number.  slean_roster_replay lists, for each of the four waves, the events the device code's own roster
functions give; a small scheduler here runs the four lists under many interleavings and asserts that every one terminates, that the
counters end at the targets the roster's definition gives, that every tile receives exactly the operations of the sequential tile Cholesky
in ascending row order, and that every access to a tile is ordered behind the conflicting accesses before it by a signal / wait pair
(vector clocks along the counters; a wait for the value v acquires the first v arrivals only -- the least a poll can have seen).
The same scheduler with a cost per event predicts the length of the split stretch per code (printed; costs from
profiles/r09_lean_half_phase_clocks_after.json, case c2_N50_half)."""
import functools
import random

import pytest

WRITES = ('chol', 'panel', 'update')


@functools.lru_cache(maxsize=None)
def lists(KT, code, nwk0=1):
    """(code in effect, the four event lists) from the library; asked once per case and never changed"""
    from sofacontrol_amd import _lib
    return _lib.lean_roster_replay(KT, code, nwk0)


def legal_codes(KT):
    return [0] + [s * k for k in range(1, KT - 1) for s in (1, -1)]


def nwk(code, nwk0, J):
    """the roster's definition, stated here on its own: workers of tile row J"""
    if code == 0:
        return nwk0
    return 3 if (J >= code if code > 0 else J < -code) else 1


def final_counters(KT, code, nwk0):
    rows = range(KT - 1)
    return [sum(nwk(code, nwk0, J) for J in rows), KT, sum(nwk(code, nwk0, J) + 1 for J in rows), 2 * max(0, KT - 2)]


def sequential_ops(KT):
    """tile (I, K), I <= K, of the right-looking tile Cholesky: the updates of the rows J < I in ascending order, then its own row's operation"""
    return {(I, K): [('update', J) for J in range(I)] + [('chol' if I == K else 'panel', I)] for I in range(KT) for K in range(I, KT)}


class Deadlock(AssertionError):
    pass


def run(waves, pick):
    """Run the four event lists; pick(runnable, step) chooses the wave that takes the next event.  Returns (counters, ops per tile)."""
    nw = len(waves)
    pos = [0] * nw
    vc = [[0] * nw for _ in range(nw)]
    counters = [0, 0, 0, 0]
    arrivals = [[] for _ in range(4)]                  # per counter: the vector clock of each arrival, in order
    last_write = {}                                    # tile -> (wave, its clock at the write)
    last_reads = {}                                    # tile -> {wave: its clock at its last read since the last write}
    ops = {}
    step = 0

    def runnable(w):
        if pos[w] >= len(waves[w]):
            return False
        kind, a, b, _ = waves[w][pos[w]]
        return kind != 'wait' or counters[a] >= b

    def ordered_behind(w, other, clock, what, tile):
        assert other == w or vc[w][other] >= clock, 'wave %d: %s of tile %r is not ordered behind wave %d' % (w, what, tile, other)

    while True:
        ready = [w for w in range(nw) if runnable(w)]
        if not ready:
            if all(pos[w] >= len(waves[w]) for w in range(nw)):
                return counters, ops
            raise Deadlock('no wave can go on: %r' % [(w, waves[w][pos[w]]) for w in range(nw) if pos[w] < len(waves[w])])
        w = pick(ready, step)
        step += 1
        kind, a, b, c = waves[w][pos[w]]
        pos[w] += 1
        vc[w][w] += 1
        if kind == 'wait':
            for seen in arrivals[a][:b]:
                vc[w] = [max(x, y) for x, y in zip(vc[w], seen)]
        elif kind == 'signal':
            counters[a] += 1
            arrivals[a].append(list(vc[w]))
        elif kind == 'read':
            if (a, b) in last_write:
                ordered_behind(w, *last_write[(a, b)], 'read', (a, b))
            last_reads.setdefault((a, b), {})[w] = vc[w][w]
        elif kind in WRITES:
            if (a, b) in last_write:
                ordered_behind(w, *last_write[(a, b)], 'write', (a, b))
            for r, clock in last_reads.get((a, b), {}).items():
                ordered_behind(w, r, clock, 'write after read', (a, b))
            last_write[(a, b)] = (w, vc[w][w])
            last_reads[(a, b)] = {}
            ops.setdefault((a, b), []).append((kind, c))


def by_priority(order):
    return lambda ready, step: min(ready, key=order.index)


def slow_set(slow):
    """the waves of `slow` take an event only when no other wave can, or every 64th step"""
    def pick(ready, step):
        fast = [w for w in ready if w not in slow]
        return ready[0] if (not fast or (step % 64 == 63 and ready[0] in slow)) else fast[0]
    return pick


def check(KT, code, nwk0, pick):
    eff, waves = lists(KT, code, nwk0)
    assert eff == code
    counters, ops = run(waves, pick)
    assert counters == final_counters(KT, code, nwk0), (KT, code, counters)
    assert ops == sequential_ops(KT), (KT, code)


@pytest.mark.parametrize('KT', range(2, 9))
def test_every_interleaving_terminates_with_the_sequential_factorisation(KT):
    """half-size workgroup (waves 2, 3 run the front as well), every legal code: 200 seeded random interleavings and three extremes --
    the factorising set as slow as possible, the front set as slow as possible, waves 2 and 3 arriving last"""
    for code in legal_codes(KT):
        for seed in range(200):
            rng = random.Random(1000 * KT + 7 * seed + code)
            check(KT, code, 1, lambda ready, step: rng.choice(ready))
        check(KT, code, 1, slow_set((0, 1)))
        check(KT, code, 1, slow_set((2, 3)))
        check(KT, code, 1, by_priority([0, 1, 2, 3]))
        check(KT, code, 1, by_priority([3, 2, 1, 0]))


@pytest.mark.parametrize('KT', range(2, 9))
def test_uniform_three_workers_of_the_full_size_set(KT):
    """the default of every other caller: three workers in every row, no roster"""
    for seed in range(50):
        rng = random.Random(seed)
        check(KT, 0, 3, lambda ready, step: rng.choice(ready))
    check(KT, 0, 3, by_priority([3, 2, 1, 0]))
    check(KT, 0, 3, by_priority([0, 1, 2, 3]))


def test_the_scheduler_sees_a_wrong_target():
    """the checks above can fail: code -1 at KT = 7 with wave 1's Ftrail target in front of row 1 (3: the three workers of row 0) one too
    high is a wave that waits for good; one too low lets it touch tiles that waves 2 and 3 are still updating"""
    waves = lists(7, -1)[1]
    at = waves[1].index(('wait', 0, 3, 0))
    tampered = lambda v: [list(w) if i != 1 else w[:at] + [('wait', 0, v, 0)] + w[at + 1:] for i, w in enumerate(waves)]
    with pytest.raises(Deadlock):
        run(tampered(4), by_priority([0, 1, 2, 3]))
    for pick in (slow_set((2, 3)), by_priority([1, 0, 2, 3])):
        with pytest.raises(AssertionError) as err:
            run(tampered(2), pick)
        assert not isinstance(err.value, Deadlock) and 'not ordered behind' in str(err.value)


def test_code_0_is_the_schedule_before_rosters():
    """KT = 7: wave 1 has 15 panel tiles and 50 updates, the chain 6 and 6; waves 2 and 3 run the front and nothing else"""
    eff, waves = lists(7, 0)
    count = lambda w, kind: sum(1 for e in waves[w] if e[0] == kind)
    assert eff == 0
    assert (count(1, 'panel'), count(1, 'update')) == (15, 50)
    assert (count(0, 'panel'), count(0, 'update'), count(0, 'chol')) == (6, 6, 7)
    assert waves[2] == [('front', 0, 0, 0)] and waves[3] == [('front', 0, 0, 0)]
    # every wait of wave 1 asks for what the uniform rule asks: Ftrail >= J, Frinv >= J + 1, Fpanel >= 2 (J + 1)
    waits = [e[1:3] for e in waves[1] if e[0] == 'wait']
    assert waits == [x for J in range(6) for x in ((1, J + 1), (0, J), (2, 2 * (J + 1)))]


def test_a_code_outside_the_legal_range_counts_as_0():
    for KT, code in ((7, 6), (7, -6), (7, 100), (2, 1), (3, 2), (8, -7)):
        eff, waves = lists(KT, code)
        assert eff == 0 and waves == lists(KT, 0)[1], (KT, code)
    assert lists(7, 5, 3)[0] == 0                       # (the full-size set has no rosters)
    for code in (5, -5, 1, -1):
        assert lists(7, code)[0] == code


def test_roster_rows_of_waves_2_and_3():
    """+k: the front first, then the rows k .. KT - 2; -k: the rows 0 .. k - 1, then the front; a skipped row leaves no event"""
    for KT in range(3, 9):
        for code in legal_codes(KT)[1:]:
            k = abs(code)
            for w in (2, 3):
                ev = lists(KT, code)[1][w]
                front = [i for i, e in enumerate(ev) if e[0] == 'front']
                assert len(front) == 1
                assert front[0] == (0 if code > 0 else len(ev) - 1)
                rows = sorted({e[3] for e in ev if e[0] in WRITES})
                want = list(range(k, KT - 1)) if code > 0 else list(range(0, k))
                # (worker 2 has no tile in a row with a single trailing column: it still arrives on the row's counters)
                entered = [e[2] - 1 for e in ev if e[0] == 'wait' and e[1] == 1]
                assert entered == want and set(rows) <= set(want), (KT, code, w, rows, entered)


# ---- the same event lists with a cost per event: the predicted length of the split stretch
# clocks, c2_N50_half of profiles/r09_lean_half_phase_clocks_after.json per factorisation: the chain's factor 19.1 k / 7, panel 2.7 k / 6,
# update 3.1 k / 6, signals 3.1 k / 14; the front on two waves 34.3 k (profiles/r10_lean_half_phase_clocks_0.json: split.front / 39 fills);
# a worker's tile operation 0.76 k: the one fitted figure, chosen so that code 0 gives the measured 60.2 k of split.factorisation
COSTS = {'chol': 2730, 'chain panel': 450, 'chain update': 520, 'signal': 220, 'tile': 760, 'front': 34300}


def predict(KT, code, costs=COSTS):
    """Event-driven replay: a wave's wait ends when the counter reaches its value.  Returns (stretch, chain end, the chain's waiting)."""
    _, waves = lists(KT, code)
    t = [0.0] * 4
    pos = [0] * 4
    times = [[] for _ in range(4)]                     # arrival times per counter
    chain_wait = 0.0
    while True:
        cand = []
        for w in range(4):
            if pos[w] < len(waves[w]):
                kind, a, b, _ = waves[w][pos[w]]
                if kind == 'wait' and len(times[a]) < b:
                    continue
                cand.append((max(t[w], sorted(times[a])[b - 1]) if kind == 'wait' and b > 0 else t[w], w))
        if not cand:
            break
        start, w = min(cand)
        kind = waves[w][pos[w]][0]
        pos[w] += 1
        if kind == 'wait':
            if w == 0:
                chain_wait += start - t[w]
            t[w] = start
        elif kind == 'signal':
            t[w] += costs['signal']
            times[waves[w][pos[w] - 1][1]].append(t[w])
        elif kind == 'read':
            pass
        elif kind == 'front':
            t[w] += costs['front']
        elif kind == 'chol':
            t[w] += costs['chol']
        else:
            t[w] += costs['chain ' + kind] if w == 0 else costs['tile']
    assert all(pos[w] == len(waves[w]) for w in range(4))
    return max(t), t[0], chain_wait


def test_predicted_stretch_per_code():
    """prints the table DESIGN section 39 quotes; asserts only what no cost can change: the stretch is never shorter than the chain's own
    work, nor than the front, and code 0 leaves all 65 worker tiles to wave 1"""
    own = 7 * COSTS['chol'] + 6 * (COSTS['chain panel'] + COSTS['chain update']) + 14 * COSTS['signal']
    print('\ncode  stretch  chain end  chain wait   (clocks, KT = 7; costs %r)' % (COSTS,))
    for code in sorted(legal_codes(7), key=lambda c: (c < 0, abs(c))):
        stretch, chain, wait = predict(7, code)
        print('%+4d  %7.0f  %9.0f  %10.0f' % (code, stretch, chain, wait))
        assert stretch >= chain >= own and stretch >= COSTS['front']
    assert predict(7, 0)[0] >= 65 * COSTS['tile']
