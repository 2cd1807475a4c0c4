"""What the families of scenario_families.py exist to reach, asserted on the CPU oracle's own runs: an edit of a model must not
lose its reach silently.  test_hip_param_sets_shapes.py compares the GPU with exactly these runs.  Every (set, seed) pair of every
family must finish with the oracle's return code 0: no replicate may be left out of a comparison."""
import numpy as np
import pytest

import scenario_families as fam
from test_hip_param_sets import SEEDS, reference


@pytest.mark.parametrize("P", fam.WIDE_P)
def test_wide(oracle_mod, P):
    want = fam.reference_wide(oracle_mod, P)
    assert len(want) == 3 and all(len(w) == len(SEEDS) for w in want)
    a, b, c = ([w.simulation for w in ws] for ws in want)
    for m in a + b + c:
        assert m.events.ptr == fam.WIDE_EVENTS and m.popNum == P
    # set 0 alone cannot switch a lockdown: the engine's log is sized by the scan over the other sets
    assert all(m.swapLockdown == 0 and len(m.loc.states) == 0 for m in a)
    assert not fam.can_switch(a[0]) and not fam.can_switch(fam.wide(P)[0].simulation)
    for ms in (b, c):
        assert fam.can_switch(ms[0])
        for m in ms:
            assert m.swapLockdown > 0 and max(m.loc.populationsId) >= P - 6
    assert any(m.good_attempt > 1 for m in a + b + c)
    assert any(m.good_attempt > 1 and m.swapLockdown > 0 for m in b + c)   # a Restart in a set whose lockdowns switch
    if P > 64:   # the second tile of populations is occupied at the end, under every set
        for ms in (a, b, c):
            assert sum(m.infectious[64:].sum() > 0 for m in ms) >= 3


def test_long_lists(oracle_mod):
    base, scen = fam.long_lists(oracle_mod)
    start = fam.list_lengths(base.simulation)
    assert base.simulation.events.ptr == fam.LONG_WARM and base.simulation.susNum == 3
    assert start.max() > 64 and base.simulation.lockdownON.any()
    rows = [fam.class_rows(s) for s in scen]
    assert len(set(rows)) == 3 and rows[1] == max(rows)
    want = fam.reference_long_lists(oracle_mod)
    assert len(want) == 3 and all(len(w) == len(fam.LONG_SEEDS) for w in want)
    ends = []
    for g, ws in enumerate(want):
        for w in ws:
            m = w.simulation
            assert m.events.ptr == fam.LONG_WARM + fam.LONG_EVENTS, g
            assert np.array_equal(m.events.as_array()[:, :fam.LONG_WARM], base.simulation.events.as_array()[:, :fam.LONG_WARM])
            ends.append(fam.list_lengths(m))
    ends = np.array(ends)
    assert ends.max() > 128
    assert ((start <= 64) & (ends > 64)).any()    # a list that grows across a tile border during the run
    for g in range(3):                            # ... and lists of two and of three tiles under every set
        assert (ends[3 * g:3 * g + 3] > 128).any() and ((ends[3 * g:3 * g + 3] > 64) & (ends[3 * g:3 * g + 3] <= 128)).any(), g


def test_recombinant(oracle_mod):
    base, scen = fam.recombinant()
    assert base.simulation.recombination > 0
    want = fam.reference_recombinant(oracle_mod)
    assert len(want) == 3 and all(len(w) == len(fam.RECOMB_SEEDS) for w in want)
    for g, ws in enumerate(want):
        ms = [w.simulation for w in ws]
        assert all(m.events.ptr == fam.RECOMB_EVENTS and len(m.rec.idevents) > 0 for m in ms), g
        assert any(m.good_attempt > 1 for m in ms), g
    assert fam.class_rows(scen[0]) != fam.class_rows(scen[1])


def test_one_group(oracle_mod):
    base, scen = fam.one_group()
    m0 = base.simulation
    assert (m0.susNum, m0.popNum, m0.hapNum) == (1, 16, 1024)
    rows = [fam.class_rows(s) for s in scen]
    assert len(set(rows)) == 3                                        # per-haplotype rates differ: other class numbers per set
    assert [fam.can_switch(s.simulation) for s in scen] == [False, True, True]
    assert not np.array_equal(scen[1].simulation.startLD, scen[2].simulation.startLD)
    want = fam.reference_one_group(oracle_mod)
    assert len(want) == 3 and all(len(w) == len(fam.ONE_GROUP_SEEDS) for w in want)
    ms = [[w.simulation for w in ws] for ws in want]
    for g in range(3):
        assert all(m.events.ptr == fam.ONE_GROUP_EVENTS for m in ms[g]), g
        assert all(m.mCounter > 0 and m.migPlus > 0 for m in ms[g]), g
    assert all(m.swapLockdown == 0 for m in ms[0]) and all(m.swapLockdown > 0 for m in ms[1] + ms[2])
    assert any(m.good_attempt > 1 for m in ms[1]) and any(m.good_attempt > 1 for m in ms[2])
    assert max(fam.list_lengths(m).max() for m in ms[1]) > 128        # lists of three tiles under B, of one under A and C
    assert max(fam.list_lengths(m).max() for m in ms[0] + ms[2]) <= 64


def test_many_sets(oracle_mod):
    _, scen = fam.many_sets()
    assert len(scen) == fam.MANY_G == len(fam.MANY_SEEDS)
    assert sorted(fam.MANY_OF) == list(range(fam.MANY_G)) and (np.diff(fam.MANY_OF) < 0).all()   # one set per replicate, not in order
    assert len({(s.simulation.bRate[0], tuple(s.simulation.dRate)) for s in scen}) == fam.MANY_G
    want = [w.simulation for w in fam.reference_many_sets(oracle_mod)]
    assert len(want) == fam.MANY_G
    assert len({m.events.ptr for m in want}) > 10
    assert any(m.events.ptr == fam.MANY_EVENTS for m in want) and any(0 < m.events.ptr < fam.MANY_EVENTS for m in want)
    assert any(m.good_attempt > 1 for m in want)


def test_unused_largest(oracle_mod):
    _, scen = fam.unused_largest()
    rows = [fam.class_rows(s) for s in scen]
    assert len(scen) == 5 and rows[1] > max(rows[:1] + rows[2:])     # the set with the most classes ...
    assert 1 not in fam.UNUSED_OF and set(fam.UNUSED_OF) == {0, 2, 3, 4}   # ... is run by nobody
    assert len(fam.UNUSED_OF) == len(fam.UNUSED_SEEDS) == 8
    assert len({(int(g), int(s)) for g, s in zip(fam.UNUSED_OF, fam.UNUSED_SEEDS)}) == 8
    want = reference(oracle_mod)     # (oracle_run asserts return code 0 for each)
    used = [want[fam.UNUSED_SOURCE[g]][k % 4].simulation for k, g in enumerate(fam.UNUSED_OF)]
    assert any(m.events.ptr > 0 for m in used)


@pytest.mark.parametrize("stop", sorted(fam.STOPS))
def test_stops(oracle_mod, stop):
    want = fam.reference_stop(oracle_mod, stop)
    assert len(want) == 4 and all(len(w) == len(SEEDS) for w in want)
    assert all(rc == 0 for ws in want for _, rc in ws)
    ms = [w.simulation for ws in want for w, _ in ws]
    assert all(m.events.ptr < fam.STOP_EVENTS for m in ms)           # nobody runs into the event count
    assert len({m.events.ptr for m in ms}) >= 8                       # every replicate stops at its own event
    assert sum(m.events.ptr == 0 and m.good_attempt == 0 for m in ms) >= 1   # every attempt failed: 0 events
    if stop == "sample":
        limit = fam.STOPS[stop]["sample_size"]
        hit = [m for m in ms if m.sCounter > limit]
        early = [m for m in ms if m.events.ptr > 0 and m.sCounter <= limit]
        assert len(hit) >= 4 and all(m.globalInfectious > 0 for m in hit)
    else:
        limit = fam.STOPS[stop]["epidemic_time"]
        hit = [m for m in ms if m.currentTime > limit]
        early = [m for m in ms if m.events.ptr > 0 and m.currentTime <= limit]
        assert len(hit) >= 4 and all(m.currentTime < limit + 1.0 for m in hit)
    assert early and all(m.globalInfectious == 0 for m in early)      # an extinction before the limit
