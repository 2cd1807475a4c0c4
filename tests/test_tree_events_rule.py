"""Tree events per interval (vgsim_amd/csrc/vgx_tree_events.h) against a pure-Python restatement of the rule's table
over the lineage records of test_lineages_rule's ``py_walk``.  ``_capi.replay_tree_events`` (the device's walk, observer and the host
tile walk compiled for the host) must give the restatement's block on the reference's direct genealogy fixtures and the random models
of test_hip_fuzz, for every grid and map of test_lineages_rule and tiles of 1, 7 and 64 records, and its signed sum must be the
lineages' block.  No GPU."""
import copy
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import load
from test_lineages_rule import GOLD, MOVE, MUT, SPLIT, TIP, _fuzz, cuts, grids, maps, py_lineages, py_walk

CHANNELS = ("samples", "coalescences", "mutations_within", "mutations_out", "mutations_in", "departures", "arrivals")
K = len(CHANNELS)
FUZZ = range(48)          # the random models test_lineages_rule walks


def py_tree_events(records, times, grid, variant_of, P, V):
    """counts [T + 1, P, V, 7] from the lineage records by the table of vgx_tree_events.h."""
    T = len(grid)
    cut = cuts(times, grid)
    out = np.zeros((T + 1, P, V, K), dtype=np.int64)
    H = len(variant_of)

    def cls(h):
        return int(variant_of[h]) if 0 <= h < H else -1
    for kind, hap, pop, nh, npop, e in records:
        i = sum(1 for c in cut if c <= e)   # cut[i - 1] <= e < cut[i]
        if not 0 <= pop < P:
            continue
        c, c2 = cls(hap), cls(nh)
        if kind == TIP and c >= 0:
            out[i, pop, c, 0] += 1
        elif kind == SPLIT and c >= 0:
            out[i, pop, c, 1] += 1
        elif kind == MUT:
            if c == c2 and c >= 0:
                out[i, pop, c, 2] += 1
            if c >= 0 and c2 != c:
                out[i, pop, c, 3] += 1
            if c2 >= 0 and c2 != c:
                out[i, pop, c2, 4] += 1
        elif kind == MOVE and c >= 0:
            out[i, pop, c, 5] += 1
            if 0 <= npop < P:
                out[i, npop, c, 6] += 1
    return out.astype(np.int32)


def net_of(counts):
    c = counts.astype(np.int64)
    return c[..., 1] - c[..., 0] + c[..., 4] - c[..., 3] + c[..., 6] - c[..., 5]


def lineages_of(counts):
    """(values [T, P, V], root [P, V]) as ``TreeEvents.lineages()`` sums them from one replicate's counts [T + 1, P, V, 7]."""
    net = net_of(counts)
    root = -net.sum(axis=0)
    return (root[None] + np.cumsum(net[:-1], axis=0)).astype(np.int32), root.astype(np.int32)


def check_chain(m, seed, what):
    from vgsim_amd import _capi
    n = int(m.events.ptr)
    times = m.events.times[:n].copy()
    P, H = int(m.popNum), int(m.hapNum)
    w = py_walk(m, seed)
    for grid in grids(times):
        for vo, V in maps(H):
            if 4 * K * P * V > 65536:   # (c3_s5_p16 with every haplotype its own class: 16 x 1024 x 7 cells) refused by the rule's LDS limit
                with pytest.raises(ValueError, match="x 7 channels need %d bytes of cells" % (4 * K * P * V)):
                    _capi.replay_tree_events(copy.deepcopy(m), seed, grid, vo, V)
                continue
            want = py_tree_events(w["records"], times, grid, vo, P, V)
            want_v, want_r = py_lineages(w["records"], times, grid, vo, P, V)
            for tile in (1, 7, 64):
                out = _capi.replay_tree_events(copy.deepcopy(m), seed, grid, vo, V, tile=tile)
                assert out["counts"].dtype == np.int32 and np.array_equal(out["counts"], want), "%s counts T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert out["records"] == len(w["records"]), what
                # the identity, cell by cell: the signed sum of the kinds is the lineages' block
                got_v, got_r = lineages_of(out["counts"])
                assert np.array_equal(got_v, want_v) and np.array_equal(got_r, want_r), "%s identity T=%d V=%d tile=%d" % (what, len(grid), V, tile)
            if V == H:
                assert int(want[..., 0].sum()) == int(m.sCounter) and int(want[..., 1].sum()) == int(m.sCounter) - 1, what


@pytest.mark.parametrize("k,path", list(enumerate(GOLD)), ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_tree_events_on_reference_chains(oracle_mod, k, path):
    meta, _ = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"]).simulation
    check_chain(m, 1000 + k, meta["case"])


@pytest.mark.parametrize("seed", FUZZ)
def test_tree_events_on_random_models(oracle_mod, seed):
    from vgsim_amd import _capi
    m, message = _fuzz(seed)
    if m is None:
        return   # the reference aborts on a zero weight: no chain
    if message is not None:   # the walk fails: the host pass's message
        t = m.events.times[:m.events.ptr]
        grid = np.array([float(t[len(t) // 2]) if len(t) else 0.5])
        with pytest.raises(ValueError) as got:
            _capi.replay_tree_events(copy.deepcopy(m), 1000 + seed, grid, np.arange(m.hapNum, dtype=np.int32), m.hapNum)
        assert str(got.value) == message
        return
    check_chain(m, 1000 + seed, "fuzz %d" % seed)


def test_every_channel_is_exercised(oracle_mod):
    """Not vacuous: over the reference chains above taken together (both maps) every channel counts something, and a chain has a
    between-class mutation under the three-class map.  The totals are the restatement's, which the hook equals chain by chain."""
    totals, between = np.zeros(K, dtype=np.int64), []
    for k, path in enumerate(GOLD):
        meta, _ = load(path)
        m = helpers.run_case_oracle(oracle_mod, meta["case"]).simulation
        times = m.events.times[:int(m.events.ptr)].copy()
        records = py_walk(m, 1000 + k)["records"]
        for vo, V in maps(int(m.hapNum)):
            per = py_tree_events(records, times, grids(times)[0], vo, int(m.popNum), V).sum(axis=(0, 1, 2), dtype=np.int64)
            totals += per
            if V == 3 and per[3] > 0:
                between.append(meta["case"])
    assert (totals > 0).all(), dict(zip(CHANNELS, totals.tolist()))
    assert between, "no chain with a between-class mutation under the three-class map"


def test_refusals(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "g9_short").simulation
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)

    def call(grid, vo, V):
        return _capi.replay_tree_events(copy.deepcopy(m), 1000, grid, vo, V)
    with pytest.raises(ValueError, match=r"vgx_test_tree_events: grid must increase strictly \(grid\[1\]\)"):
        call([0.5, 0.5], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tree_events: T = 0 must be at least 1"):
        call([], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tree_events: V = 0 must be at least 1"):
        call([0.5], np.full(H, -1, dtype=np.int32), 0)
    bad = ident.copy()
    bad[1] = H
    with pytest.raises(ValueError, match=r"vgx_test_tree_events: variant_of\[1\] = %d is outside \[-1, %d\)" % (H, H)):
        call([0.5], bad, H)
    V = 16384 // (7 * P) + 1   # 7 P V 4 bytes of cells just above 64 KiB, P V 4 bytes far below
    assert 4 * P * V <= 65536 < 28 * P * V
    with pytest.raises(ValueError, match=r"vgx_test_tree_events: %d populations x %d classes x 7 channels need %d bytes of cells, above the 65536 bytes of LDS"
                       % (P, V, 28 * P * V)):
        call([0.5], np.zeros(H, dtype=np.int32), V)
    out = call([0.5], np.zeros(H, dtype=np.int32), V - 1)   # the largest V that fits is taken
    assert out["counts"].shape == (2, P, V - 1, 7)
    m.sCounter = 1
    with pytest.raises(ValueError, match="Less than two cases were sampled"):
        call([0.5], ident, H)
