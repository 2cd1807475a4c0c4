"""Tree events per interval of TAU chains (vgx_test_tau_tree_events) against the table of vgx_tree_events.h restated in
Python (test_tree_events_rule's ``py_tree_events``) over the lineage records of test_tau_lineages_rule's ``py_tau_walk``: on the chains
where that file asserts the walk (the reference's tau genealogy fixtures, continued chains, the random models), for every grid and
map, tiles of 1, 7 and 64 records, rows split and shuffled, and with the identity that gives the lineages' block.  No GPU."""
import copy
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import load
from test_lineages_rule import grids, maps, py_lineages
from test_tau_genealogy_walk import FUZZ, GOLD, decanonicalised, trailing_steps
from test_tau_lineages_rule import MULTI, _fuzz, py_tau_walk
from test_tree_events_rule import K, lineages_of, py_tree_events


def check_chain(m, seed, raw, what, scramble_seed=5):
    """The block of the hook on one chain and generator start against the restatement; the walk's message on a chain whose walk fails.
    Returns whether the chain is healthy."""
    from vgsim_amd import _capi
    n = int(m.events.ptr)
    times = m.events.times[:n].copy()
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)
    try:
        g = _capi.tau_genealogy_walk(copy.deepcopy(m), seed, rng_raw=raw)
    except RuntimeError as e:
        with pytest.raises(ValueError) as got:
            _capi.replay_tree_events(copy.deepcopy(m), seed, [float(times[n // 2])], ident, H, rng_raw=raw, tau=True)
        assert str(got.value) == str(e), what
        return False
    w = py_tau_walk(m, seed, raw)
    raw_rows = decanonicalised(m, scramble_seed)
    for grid in grids(times):
        for vo, V in maps(H):
            if 4 * K * P * V > 65536:
                with pytest.raises(ValueError, match="x 7 channels need %d bytes of cells" % (4 * K * P * V)):
                    _capi.replay_tree_events(copy.deepcopy(m), seed, grid, vo, V, rng_raw=raw, tau=True)
                continue
            want = py_tree_events(w["records"], times, grid, vo, P, V)
            want_v, want_r = py_lineages(w["records"], times, grid, vo, P, V)
            for tile in (1, 7, 64):
                out = _capi.replay_tree_events(copy.deepcopy(m), seed, grid, vo, V, tile=tile, rng_raw=raw, tau=True)
                assert out["counts"].dtype == np.int32 and np.array_equal(out["counts"], want), "%s counts T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert out["records"] == len(w["records"]) and out["rng_raw"] == g["rng_raw"] and out["nodes_used"] == g["nodes_used"], what
                got_v, got_r = lineages_of(out["counts"])
                assert np.array_equal(got_v, want_v) and np.array_equal(got_r, want_r), "%s identity T=%d V=%d tile=%d" % (what, len(grid), V, tile)
            # the order and granularity of the trailing steps' rows change nothing
            out = _capi.replay_tree_events(copy.deepcopy(raw_rows), seed, grid, vo, V, tile=7, rng_raw=raw, tau=True)
            assert np.array_equal(out["counts"], want) and out["rng_raw"] == g["rng_raw"], what + " split and shuffled rows"
            if V == H:
                assert int(want[..., 0].sum()) == int(m.sCounter) and int(want[..., 1].sum()) == int(m.sCounter) - 1, what
    return True


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_tree_events_on_reference_tau_chains(oracle_mod, path):
    meta, _ = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"], record_multievents=True).simulation
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    assert trailing_steps(m) < m.events.ptr
    raw = tuple(st.rng_final) + (0, 0) if meta["genealogy_seed"] is None else None
    assert check_chain(m, meta["genealogy_seed"], raw, meta["case"])


def test_continued_chains(oracle_mod):
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    assert 0 < trailing_steps(m) < m.events.ptr
    assert check_chain(m, 31, None, "tau_d")
    m = helpers.run_case_oracle(oracle_mod, "tau_then_direct", record_multievents=True).simulation
    assert oracle_mod.run_tau(m, 25, 10 ** 12, -1, 200, record_multievents=True) == 0
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    first = trailing_steps(m)
    t = m.events.types[:first]
    assert first < m.events.ptr and (t == MULTI).any() and t[0] != MULTI and t[-1] != MULTI   # rows of an earlier tau call in the prefix
    for seed, raw in ((32, None), (None, tuple(st.rng_final) + (1, 0x9E3779B9))):
        assert check_chain(m, seed, raw, "tau_then_direct + tau")


@pytest.mark.parametrize("seed", FUZZ)
def test_tree_events_on_random_models(oracle_mod, seed):
    m, final = _fuzz(seed)
    for gseed, raw in ((None, final), (1000 + seed, None)):
        check_chain(m, gseed, raw, "fuzz %d seed %r" % (seed, gseed), scramble_seed=seed)


def test_a_grid_point_at_a_step_time_has_the_step_applied(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    n, first = int(m.events.ptr), trailing_steps(m)
    t = m.events.times[:n]
    H = int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)
    w = py_tau_walk(m, 31)
    steps_with_records = sorted({r[5] for r in w["records"] if first <= r[5] < n - 1 and t[r[5] - 1] < t[r[5]] < t[r[5] + 1]})
    assert steps_with_records
    k = steps_with_records[len(steps_with_records) // 2]
    in_step = sum(1 for r in w["records"] if r[5] == k)

    def call(point):
        return _capi.replay_tree_events(copy.deepcopy(m), 31, [point], ident, H, tau=True)["counts"]
    at, after, before = call(float(t[k])), call(0.5 * (float(t[k]) + float(t[k + 1]))), call(0.5 * (float(t[k - 1]) + float(t[k])))
    # the whole step lies in interval 0 (up to the grid time) when the grid time is the step's time, in the tail when it is earlier
    assert np.array_equal(at, after) and not np.array_equal(at, before)
    assert np.array_equal(at, py_tree_events(w["records"], t, [float(t[k])], ident, int(m.popNum), H))
    moved = (before[1].astype(np.int64) - at[1]).sum()
    assert moved > 0 and (before[1] >= at[1]).all() and np.array_equal(before.sum(axis=0), at.sum(axis=0))
    assert moved >= in_step   # every record of the step counts at one cell at least (every haplotype is tracked)


def test_refusals(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)

    def call(grid, vo, V):
        return _capi.replay_tree_events(copy.deepcopy(m), 1000, grid, vo, V, tau=True)
    with pytest.raises(ValueError, match=r"vgx_test_tau_tree_events: grid must increase strictly \(grid\[1\]\)"):
        call([0.5, 0.5], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tau_tree_events: T = 0 must be at least 1"):
        call([], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tau_tree_events: V = 0 must be at least 1"):
        call([0.5], np.full(H, -1, dtype=np.int32), 0)
    bad = ident.copy()
    bad[1] = H
    with pytest.raises(ValueError, match=r"vgx_test_tau_tree_events: variant_of\[1\] = %d is outside \[-1, %d\)" % (H, H)):
        call([0.5], bad, H)
    V = 16384 // (7 * P) + 1   # 7 P V 4 bytes of cells just above 64 KiB, P V 4 bytes far below
    assert 4 * P * V <= 65536 < 28 * P * V
    with pytest.raises(ValueError, match=r"vgx_test_tau_tree_events: %d populations x %d classes x 7 channels need %d bytes of cells, above the 65536 bytes of LDS"
                       % (P, V, 28 * P * V)):
        call([0.5], np.zeros(H, dtype=np.int32), V)
    m.sCounter = 1
    with pytest.raises(ValueError, match="Less than two cases were sampled"):
        call([0.5], ident, H)
