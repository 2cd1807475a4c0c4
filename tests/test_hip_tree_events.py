"""Ensemble.tree_events(): samples, coalescences, lineage mutations and lineage moves per interval of a grid, population and variant
class of every replicate on the device (vgx_get_tree_events), exactly what the host replay of the same rule
(``_capi.replay_tree_events``, pinned to a pure-Python restatement in test_tree_events_rule.py) gives on every replicate's chain and
state; its ``lineages()`` is ``Ensemble.lineages()`` field for field; the walk's status and generator are those of
``genealogies()``; subsets, several walk passes, walks that fail, the summary and the refusals."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _ensemble, _seed_of
from test_hip_lineages import _grid, _three

pytestmark = pytest.mark.gpu
LN_FIELDS = ("values", "root", "status", "status_arg", "records", "rng_raw")


@pytest.fixture(autouse=True)
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "64")   # several tiles per replicate at these sizes


def _all_tracked(ens):
    """(variant_of, V) with every haplotype tracked: its own class where 7 P V cells fit the LDS limit, else four classes."""
    H, P = ens.model.hapNum, ens.model.popNum
    if 28 * P * H <= 65536:
        return np.arange(H, dtype=np.int32), H
    return (np.arange(H) % 4).astype(np.int32), 4


def _host_row(ens, r, seed, grid, vo, V, tile=0):
    """replay_tree_events on replicate r's state and chain, started where Ensemble.genealogy(r, seed) starts."""
    from vgsim_amd import _capi
    from vgsim_amd._model import Events
    m = ens.replicate_state(r)
    chain = ens.replicate_events(r)
    ev = Events()
    ev.CreateEvents(max(chain.shape[1], 1))
    ev.times[:chain.shape[1]] = chain[0]
    for k, name in enumerate(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")):
        getattr(ev, name)[:chain.shape[1]] = chain[k + 1].astype(np.int64)
    ev.ptr = chain.shape[1]
    m.events = ev
    raw = None
    if seed is None:
        c = ens.engine.counters(r)
        att, draws = (int(c.reserved[1]), 2 * int(c.reserved[2])) if c.reserved[1] >= 0 else (0, 0)
        pos = (C.c_uint64 * 4)()
        ens.engine.lib.vgx_rng_position(int(ens.seeds[r]), att, draws, C.byref(pos))
        raw = tuple(int(x) for x in pos) + (0, 0)
    return _capi.replay_tree_events(m, seed, grid, vo, V, tile=tile, rng_raw=raw)


def assert_rows_equal_host(ens, te, seed, grid, vo, V):
    """Every row against the host replay: the same block, or zeros and the host's message.  Returns the healthy rows."""
    healthy = 0
    for i, r in enumerate(te.replicates):
        try:
            want = _host_row(ens, int(r), _seed_of(seed, i), grid, vo, V)
        except ValueError as e:
            assert te.status[i] != 0 and not te.ok[i], "replicate %d: the host replay raised %r" % (r, str(e))
            assert te.message(i) == str(e), "replicate %d" % r
            assert not te.counts[i].any() and te.records[i] == 0, "replicate %d" % r
            continue
        assert te.status[i] == 0, "replicate %d: %s" % (r, te.message(i))
        assert np.array_equal(te.counts[i], want["counts"]), "replicate %d counts" % r
        assert te.records[i] == want["records"] and tuple(int(x) for x in te.rng_raw[i]) == want["rng_raw"], "replicate %d" % r
        healthy += 1
    return healthy


def assert_lineages_equal(te, ln):
    got = te.lineages()
    for k in LN_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(ln, k)), k
    assert got.values.dtype == np.int32 and got.root.dtype == np.int32


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70"])
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_rows_equal_the_host_replay(name, seed):
    R = 6
    ens = _ensemble(name, R)
    P = ens.model.popNum
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    log_before = [ens.replicate_events(r).copy() for r in range(R)]
    ln = ens.lineages(times=grid, variants=vo, seed=s)
    te = ens.tree_events(times=grid, variants=vo, seed=s)
    assert list(te.replicates) == list(range(R)) and te.passes >= 1 and te.counts.dtype == np.int32
    assert te.counts.shape == (R, len(grid) + 1, P, V, 7) and te.CHANNELS[1] == "coalescences" and len(te.CHANNELS) == 7
    assert assert_rows_equal_host(ens, te, s, grid, vo, V) > 0
    for k, name_k in enumerate(te.CHANNELS):
        assert np.array_equal(getattr(te, name_k)(), te.counts[..., k])
    # the walk is that of genealogies(): the same status and the same generator afterwards
    batch = ens.genealogies(seed=s)
    assert np.array_equal(te.status, batch.status) and np.array_equal(te.status_arg, batch.status_arg)
    assert np.array_equal(te.rng_raw, batch.rng_raw)
    # one walk serves both questions, and leaves the log and lineages() as they were
    assert_lineages_equal(te, ln)
    again = ens.lineages(times=grid, variants=vo, seed=s)
    for k in LN_FIELDS:
        assert np.array_equal(getattr(again, k), getattr(ln, k)), k
    assert all(np.array_equal(ens.replicate_events(r), log_before[r]) for r in range(R))
    for i in np.nonzero(te.ok)[0]:
        sC = int(ens.engine.counters(int(i)).reserved[4])
        assert int(te.samples()[i].sum()) == sC and int(te.coalescences()[i].sum()) == sC - 1, "replicate %d" % i
        # internal nodes of the tree cut on the same grid (an event at exactly a grid time lies in the interval that ends there)
        g = batch.replicate(int(i))
        tree = np.asarray(g["tree"])
        internal = np.zeros(len(tree), dtype=bool)
        internal[tree[tree >= 0]] = True
        want = np.bincount(np.searchsorted(grid, np.asarray(g["times"])[internal], side="left"), minlength=len(grid) + 1)
        assert np.array_equal(te.coalescences()[i].sum(axis=(-1, -2)), want), "replicate %d" % i
    # three classes, one haplotype untracked, on one point
    vo3 = _three(ens.model.hapNum)
    V3 = int(vo3.max()) + 1
    one = ens.tree_events(times=grid[2:3], variants=vo3, seed=s)
    assert np.array_equal(one.variant_of, vo3) and one.counts.shape[1:] == (2, P, V3, 7)
    assert_rows_equal_host(ens, one, s, grid[2:3], vo3, V3)
    assert_lineages_equal(one, ens.lineages(times=grid[2:3], variants=vo3, seed=s))
    ens.close()


def test_partial_wavefronts_subsets_and_passes(monkeypatch):
    R = 130
    ens = _ensemble("g9_short", R, n_max=1500, seeds0=7000)
    H = ens.model.hapNum
    ident = np.arange(H, dtype=np.int32)
    grid = _grid(ens)
    full = ens.tree_events(times=grid, seed=99)
    assert assert_rows_equal_host(ens, full, 99, grid, ident, H) > 100
    assert_lineages_equal(full, ens.lineages(times=grid, seed=99))
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tree_events(times=grid, seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_rows_equal_host(ens, sub, seeds, grid, ident, H)
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "200000")   # several walk passes
    small = ens.tree_events(times=grid, seed=99)
    assert small.passes > 1
    for k in ("counts", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "7")        # no value depends on the tile
    tiny = ens.tree_events(times=grid, seed=99)
    assert np.array_equal(tiny.counts, full.counts)
    ens.close()


def test_failed_walks_give_zeros_and_do_not_fail_the_call():
    from vgsim_amd import _capi
    ens = _ensemble("recomb_a", 8, n_max=3000)
    H = ens.model.hapNum
    grid = _grid(ens)
    te = ens.tree_events(times=grid, seed=21)
    batch = ens.genealogies(seed=21)
    assert (te.status == 4).any() and np.array_equal(te.status, batch.status), te.status   # lineages that never coalesce
    bad = int(np.nonzero(te.status == 4)[0][0])
    assert "never coalesced" in te.message(bad) and te.message(bad) == batch.message(bad) and not te.counts[bad].any()
    assert_rows_equal_host(ens, te, 21, grid, np.arange(H, dtype=np.int32), H)
    # a failed walk inside a group refuses the summary, after the counts are there
    with pytest.raises(_capi.VgxError, match=r"vgx_get_tree_events: summary: \d+ replicate\(s\) of a group have a walk that failed") as refused:
        ens.tree_events(times=grid, seed=21, summary=dict(quantiles=(0.5,)))
    late = refused.value.tree_events
    assert np.array_equal(late.counts, te.counts) and np.array_equal(late.status, te.status) and late.summary is None
    ens.close()

    ens = _ensemble("extinct", 24, n_max=50, seeds0=1)
    H = ens.model.hapNum
    grid = _grid(ens)
    te = ens.tree_events(times=grid, seed=5)
    batch = ens.genealogies(seed=5)
    assert (te.status == 1).any() and np.array_equal(te.status, batch.status), te.status     # fewer than two samples
    assert_rows_equal_host(ens, te, 5, grid, np.arange(H, dtype=np.int32), H)
    # fewer than two samples is known before the walk: such rows are in no group of the summary
    keep = np.nonzero(te.status <= 1)[0]
    band = ens.tree_events(times=grid, seed=5, replicates=keep, summary=dict(quantiles=(0.5,), method='lower'))
    ok = band.ok
    assert np.array_equal(band.status, te.status[keep]) and (~ok).any()
    assert np.array_equal(band.summary.count, [ok.sum()])
    assert np.array_equal(band.summary.sum[0], band.counts[ok].astype(np.int64).sum(axis=0))
    ens.close()


def test_summary_bands_and_values_false():
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import _summary_ranks
    R, Q = 12, (0.1, 0.5, 0.9)
    ens = _ensemble("g9_short", R, n_max=2000, seeds0=300)
    vo = _three(ens.model.hapNum)
    grid = _grid(ens)
    te = ens.tree_events(times=grid, variants=vo, seed=8)
    reps = np.nonzero(te.ok)[0]
    assert len(reps) >= 4
    by = np.arange(R) % 2
    band = ens.tree_events(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.counts, te.counts[reps])
    s, g = band.summary, by[reps]
    ranks = np.stack([_summary_ranks(Q, int((g == k).sum()), 'lower') for k in range(2)])
    want = _capi.column_summary(band.counts.reshape(len(reps), -1), g, 2, ranks)
    cols = band.counts.shape[1:]
    assert cols == (len(grid) + 1, ens.model.popNum, 3, 7)
    assert np.array_equal(s.count, want["count"])
    for k in ("sum", "min", "max"):
        assert np.array_equal(getattr(s, k), want[k].reshape((2,) + cols)), k
    assert np.array_equal(s.sumsq_words, want["sumsq"].reshape((2,) + cols + (2,)))
    assert np.array_equal(s.quantiles, want["stat"].reshape((2, len(Q)) + cols).astype(np.float64))
    # numpy on the delivered block
    for k in range(2):
        rows = band.counts[g == k].astype(np.int64)
        assert np.array_equal(s.sum[k], rows.sum(axis=0)) and np.array_equal(s.min[k], rows.min(axis=0)) and np.array_equal(s.max[k], rows.max(axis=0))
        assert np.array_equal(s.quantiles[k], np.quantile(rows, Q, axis=0, method='lower'))
    alone = ens.tree_events(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'), values=False)
    assert alone.counts is None and np.array_equal(alone.status, band.status) and np.array_equal(alone.records, band.records)
    assert np.array_equal(alone.summary.sum, s.sum) and np.array_equal(alone.summary.quantiles, s.quantiles)
    with pytest.raises(ValueError, match="values=False needs summary="):
        ens.tree_events(times=grid, values=False)
    ens.close()


def test_refusals():
    ens = _ensemble("g9_short", 3, n_max=500)
    P, H = ens.model.popNum, ens.model.hapNum
    with pytest.raises(ValueError, match="replicates must be distinct"):
        ens.tree_events(times=[0.5], replicates=[1, 1])
    with pytest.raises(ValueError, match="replicate index out of range"):
        ens.tree_events(times=[0.5], replicates=[3])
    with pytest.raises(ValueError, match="grid must increase strictly"):
        ens.tree_events(times=[0.5, 0.5])
    with pytest.raises(ValueError, match="one seed per selected replicate"):
        ens.tree_events(times=[0.5], seed=[1, 2])
    V = 16384 // (7 * P) + 1   # 7 P V 4 bytes of cells just above 64 KiB: lineages() takes it, tree_events() does not
    with pytest.raises(ValueError, match=r"%d populations x %d classes x 7 channels need %d bytes of cells, above the 65536 bytes of LDS" % (P, V, 28 * P * V)):
        ens.tree_events(times=[0.5], variants=np.full(H, V - 1, dtype=np.int64))
    assert ens.lineages(times=[0.5], variants=np.full(H, V - 1, dtype=np.int64)).values.shape[-1] == V
    assert ens.tree_events(times=[0.5], variants=np.full(H, V - 2, dtype=np.int64)).counts.shape[-2:] == (V - 1, 7)
    # the library's own refusal, past the Python check
    from vgsim_amd import _capi
    io = _capi.VgxTreeEventsIO()
    grid, vo = np.array([0.5]), np.zeros(H, dtype=np.int32)
    io.n, io.T, io.grid, io.V, io.variant_of = 0, 1, _capi._p(grid), V, vo.ctypes.data_as(C.POINTER(C.c_int32))
    with pytest.raises(_capi.VgxError, match=r"vgx_get_tree_events: %d populations x %d classes x 7 channels need %d bytes" % (P, V, 28 * P * V)):
        ens.engine._check(ens.engine.lib.vgx_get_tree_events(ens.engine.handle, C.byref(io)))
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"tree_events\(\) needs the event log"):
        ens.tree_events(times=[0.5])
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"tree_events\(\) walks direct chains only"):
        ens.tree_events(times=[0.5])
    ens.close()


def test_tiles_past_the_launch_cap(monkeypatch):
    """More tiles than a launch has workgroup rows (65535): a workgroup then strides over several.  The ensemble, the grid and the
    preconditions (more than 65535 + 256 records, interval changes inside the head and inside the tail of the log) are those of
    test_hip_tile_stride's lineage case; tiles of one record against the default tile and against the host replay."""
    import test_hip_tile_stride as ts
    from test_hip_lineages import _host_row as lineages_host_row
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(ts.lineage_sim(), 2, seeds=np.array(ts.LINEAGE_SEEDS, dtype=np.int64))
    try:
        with helpers.quiet():
            res = ens.simulate(ts.LINEAGE_EVENTS, sample_size=10 ** 9, attempts=ts.ATTEMPTS, record_events=True)
        assert not res.restarts.any() and [int(n) for n in res.events] == [ts.LINEAGE_EVENTS] * 2
        chains = [ts.event_chain(ens, r) for r in range(2)]
        grid = ts.common_grid([t for t, _ in chains])
        H = ens.model.hapNum
        ident = np.arange(H, dtype=np.int32)
        t, cols = chains[0]
        ts.assert_lineage_borders(t, cols[0], grid, lineages_host_row(ens, 0, ts.WALK_SEED, grid, ident, H))
        monkeypatch.delenv("VGX_LINEAGES_TILE_RECORDS", raising=False)
        whole = ens.tree_events(times=grid, seed=ts.WALK_SEED)
        assert whole.status[0] == 0 and whole.records[0] > ts.CAP + 256, (whole.status, whole.records)
        monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "1")
        one = ens.tree_events(times=grid, seed=ts.WALK_SEED)
        assert assert_rows_equal_host(ens, one, ts.WALK_SEED, grid, ident, H) >= 1
        for k in ("counts", "status", "status_arg", "records", "rng_raw"):
            assert np.array_equal(getattr(one, k), getattr(whole, k)), k
    finally:
        ens.close()
