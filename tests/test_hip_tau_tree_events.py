"""Ensemble.tau_tree_events(): the tree events per interval of every replicate of a tau ensemble on the device
(vgx_get_tau_tree_events), exactly what the host replay of the same rule (``_capi.replay_tree_events(tau=True)``, pinned to a
pure-Python restatement in test_tau_tree_events_rule.py) gives on every replicate's chain and state; its ``lineages()`` is
``Ensemble.tau_lineages()`` field for field; the walk's status and six generator words are those of ``tau_genealogies()``; both tau
paths, the three seed forms, chains with and without a prefix, restarted replicates, subsets, passes, tiles, walks that fail, the
summary, the refusals and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _seed_of
from test_hip_ensemble_tau_genealogies import PATHS, SEEDS, _fresh, _near_critical_warm, seed_forms, warm
from test_hip_tau_lineages import _few_samples_ensemble, _grid, _three
from test_hip_tree_events import LN_FIELDS, _all_tracked, assert_lineages_equal

pytestmark = pytest.mark.gpu
TE_FIELDS = ("counts", "status", "status_arg", "records", "rng_raw")


@pytest.fixture(autouse=True)
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "64")   # several tiles per replicate at these sizes


def _host_row(ens, r, seed, grid, vo, V, tile=0):
    """replay_tree_events(tau=True) on replicate r's state and whole chain, started where Ensemble.tau_genealogy(r, seed) starts."""
    from vgsim_amd import _capi
    try:
        m = ens._tau_chain_model(r)
    except RuntimeError as e:   # a step of more rows than the device pass sorts: the status-10 text
        raise ValueError(str(e))
    return _capi.replay_tree_events(m, seed, grid, vo, V, tile=tile, rng_position=(0, 0), tau=True)


def assert_rows_equal_host(ens, te, seed, grid, vo, V):
    """Every row against the host replay: the same block, or zeros, a nonzero status and the host's message.  Returns the healthy rows."""
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


def check_against_genealogies_and_lineages(ens, te, seed, grid, vo):
    """The walk is that of tau_genealogies(): status, status_arg and all six generator words; with every haplotype tracked the
    samples are the tips and the coalescences the internal nodes of the batch's tree; lineages() is tau_lineages()."""
    batch = ens.tau_genealogies(seed=seed, replicates=te.replicates)
    assert np.array_equal(te.status, batch.status) and np.array_equal(te.status_arg, batch.status_arg)
    assert te.rng_raw.shape == (len(te.replicates), 6) and np.array_equal(te.rng_raw, batch.rng_raw)
    for i in np.nonzero(te.ok)[0]:
        r = int(te.replicates[i])
        sC = int(ens.engine.counters(r).reserved[4])
        tree = np.asarray(batch.replicate(r)["tree"])
        assert len(tree) == 2 * sC - 1
        assert int(te.samples()[i].sum()) == sC and int(te.coalescences()[i].sum()) == len(np.unique(tree[tree >= 0])) == sC - 1, "replicate %d" % r
    assert_lineages_equal(te, ens.tau_lineages(times=grid, variants=vo, seed=seed, replicates=te.replicates))


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_rows_equal_the_host_replay(name, path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    R = 6
    ens = Ensemble(sim, R, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.model.events.ptr > 0 and all(ens.engine.counters(r).restarts == 0 for r in range(R))
    P, H = ens.model.popNum, ens.model.hapNum
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    for s in seed_forms(R):
        te = ens.tau_tree_events(times=grid, variants=vo, seed=s)
        assert list(te.replicates) == list(range(R)) and te.passes >= 1 and te.counts.dtype == np.int32
        assert te.counts.shape == (R, len(grid) + 1, P, V, 7) and len(te.stage_ms) == 3
        assert assert_rows_equal_host(ens, te, s, grid, vo, V) > 0, name
        check_against_genealogies_and_lineages(ens, te, s, grid, vo)
    # three classes, one haplotype untracked, on one point
    vo3 = _three(H)
    V3 = max(int(vo3.max()) + 1, 1)
    one = ens.tau_tree_events(times=grid[2:3], variants=vo3, seed=s)
    assert np.array_equal(one.variant_of, vo3) and one.counts.shape[1:] == (2, P, V3, 7)
    assert_rows_equal_host(ens, one, s, grid[2:3], vo3, V3)
    assert_lineages_equal(one, ens.tau_lineages(times=grid[2:3], variants=vo3, seed=s))
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log; and replicates that restarted (no prefix for them) beside ones
    that carry the prefix."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    for s in (None, 99):
        te = ens.tau_tree_events(times=grid, variants=vo, seed=s)
        assert_rows_equal_host(ens, te, s, grid, vo, V)
        check_against_genealogies_and_lineages(ens, te, s, grid, vo)
    ens.close()
    sim = _near_critical_warm()
    ens = Ensemble(sim, 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    for s in (None, 99):
        te = ens.tau_tree_events(times=grid, variants=vo, seed=s)
        assert_rows_equal_host(ens, te, s, grid, vo, V)
        check_against_genealogies_and_lineages(ens, te, s, grid, vo)
    ens.close()


def test_subsets_passes_and_tiles(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    full = ens.tau_tree_events(times=grid, variants=vo, seed=99)
    assert full.passes == 1 and full.ok.sum() > 100
    assert_lineages_equal(full, ens.tau_lineages(times=grid, variants=vo, seed=99))
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_tree_events(times=grid, variants=vo, seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert assert_rows_equal_host(ens, sub, seeds, grid, vo, V) > 30
    same = ens.tau_tree_events(times=grid, variants=vo, seed=99, replicates=order)
    for k in TE_FIELDS:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes
    small = ens.tau_tree_events(times=grid, variants=vo, seed=99)
    assert small.passes > 1
    for k in TE_FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "7")          # no value depends on the tile
    tiny = ens.tau_tree_events(times=grid, variants=vo, seed=99)
    for k in TE_FIELDS:
        assert np.array_equal(getattr(tiny, k), getattr(full, k)), k
    ens.close()


def test_failed_walks_give_zeros_and_do_not_fail_the_call():
    from vgsim_amd import _capi
    ens = _few_samples_ensemble()
    grid = _grid(ens)
    vo, V = _all_tracked(ens)
    te = ens.tau_tree_events(times=grid, variants=vo, seed=5)
    batch = ens.tau_genealogies(seed=5)
    assert (te.status == 1).any() and te.ok.any() and np.array_equal(te.status, batch.status), te.status
    assert_rows_equal_host(ens, te, 5, grid, vo, V)
    keep = np.nonzero(te.status <= 1)[0]
    band = ens.tau_tree_events(times=grid, variants=vo, seed=5, replicates=keep, summary=dict(quantiles=(0.5,), method='lower'))
    ok = band.ok
    assert np.array_equal(band.status, te.status[keep]) and (~ok).any()
    assert np.array_equal(band.summary.count, [ok.sum()])
    assert np.array_equal(band.summary.sum[0], band.counts[ok].astype(np.int64).sum(axis=0))
    # a failed walk of another kind inside a group refuses the summary, after the counts are there
    assert (te.status > 1).any(), te.status
    with pytest.raises(_capi.VgxError, match=r"vgx_get_tau_tree_events: summary: \d+ replicate\(s\) of a group have a walk that failed") as refused:
        ens.tau_tree_events(times=grid, variants=vo, seed=5, summary=dict(quantiles=(0.5,)))
    late = refused.value.tree_events
    assert np.array_equal(late.counts, te.counts) and np.array_equal(late.status, te.status) and late.summary is None
    ens.close()


def test_summary_bands_and_values_false():
    from vgsim_amd.ensemble import Ensemble
    R, Q = 12, (0.1, 0.5, 0.9)
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, R, seeds=300 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    vo = _three(ens.model.hapNum)
    grid = _grid(ens)
    te = ens.tau_tree_events(times=grid, variants=vo, seed=8)
    reps = np.nonzero(te.ok)[0]
    assert len(reps) >= 4
    by = np.arange(R) % 2
    band = ens.tau_tree_events(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.counts, te.counts[reps])
    s, g = band.summary, by[reps]
    for k in range(2):   # numpy on the delivered block
        rows = band.counts[g == k].astype(np.int64)
        assert s.count[k] == len(rows)
        assert np.array_equal(s.sum[k], rows.sum(axis=0)) and np.array_equal(s.min[k], rows.min(axis=0)) and np.array_equal(s.max[k], rows.max(axis=0))
        assert np.array_equal(s.quantiles[k], np.quantile(rows, Q, axis=0, method='lower'))
    alone = ens.tau_tree_events(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'), values=False)
    assert alone.counts is None and np.array_equal(alone.status, band.status)
    assert np.array_equal(alone.summary.sum, s.sum) and np.array_equal(alone.summary.quantiles, s.quantiles)
    with pytest.raises(ValueError, match="values=False needs summary="):
        ens.tau_tree_events(times=grid, values=False)
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_tree_events(times=[0.5])
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_tree_events(times=[0.5])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_tree_events(times=[0.5])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_tree_events(times=[0.5], **kw)
    with pytest.raises(ValueError, match="grid must increase strictly"):
        ens.tau_tree_events(times=[0.5, 0.5])
    P, H = ens.model.popNum, ens.model.hapNum
    V = 16384 // (7 * P) + 1   # 7 P V 4 bytes of cells just above 64 KiB: tau_lineages() takes it, tau_tree_events() does not
    with pytest.raises(ValueError, match=r"x 7 channels need %d bytes of cells, above the 65536 bytes of LDS" % (28 * P * V)):
        ens.tau_tree_events(times=[0.5], variants=np.full(H, V - 1, dtype=np.int64))
    assert ens.tau_lineages(times=[0.5], variants=np.full(H, V - 1, dtype=np.int64)).values.shape[-1] == V
    with pytest.raises(ValueError, match=r"tree_events\(\) walks direct chains only"):   # the direct call refuses tau chains
        ens.tree_events(times=[0.5])
    assert len(ens.tau_tree_events(times=[0.5], seed=1, replicates=[1]).replicates) == 1
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    grid = _grid(ens)
    vo, _ = _all_tracked(ens)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    events = [ens.replicate_events(r) for r in range(ens.R)]
    ln = ens.tau_lineages(times=grid, variants=vo, seed=5)
    a = ens.tau_tree_events(times=grid, variants=vo, seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
        assert np.array_equal(events[r], ens.replicate_events(r)), r
    ln2 = ens.tau_lineages(times=grid, variants=vo, seed=5)
    for k in LN_FIELDS:
        assert np.array_equal(getattr(ln, k), getattr(ln2, k)), k
    b = ens.tau_tree_events(times=grid, variants=vo, seed=5)
    for k in TE_FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    ens.close()
