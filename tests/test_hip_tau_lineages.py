"""Ensemble.tau_lineages(): ancestral lineages per grid time, population and variant class of every replicate of a tau ensemble on
the device (vgx_get_tau_lineages), exactly what the host replay of the same rule (``_capi.replay_tau_lineages``: the tau walk,
observer, tile walk and suffix sum compiled for the host, pinned to a pure-Python restatement in test_tau_lineages_rule.py) gives on
every replicate's chain and state, assembled as ``Ensemble.tau_genealogy`` assembles it; the walk's status and six generator words
are those of ``tau_genealogies()``; both tau paths, the three seed forms, chains with and without a prefix, restarted replicates,
subsets, several passes, tiles, walks that fail, the summary, the refusals and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _seed_of
from test_hip_ensemble_tau_genealogies import PATHS, SEEDS, _fresh, _near_critical_warm, seed_forms, warm
from test_lineages_rule import alive

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "64")   # several tiles per replicate at these sizes


def _own_times(ens, r):
    return ens.replicate_events(r)[0][int(ens.engine.counters(r).ev_first_new):]


def _grid(ens):
    """A common grid: one point below the first event of any chain, one inside the prefix (if the model holds one), one exactly at
    an own step's time of the replicate with the most steps, one inside its own steps, and one above every chain's end."""
    pre = np.asarray(ens.model.events.times[:int(ens.model.events.ptr)], dtype=np.float64)
    steps = [_own_times(ens, r) for r in range(ens.R)]
    own = max(steps, key=len)
    assert len(own) >= 2
    first = min(float(t[0]) for t in steps if len(t))
    last = max(float(t[-1]) for t in steps if len(t))
    j = min((2 * len(own)) // 3, len(own) - 2)
    points = {min(first, float(pre[0]) if len(pre) else np.inf) - 1.0, float(own[len(own) // 3]),
              0.5 * (float(own[j]) + float(own[j + 1])), 10.0 * abs(last) + 1.0}
    if len(pre) >= 2:
        k = next(i for i in range(len(pre) // 2, len(pre) - 1) if pre[i] < pre[i + 1])
        points.add(0.5 * (float(pre[k]) + float(pre[k + 1])))
    return np.array(sorted(points))


def _three(H):
    vo = (np.arange(H) % 3).astype(np.int32)
    vo[H // 2] = -1
    return vo


def _host_row(ens, r, seed, grid, vo, V, tile=0):
    """replay_tau_lineages on replicate r's state and whole chain, started where Ensemble.tau_genealogy(r, seed) starts."""
    from vgsim_amd import _capi
    try:
        m = ens._tau_chain_model(r)
    except RuntimeError as e:   # a step of more rows than the device pass sorts: the status-10 text
        raise ValueError(str(e))
    return _capi.replay_tau_lineages(m, seed, grid, vo, V, tile=tile, rng_position=(0, 0))


def assert_rows_equal_host(ens, ln, seed, grid, vo, V):
    """Every row against the host replay: the same block, or zeros, a nonzero status and the host's message.  Returns the healthy rows."""
    healthy = 0
    for i, r in enumerate(ln.replicates):
        try:
            want = _host_row(ens, int(r), _seed_of(seed, i), grid, vo, V)
        except ValueError as e:
            assert ln.status[i] != 0 and not ln.ok[i], "replicate %d: the host replay raised %r" % (r, str(e))
            assert ln.message(i) == str(e), "replicate %d" % r
            assert not ln.values[i].any() and not ln.root[i].any() and ln.records[i] == 0, "replicate %d" % r
            continue
        assert ln.status[i] == 0, "replicate %d: %s" % (r, ln.message(i))
        assert np.array_equal(ln.values[i], want["values"]), "replicate %d values" % r
        assert np.array_equal(ln.root[i], want["root"]), "replicate %d root" % r
        assert ln.records[i] == want["records"] and tuple(int(x) for x in ln.rng_raw[i]) == want["rng_raw"], "replicate %d" % r
        healthy += 1
    return healthy


def check_against_genealogies(ens, ln, seed, grid):
    """The walk is that of tau_genealogies(): status, status_arg and all six generator words; on healthy rows one root and the
    lineages-through-time curve of the batch's tree (the nodes of one step share a time: zero-length branches are alive nowhere)."""
    batch = ens.tau_genealogies(seed=seed, replicates=ln.replicates)
    assert np.array_equal(ln.status, batch.status) and np.array_equal(ln.status_arg, batch.status_arg)
    assert ln.rng_raw.shape == (len(ln.replicates), 6) and np.array_equal(ln.rng_raw, batch.rng_raw)
    for i in np.nonzero(ln.ok)[0]:
        assert int(ln.root[i].sum()) == 1, "replicate %d root" % ln.replicates[i]
        assert np.array_equal(ln.total()[i], alive(batch.replicate(int(ln.replicates[i])), grid)), "replicate %d" % ln.replicates[i]
    assert (ln.values >= 0).all()


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
    assert len(grid) == 5
    ident = np.arange(H, dtype=np.int32)
    for s in seed_forms(R):
        ln = ens.tau_lineages(times=grid, seed=s)
        assert list(ln.replicates) == list(range(R)) and ln.passes >= 1 and ln.values.dtype == np.int32
        assert ln.values.shape == (R, len(grid), P, H) and ln.root.shape == (R, P, H) and len(ln.stage_ms) == 4
        assert assert_rows_equal_host(ens, ln, s, grid, ident, H) > 0, name
        check_against_genealogies(ens, ln, s, grid)
    # the share of the infectious hosts that are ancestors of the sample, over tau_prevalence's int64 values
    pv = ens.tau_prevalence(times=grid)
    share = ln.sampled_share(pv)
    assert np.isnan(share[pv.values <= 0]).all() and np.array_equal(share[pv.values > 0], (ln.values / np.maximum(pv.values, 1))[pv.values > 0])
    # three classes, one haplotype untracked, on one point
    vo = _three(H)
    V3 = max(int(vo.max()) + 1, 1)   # (three, unless the model has fewer haplotypes)
    one = ens.tau_lineages(times=grid[2:3], variants=vo, seed=s)
    assert np.array_equal(one.variant_of, vo) and one.values.shape[1:] == (1, P, V3)
    assert_rows_equal_host(ens, one, s, grid[2:3], vo, V3)
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log; and replicates that restarted (no prefix for them) beside ones
    that carry the prefix: the loop over the prefix's times is shared by the latter alone."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    H = ens.model.hapNum
    grid = _grid(ens)
    for s in (None, 99):
        ln = ens.tau_lineages(times=grid, seed=s)
        assert_rows_equal_host(ens, ln, s, grid, np.arange(H, dtype=np.int32), H)
        check_against_genealogies(ens, ln, s, grid)
    ens.close()
    sim = _near_critical_warm()
    ens = Ensemble(sim, 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    H = ens.model.hapNum
    grid = _grid(ens)
    for s in (None, 99):
        ln = ens.tau_lineages(times=grid, seed=s)
        assert_rows_equal_host(ens, ln, s, grid, np.arange(H, dtype=np.int32), H)
        check_against_genealogies(ens, ln, s, grid)
    ens.close()


def test_subsets_passes_and_tiles(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    H = ens.model.hapNum
    ident = np.arange(H, dtype=np.int32)
    grid = _grid(ens)
    full = ens.tau_lineages(times=grid, seed=99)
    assert full.passes == 1 and full.ok.sum() > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_lineages(times=grid, seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert assert_rows_equal_host(ens, sub, seeds, grid, ident, H) > 30
    same = ens.tau_lineages(times=grid, seed=99, replicates=order)
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes
    small = ens.tau_lineages(times=grid, seed=99)
    assert small.passes > 1
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "7")          # no value depends on the tile
    tiny = ens.tau_lineages(times=grid, seed=99)
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(tiny, k), getattr(full, k)), k
    ens.close()


def _few_samples_ensemble():
    """The near-critical model: attempts that die out early leave replicates with fewer than two samples beside healthy ones."""
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(_near_critical_warm(), 32, seeds=500 + np.arange(32, dtype=np.int64))
    ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    return ens


def test_failed_walks_give_zeros_and_do_not_fail_the_call():
    """Replicates below two samples (status 1) beside healthy ones: zeros, the call goes through, and the summary leaves them out.
    The same ensemble holds walks that fail otherwise (status 12: at these very small counts tau steps write rows numpy's
    hypergeometric would refuse): inside a group they refuse the summary, with the values attached."""
    from vgsim_amd import _capi
    ens = _few_samples_ensemble()
    H = ens.model.hapNum
    grid = _grid(ens)
    ln = ens.tau_lineages(times=grid, seed=5)
    batch = ens.tau_genealogies(seed=5)
    assert (ln.status == 1).any() and ln.ok.any() and np.array_equal(ln.status, batch.status), ln.status
    assert_rows_equal_host(ens, ln, 5, grid, np.arange(H, dtype=np.int32), H)
    keep = np.nonzero(ln.status <= 1)[0]
    band = ens.tau_lineages(times=grid, seed=5, replicates=keep, summary=dict(quantiles=(0.5,), method='lower'))
    ok = band.ok
    assert np.array_equal(band.status, ln.status[keep]) and (~ok).any()
    assert np.array_equal(band.summary.count, [ok.sum()])
    assert np.array_equal(band.summary.sum[0], band.values[ok].astype(np.int64).sum(axis=0))
    # a failed walk of another kind inside a group refuses the summary, after the values are there
    assert (ln.status > 1).any(), ln.status
    with pytest.raises(_capi.VgxError, match=r"vgx_get_tau_lineages: summary: \d+ replicate\(s\) of a group have a walk that failed") as refused:
        ens.tau_lineages(times=grid, seed=5, summary=dict(quantiles=(0.5,)))
    late = refused.value.lineages
    assert np.array_equal(late.values, ln.values) and np.array_equal(late.root, ln.root) and np.array_equal(late.status, ln.status)
    assert late.summary is None
    ens.close()


def test_summary_bands_and_values_false():
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble, _summary_ranks
    R, Q = 12, (0.1, 0.5, 0.9)
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, R, seeds=300 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    vo = _three(ens.model.hapNum)
    grid = _grid(ens)
    ln = ens.tau_lineages(times=grid, variants=vo, seed=8)
    reps = np.nonzero(ln.ok)[0]
    assert len(reps) >= 4
    by = np.arange(R) % 2
    band = ens.tau_lineages(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.values, ln.values[reps])
    s, g = band.summary, by[reps]
    ranks = np.stack([_summary_ranks(Q, int((g == k).sum()), 'lower') for k in range(2)])
    want = _capi.column_summary(band.values.reshape(len(reps), -1), g, 2, ranks)
    cols = band.values.shape[1:]
    assert np.array_equal(s.count, want["count"])
    for k in ("sum", "min", "max"):
        assert np.array_equal(getattr(s, k), want[k].reshape((2,) + cols)), k
    assert np.array_equal(s.sumsq_words, want["sumsq"].reshape((2,) + cols + (2,)))
    assert np.array_equal(s.quantiles, want["stat"].reshape((2, len(Q)) + cols).astype(np.float64))
    alone = ens.tau_lineages(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'), values=False)
    assert alone.values is None and np.array_equal(alone.root, band.root)
    assert np.array_equal(alone.summary.sum, s.sum) and np.array_equal(alone.summary.quantiles, s.quantiles)
    with pytest.raises(ValueError, match="values=False needs summary="):
        ens.tau_lineages(times=grid, values=False)
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_lineages(times=[0.5])
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_lineages(times=[0.5])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_lineages(times=[0.5])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_lineages(times=[0.5], **kw)
    with pytest.raises(ValueError, match="grid must increase strictly"):
        ens.tau_lineages(times=[0.5, 0.5])
    with pytest.raises(ValueError, match="above the 65536 bytes of LDS"):
        ens.tau_lineages(times=[0.5], variants=np.full(ens.model.hapNum, 16384 // ens.model.popNum, dtype=np.int64))
    with pytest.raises(ValueError, match="direct chains only"):   # the direct call still refuses tau chains
        ens.lineages(times=[0.5])
    assert len(ens.tau_lineages(times=[0.5], seed=1, replicates=[1]).replicates) == 1
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    grid = _grid(ens)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    events = [ens.replicate_events(r) for r in range(ens.R)]
    first = ens.tau_genealogies(seed=5)
    pv = ens.tau_prevalence(times=grid)
    a = ens.tau_lineages(times=grid, seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
        assert np.array_equal(events[r], ens.replicate_events(r)), r
    second = ens.tau_genealogies(seed=5)
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
              "mig_offsets", "mig_node", "mig_old", "mig_new", "mig_time", "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    pv2 = ens.tau_prevalence(times=grid)
    assert np.array_equal(pv.values, pv2.values) and np.array_equal(pv.final, pv2.final)
    b = ens.tau_lineages(times=grid, seed=5)
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    ens.close()
