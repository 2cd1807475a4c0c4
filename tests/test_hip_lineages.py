"""Ensemble.lineages(): ancestral lineages per grid time, population and variant class of every replicate on the device
(vgx_get_lineages), exactly what the host replay of the same rule (``_capi.replay_lineages``: the walk, observer, tile walk and
suffix sum compiled for the host, pinned to a pure-Python restatement in test_lineages_rule.py) gives on every replicate's chain
and state; the walk's status and generator are those of ``genealogies()``; partly filled wavefronts, subsets, several walk passes,
walks that fail, and the summary."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _ensemble, _seed_of
from test_lineages_rule import alive

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "64")   # several tiles per replicate at these sizes


def _grid(ens):
    """A common grid from replicate 0's event times: below its first event, inside the chain (one point exactly at an event
    time), and above every chain's last event."""
    t = ens.replicate_events(0)[0]
    n = len(t)
    inner = [float(t[n // 5]), 0.5 * (float(t[n // 2]) + float(t[n // 2 + 1])), float(t[(4 * n) // 5])]
    return np.array(sorted({0.5 * float(t[0])} | set(inner) | {10.0 * float(t[-1]) + 1.0}))


def _three(H):
    vo = (np.arange(H) % 3).astype(np.int32)
    vo[H // 2] = -1
    return vo


def _host_row(ens, r, seed, grid, vo, V, tile=0):
    """replay_lineages on replicate r's state and chain, started where Ensemble.genealogy(r, seed) starts."""
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
    return _capi.replay_lineages(m, seed, grid, vo, V, tile=tile, rng_raw=raw)


def assert_rows_equal_host(ens, ln, seed, grid, vo, V):
    """Every row against the host replay: the same block, or zeros and the host's message.  Returns the healthy rows."""
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


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70"])
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_rows_equal_the_host_replay(name, seed):
    R = 6
    ens = _ensemble(name, R)
    H = ens.model.hapNum
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    grid = _grid(ens)
    ln = ens.lineages(times=grid, seed=s)
    assert list(ln.replicates) == list(range(R)) and ln.passes >= 1 and ln.values.dtype == np.int32
    assert ln.values.shape == (R, len(grid), ens.model.popNum, H) and ln.root.shape == (R, ens.model.popNum, H)
    assert assert_rows_equal_host(ens, ln, s, grid, np.arange(H, dtype=np.int32), H) > 0
    # the walk is that of genealogies(): the same status and the same generator afterwards
    batch = ens.genealogies(seed=s)
    assert np.array_equal(ln.status, batch.status) and np.array_equal(ln.status_arg, batch.status_arg)
    assert np.array_equal(ln.rng_raw, batch.rng_raw)
    pv = ens.prevalence(times=grid)
    for i in np.nonzero(ln.ok)[0]:
        assert int(ln.root[i].sum()) == 1
        assert np.array_equal(ln.total()[i], alive(batch.replicate(int(i)), grid)), "replicate %d" % i
    assert (ln.values >= 0).all() and (ln.values <= pv.values).all()      # the sample's ancestors are among the infectious hosts
    share = ln.sampled_share(pv)
    assert np.isnan(share[pv.values <= 0]).all() and np.array_equal(share[pv.values > 0], (ln.values / np.maximum(pv.values, 1))[pv.values > 0])
    # three classes, one haplotype untracked, on one point
    vo = _three(H)
    V3 = int(vo.max()) + 1   # (three, unless the model has fewer haplotypes)
    one = ens.lineages(times=grid[2:3], variants=vo, seed=s)
    assert np.array_equal(one.variant_of, vo) and one.values.shape[1:] == (1, ens.model.popNum, V3)
    assert_rows_equal_host(ens, one, s, grid[2:3], vo, V3)
    ens.close()


def test_partial_wavefronts_subsets_and_passes(monkeypatch):
    R = 130
    ens = _ensemble("g9_short", R, n_max=1500, seeds0=7000)
    H = ens.model.hapNum
    ident = np.arange(H, dtype=np.int32)
    grid = _grid(ens)
    full = ens.lineages(times=grid, seed=99)
    assert assert_rows_equal_host(ens, full, 99, grid, ident, H) > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.lineages(times=grid, seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_rows_equal_host(ens, sub, seeds, grid, ident, H)
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "200000")   # several walk passes
    small = ens.lineages(times=grid, seed=99)
    assert small.passes > 1
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "7")        # no value depends on the tile
    tiny = ens.lineages(times=grid, seed=99)
    assert np.array_equal(tiny.values, full.values) and np.array_equal(tiny.root, full.root)
    ens.close()


def test_failed_walks_give_zeros_and_do_not_fail_the_call():
    from vgsim_amd import _capi
    ens = _ensemble("recomb_a", 8, n_max=3000)
    H = ens.model.hapNum
    grid = _grid(ens)
    ln = ens.lineages(times=grid, seed=21)
    batch = ens.genealogies(seed=21)
    assert (ln.status == 4).any() and np.array_equal(ln.status, batch.status), ln.status   # lineages that never coalesce
    bad = int(np.nonzero(ln.status == 4)[0][0])
    assert "never coalesced" in ln.message(bad) and ln.message(bad) == batch.message(bad)
    assert_rows_equal_host(ens, ln, 21, grid, np.arange(H, dtype=np.int32), H)
    # a failed walk inside a group refuses the summary, after the values are there
    with pytest.raises(_capi.VgxError, match=r"vgx_get_lineages: summary: \d+ replicate\(s\) of a group have a walk that failed") as refused:
        ens.lineages(times=grid, seed=21, summary=dict(quantiles=(0.5,)))
    late = refused.value.lineages
    assert np.array_equal(late.values, ln.values) and np.array_equal(late.root, ln.root) and np.array_equal(late.status, ln.status)
    assert late.summary is None
    ens.close()

    ens = _ensemble("extinct", 24, n_max=50, seeds0=1)
    H = ens.model.hapNum
    grid = _grid(ens)
    ln = ens.lineages(times=grid, seed=5)
    batch = ens.genealogies(seed=5)
    assert (ln.status == 1).any() and np.array_equal(ln.status, batch.status), ln.status     # fewer than two samples
    assert_rows_equal_host(ens, ln, 5, grid, np.arange(H, dtype=np.int32), H)
    # fewer than two samples is known before the walk: such rows are in no group of the summary
    keep = np.nonzero(ln.status <= 1)[0]
    band = ens.lineages(times=grid, seed=5, replicates=keep, summary=dict(quantiles=(0.5,), method='lower'))
    ok = band.ok
    assert np.array_equal(band.status, ln.status[keep]) and (~ok).any()
    assert np.array_equal(band.summary.count, [ok.sum()])
    assert np.array_equal(band.summary.sum[0], band.values[ok].astype(np.int64).sum(axis=0))
    ens.close()


def test_summary_bands_and_values_false():
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import _summary_ranks
    R, Q = 12, (0.1, 0.5, 0.9)
    ens = _ensemble("g9_short", R, n_max=2000, seeds0=300)
    vo = _three(ens.model.hapNum)
    grid = _grid(ens)
    ln = ens.lineages(times=grid, variants=vo, seed=8)
    reps = np.nonzero(ln.ok)[0]
    assert len(reps) >= 4
    by = np.arange(R) % 2
    band = ens.lineages(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
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
    alone = ens.lineages(times=grid, variants=vo, seed=8, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'), values=False)
    assert alone.values is None and np.array_equal(alone.root, band.root)
    assert np.array_equal(alone.summary.sum, s.sum) and np.array_equal(alone.summary.quantiles, s.quantiles)
    with pytest.raises(ValueError, match="values=False needs summary="):
        ens.lineages(times=grid, values=False)
    ens.close()


def test_refusals():
    ens = _ensemble("g9_short", 3, n_max=500)
    with pytest.raises(ValueError, match="replicates must be distinct"):
        ens.lineages(times=[0.5], replicates=[1, 1])
    with pytest.raises(ValueError, match="replicate index out of range"):
        ens.lineages(times=[0.5], replicates=[3])
    with pytest.raises(ValueError, match="grid must increase strictly"):
        ens.lineages(times=[0.5, 0.5])
    with pytest.raises(ValueError, match="one seed per selected replicate"):
        ens.lineages(times=[0.5], seed=[1, 2])
    with pytest.raises(ValueError, match="above the 65536 bytes of LDS"):
        ens.lineages(times=[0.5], variants=np.full(ens.model.hapNum, 16384 // ens.model.popNum, dtype=np.int64))
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.lineages(times=[0.5])
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match="tau"):
        ens.lineages(times=[0.5])
    ens.close()
