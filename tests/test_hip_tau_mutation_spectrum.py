"""Ensemble.tau_mutation_spectrum(): the rows of tau ensembles against the host sweep ``_capi.mutation_spectrum`` (the definition)
applied to the trees and mutation records ``tau_genealogies()`` returns for the same walks, for equality; status, the six generator
words and messages of ``tau_genealogies()``; both tau paths, the three seed forms, chains with and without a prefix, restarted
replicates, subsets, order, several passes, failed walks, refusals and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_tau_tree_shapes import PATHS, SEEDS, _few_samples_ensemble, _fresh, _near_critical_warm, seed_forms, warm
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu

BLOCKS = ("spectrum", "substitutions", "sums", "stats")
FIELDS = BLOCKS + ("status", "status_arg", "rng_raw", "replicates")
RECORD_CASES = ("tau_b", "tau_c")   # their walks leave mutation records (7 each in the goldens): the comparison is not of zeros


def assert_rows_equal_genealogies(ens, ms, batch):
    """Every row against the host sweep over the tree and records tau_genealogies() returns for the same walk.  Returns (healthy
    rows, records in them)."""
    healthy = records = 0
    S = int(ens.model.sites)
    assert ms.sites == S and ms.spectrum.shape == (len(ms.replicates), max(S, 0), 32)
    assert np.array_equal(ms.status, batch.status) and np.array_equal(ms.status_arg, batch.status_arg)
    assert ms.rng_raw.shape == (len(ms.replicates), 6) and np.array_equal(ms.rng_raw, batch.rng_raw)
    assert np.array_equal(ms.replicates, batch.replicates)
    for i, r in enumerate(ms.replicates):
        assert ms.message(i) == batch.message(i)
        if not ms.ok[i]:
            assert not any(getattr(ms, k)[i].any() for k in BLOCKS), r
            continue
        g = batch.replicate(int(r))
        want = _capi.mutation_spectrum(g["tree"], g["mut_node"], g["mut_AS"], g["mut_DS"], g["mut_site"], S)
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(ms, k)[i], w), (r, k, getattr(ms, k)[i], w)
        assert ms.tips[i] == ens.engine.counters(int(r)).reserved[4], r
        assert ms.spectrum[i].sum() == ms.mutations[i] == len(g["mut_node"]), r
        healthy += 1
        records += len(g["mut_node"])
    return healthy, records


def assert_derived_values(ms):
    for f in (ms.singleton_share, ms.pi, ms.watterson, ms.theta_h, ms.fay_wu_h, ms.tajimas_d):
        assert np.isnan(f()[~ms.ok]).all(), f.__name__
    assert np.array_equal(ms.per_site().sum(-1), ms.mutations) and np.all(ms.pi()[ms.ok] >= 0)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])   # (tau_a: a model without sites, empty per-site blocks)
def test_rows_equal_the_host_sweep_over_tau_genealogies(name, path, monkeypatch):
    """A tau call that continues a direct warm-up (the prefix), on both tau paths, for the three seed forms."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    R = 6
    ens = Ensemble(sim, R, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.model.events.ptr > 0 and all(ens.engine.counters(r).restarts == 0 for r in range(R))
    total = 0
    for s in seed_forms(R):
        ms = ens.tau_mutation_spectrum(seed=s)
        assert all(getattr(ms, k).dtype == np.int64 for k in BLOCKS)
        assert list(ms.replicates) == list(range(R)) and ms.passes >= 1 and len(ms.kernel_ms) == 2 and len(ms.stage_ms) == 3
        healthy, records = assert_rows_equal_genealogies(ens, ms, ens.tau_genealogies(seed=s))
        assert healthy >= 1, name
        total += records
        assert_derived_values(ms)
    print("%s %s: %d records" % (name, path, total))
    if name in RECORD_CASES:
        assert total >= 1, name
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix_and_restarted_replicates(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log; and replicates that restarted (no prefix for them) beside ones
    that did not, in one launch."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    for s in (None, 99):
        assert_rows_equal_genealogies(ens, ens.tau_mutation_spectrum(seed=s), ens.tau_genealogies(seed=s))
    ens.close()
    ens = Ensemble(_near_critical_warm(), 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    for s in (None, 99):
        ms = ens.tau_mutation_spectrum(seed=s)
        assert ms.passes == 1
        assert_rows_equal_genealogies(ens, ms, ens.tau_genealogies(seed=s))
    ens.close()


def test_subsets_order_and_passes(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    full = ens.tau_mutation_spectrum(seed=99)
    assert full.passes == 1
    healthy, records = assert_rows_equal_genealogies(ens, full, ens.tau_genealogies(seed=99))
    assert healthy > 100 and records >= 1
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_mutation_spectrum(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert assert_rows_equal_genealogies(ens, sub, ens.tau_genealogies(seed=seeds, replicates=order))[0] > 30
    same = ens.tau_mutation_spectrum(seed=99, replicates=order)
    for k in FIELDS[:-1]:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes: same kernels, same trees, same order
    small = ens.tau_mutation_spectrum(seed=99)
    assert small.passes > 1
    for k in FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    ens = _few_samples_ensemble()
    ms = ens.tau_mutation_spectrum(seed=5)
    batch = ens.tau_genealogies(seed=5)
    assert (ms.status == 1).any() and ms.ok.any() and np.array_equal(ms.status, batch.status), ms.status
    assert "Less than two" in ms.message(int(np.nonzero(ms.status == 1)[0][0]))
    assert_rows_equal_genealogies(ens, ms, batch)
    assert not any(getattr(ms, k)[~ms.ok].any() for k in BLOCKS)
    assert_derived_values(ms)
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match=r"tau_mutation_spectrum\(\).*simulate_tau"):
        ens.tau_mutation_spectrum()
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match=r"tau_mutation_spectrum\(\).*tau chains only"):
        ens.tau_mutation_spectrum()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match=r"tau_mutation_spectrum\(\).*record_events"):
        ens.tau_mutation_spectrum()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_mutation_spectrum(**kw)
    with pytest.raises(ValueError, match=r"mutation_spectrum\(\) walks direct chains only: the last call was simulate_tau"):
        ens.mutation_spectrum()   # the direct call still refuses tau chains with its own text
    one = ens.tau_mutation_spectrum(seed=1, replicates=[1])
    assert one.stats.shape == (1, 4) and list(one.replicates) == [1]
    none = ens.tau_mutation_spectrum(replicates=[])
    assert none.stats.shape == (0, 4) and none.spectrum.shape[0] == 0 and none.passes == 0
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    chains = [ens.replicate_events(r).copy() for r in range(ens.R)]
    before = ens.tau_genealogies(seed=5)
    first = ens.tau_mutation_spectrum(seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
        assert np.array_equal(chains[r], ens.replicate_events(r)), r
    after = ens.tau_genealogies(seed=5)
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
              "mig_offsets", "mig_node", "mig_old", "mig_new", "mig_time", "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    second = ens.tau_mutation_spectrum(seed=5)
    for k in FIELDS:
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    ens.close()
