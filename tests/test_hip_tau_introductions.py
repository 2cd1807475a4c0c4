"""Ensemble.tau_introductions(): the rows of tau ensembles against the host sweep ``_capi.introductions`` (the definition) applied
to the trees and node labels ``tau_genealogies()`` returns for the same walks, for equality; status, the six generator words and
messages of ``tau_genealogies()``; both tau paths, the three seed forms, chains with and without a prefix, restarted replicates,
subsets, order, several passes, failed walks, refusals and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_introductions import BLOCKS, FIELDS, assert_derived_values
from test_hip_tau_tree_shapes import PATHS, SEEDS, _few_samples_ensemble, _fresh, _near_critical_warm, seed_forms, warm
from test_introductions_rule import assert_identities
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu


def assert_rows_equal_genealogies(ens, it, batch):
    """Every row against the host sweep over the tree and labels tau_genealogies() returns for the same walk.  Returns (healthy
    rows, introductions in them)."""
    healthy = intro = 0
    P = int(ens.model.popNum)
    n = len(it.replicates)
    assert it.pops == P and it.tips_by_pop.shape == (n, P) and it.imports.shape == (n, P, P) and it.into.shape == (n, P, 6)
    assert it.spectrum.shape == (n, P, 32) and it.stats.shape == (n, 8)
    assert np.array_equal(it.status, batch.status) and np.array_equal(it.status_arg, batch.status_arg)
    assert it.rng_raw.shape == (n, 6) and np.array_equal(it.rng_raw, batch.rng_raw)
    assert np.array_equal(it.replicates, batch.replicates)
    for i, r in enumerate(it.replicates):
        assert it.message(i) == batch.message(i)
        if not it.ok[i]:
            assert not any(getattr(it, k)[i].any() for k in BLOCKS), r
            continue
        g = batch.replicate(int(r))
        want = _capi.introductions(g["tree"], g["tree_pop"], P)
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(it, k)[i], w), (r, k, getattr(it, k)[i], w)
        assert_identities(tuple(getattr(it, k)[i] for k in BLOCKS), r)
        assert it.tips[i] == ens.engine.counters(int(r)).reserved[4], r
        healthy += 1
        intro += int(it.introductions[i])
    return healthy, intro


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_b", "tau_c", "tau_d"])
def test_rows_equal_the_host_sweep_over_tau_genealogies(name, path, monkeypatch):
    """A tau call that continues a direct warm-up (the prefix), on both tau paths, for the three seed forms."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    R = 6
    ens = Ensemble(sim, R, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.model.events.ptr > 0 and all(ens.engine.counters(r).restarts == 0 for r in range(R))
    for s in seed_forms(R):
        it = ens.tau_introductions(seed=s)
        assert all(getattr(it, k).dtype == np.int64 for k in BLOCKS)
        assert list(it.replicates) == list(range(R)) and it.passes >= 1 and len(it.kernel_ms) == 2 and len(it.stage_ms) == 3
        healthy, intro = assert_rows_equal_genealogies(ens, it, ens.tau_genealogies(seed=s))
        print("%s %s: %d healthy of %d, %d introductions" % (name, path, healthy, R, intro))
        assert 4 * healthy >= 3 * R, name
        assert intro > 0, name   # (the comparison is not of zeros)
        assert_derived_values(it)
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
        assert_rows_equal_genealogies(ens, ens.tau_introductions(seed=s), ens.tau_genealogies(seed=s))
    ens.close()
    ens = Ensemble(_near_critical_warm(), 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    for s in (None, 99):
        it = ens.tau_introductions(seed=s)
        assert it.passes == 1
        assert_rows_equal_genealogies(ens, it, ens.tau_genealogies(seed=s))
    ens.close()


def test_subsets_order_and_passes(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    full = ens.tau_introductions(seed=99)
    assert full.passes == 1
    healthy, intro = assert_rows_equal_genealogies(ens, full, ens.tau_genealogies(seed=99))
    assert 4 * healthy >= 3 * R and intro > 0
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_introductions(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    healthy, intro = assert_rows_equal_genealogies(ens, sub, ens.tau_genealogies(seed=seeds, replicates=order))
    assert 4 * healthy >= 3 * 40 and intro > 0
    same = ens.tau_introductions(seed=99, replicates=order)
    for k in FIELDS[:-1]:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes: same kernels, same trees, same order
    small = ens.tau_introductions(seed=99)
    assert small.passes > 1
    for k in FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    ens = _few_samples_ensemble()
    it = ens.tau_introductions(seed=5)
    batch = ens.tau_genealogies(seed=5)
    assert (it.status == 1).any() and it.ok.any() and np.array_equal(it.status, batch.status), it.status
    assert "Less than two" in it.message(int(np.nonzero(it.status == 1)[0][0]))
    assert_rows_equal_genealogies(ens, it, batch)
    assert not any(getattr(it, k)[~it.ok].any() for k in BLOCKS)
    assert_derived_values(it)
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match=r"tau_introductions\(\).*simulate_tau"):
        ens.tau_introductions()
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match=r"tau_introductions\(\).*tau chains only"):
        ens.tau_introductions()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match=r"tau_introductions\(\).*record_events"):
        ens.tau_introductions()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_introductions(**kw)
    with pytest.raises(ValueError, match=r"introductions\(\) walks direct chains only: the last call was simulate_tau"):
        ens.introductions()   # the direct call still refuses tau chains with its own text
    one = ens.tau_introductions(seed=1, replicates=[1])
    assert one.stats.shape == (1, 8) and list(one.replicates) == [1]
    none = ens.tau_introductions(replicates=[])
    assert none.stats.shape == (0, 8) and none.imports.shape[0] == 0 and none.passes == 0
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    chains = [ens.replicate_events(r).copy() for r in range(ens.R)]
    before = ens.tau_genealogies(seed=5)
    first = ens.tau_introductions(seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
        assert np.array_equal(chains[r], ens.replicate_events(r)), r
    after = ens.tau_genealogies(seed=5)
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mig_offsets", "mig_node", "mig_old", "mig_new", "mig_time",
              "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    second = ens.tau_introductions(seed=5)
    for k in FIELDS:
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    ens.close()
