"""Ensemble.genealogies(): the backward pass of every replicate on the device (vgx_get_genealogies), bit for bit what the
per-replicate host path Ensemble.genealogy(r, seed) gives — every key, rng_raw included — for the three seed forms, every
direct kernel's final state, partly filled wavefronts, subsets, several device passes, and replicates whose walk fails."""
import numpy as np
import pytest

import helpers
import models

pytestmark = pytest.mark.gpu

KEYS = ("tree", "tree_pop", "times", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
        "mig_node", "mig_time", "mig_old", "mig_new", "nodes_used", "rng_raw")


def _ensemble(name, R, n_max=3000, seeds0=100, **kw):
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, name)
        setup, ph = phases[0]
        setup(sim)
    ens = Ensemble(sim, R, seeds=seeds0 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        ens.simulate(min(ph["iterations"], n_max), sample_size=10 ** 9, attempts=ph.get("attempts", 200), record_events=True, **kw)
    return ens


def _seed_of(seed, i):
    return seed if seed is None or np.isscalar(seed) else int(seed[i])


def assert_batch_equals_host(ens, batch, seed):
    """Every row of the batch against Ensemble.genealogy(r, seed_r): same dict, or the same exception."""
    healthy = 0
    for i, r in enumerate(batch.replicates):
        s = _seed_of(seed, i)
        try:
            want = ens.genealogy(int(r), s)
        except RuntimeError as e:
            assert batch.status[i] != 0, "replicate %d: the host path raised %r, the batch did not" % (r, str(e))
            with pytest.raises(RuntimeError) as got:
                batch.replicate(int(r))
            assert str(got.value) == str(e), "replicate %d" % r
            continue
        assert batch.status[i] == 0, "replicate %d: %s" % (r, batch.message(i))
        got = batch.replicate(int(r))
        assert set(got) == set(want)
        for k in KEYS:
            if k in ("nodes_used", "rng_raw"):
                assert got[k] == want[k], "replicate %d %s" % (r, k)
            else:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), "replicate %d %s" % (r, k)
        healthy += 1
    return healthy


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70", "extinct_restart"])
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_batch_equals_per_replicate_host_pass(name, seed):
    R = 6
    ens = _ensemble(name, R)
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    batch = ens.genealogies(seed=s)
    assert list(batch.replicates) == list(range(R)) and batch.passes >= 1
    healthy = assert_batch_equals_host(ens, batch, s)
    assert healthy > 0 or name == "extinct_restart"   # (its replicates die out early: statuses and messages are what is compared)
    ens.close()


def test_every_direct_kernels_final_state_is_read():
    ran = set()
    for kernel in ("wave", "lane", "quad", "quadg", "solo", "lone"):
        try:
            ens = _ensemble("g5_short", 4, n_max=2000, kernel=kernel)
        except Exception:   # a kernel that does not take the model
            continue
        ran.add(ens.engine.last_kernel)
        batch = ens.genealogies(seed=None)
        assert assert_batch_equals_host(ens, batch, None) > 0, kernel
        ens.close()
    assert {"wave", "quad", "quadg", "solo"} <= ran, ran


def test_partial_wavefront_subsets_and_passes(monkeypatch):
    R = 130
    ens = _ensemble("g9_short", R, n_max=1500, seeds0=7000)
    full = ens.genealogies(seed=99)
    assert assert_batch_equals_host(ens, full, 99) > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.genealogies(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_batch_equals_host(ens, sub, seeds)
    lane = ens.genealogies(seed=99, layout="lane")   # the one-replicate-per-lane layout: the same walk
    for k in ("status", "node_offsets", "tree", "times", "mut_node", "mig_time", "rng_raw"):
        assert np.array_equal(getattr(lane, k), getattr(full, k)), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "200000")   # several device passes
    small = ens.genealogies(seed=99)
    assert small.passes > 1
    for k in ("status", "node_offsets", "tree", "times", "mut_offsets", "mut_time", "mig_offsets", "mig_node", "rng_raw"):
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_failed_replicates_do_not_fail_the_call():
    ens = _ensemble("recomb_a", 8, n_max=3000)
    batch = ens.genealogies(seed=21)
    assert (batch.status == 4).any(), batch.status           # lineages that never coalesce
    assert "never coalesced" in batch.message(int(np.nonzero(batch.status == 4)[0][0]))
    assert_batch_equals_host(ens, batch, 21)
    ens.close()
    ens = _ensemble("extinct", 24, n_max=50, seeds0=1)
    batch = ens.genealogies(seed=5)
    assert (batch.status == 1).any(), batch.status           # fewer than two samples
    assert_batch_equals_host(ens, batch, 5)
    ens.close()


def test_refusals():
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    ens = _ensemble("g9_short", 2, n_max=500)
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.genealogies()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match="tau"):
        ens.genealogies()
    ens.close()
    with helpers.quiet():   # a model that already holds events when the ensemble starts
        sim, phases = models.build(Simulator, "g9_short")
        phases[0][0](sim)
        sim.simulate(300)
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with helpers.quiet():
        ens.simulate(300, sample_size=10 ** 9, record_events=True)
    if all(ens.engine.counters(r).ev_first_new != 0 for r in range(2)):
        with pytest.raises(ValueError, match="does not start"):
            ens.genealogies(seed=1)
    else:   # (a replicate that restarted rewinds its log to 0)
        with pytest.raises(ValueError, match="does not start"):
            ens.genealogies(seed=1, replicates=[r for r in range(2) if ens.engine.counters(r).ev_first_new != 0])
    ens.close()
