"""Ensemble.tau_genealogies(): the backward pass of every replicate of a tau ensemble on the device (vgx_get_tau_genealogies).  Every
row of the batch equals Ensemble.tau_genealogy(r, seed_r) — the host pass vgx_get_genealogy on the replicate's whole chain in the
reference's layout — on every key, all six rng_raw words included, or raises the same message; and equals the expectation
assembled here from read-outs that exist without this feature (replicate_events, engine.multievents, canonical_multievents,
replicate_state, _capi.get_genealogy).  Both tau paths, the three seed forms, chains with and without a prefix, restarted
replicates, subsets, partly filled passes, several passes, and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import KEYS, _seed_of
from test_hip_ensemble_tau_timelines import SEEDS, _fresh, _near_critical_warm, queries
from test_hip_tau_trajectories import PATHS, warm
from test_tau_genealogy_walk import HYPER_DRAWS, HYPER_SETS, HYPER_SETS_WIDE, hyper_starts

pytestmark = pytest.mark.gpu

MULTI = 6
EV_COLUMNS = ("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")


def expected(ens, r, seed):
    """The host pass on the whole chain of replicate r, assembled from the read-outs of the engine and the model's own log."""
    from vgsim_amd import _capi
    from vgsim_amd._model import Events, MultiEvents
    eng, model = ens.engine, ens.model
    c = eng.counters(r)
    restarted = c.restarts > 0
    n_pre = 0 if restarted else int(model.events.ptr)
    k_pre = 0 if restarted else int(model.multievents.ptr)
    assert c.ev_first_new == n_pre
    own = ens.replicate_events(r)[:, n_pre:]
    assert (own[1] == MULTI).all()
    starts, ends = own[2].astype(np.int64), own[3].astype(np.int64)
    rows = _capi.canonical_multievents(eng.multievents(r), starts, ends, model.sites, model.susNum)
    m = ens.replicate_state(r)
    n = n_pre + own.shape[1]
    ev = Events()
    ev.CreateEvents(max(n, 1))
    ev.times[:n] = np.concatenate((model.events.times[:n_pre], own[0]))
    ev.types[:n] = np.concatenate((model.events.types[:n_pre], np.full(own.shape[1], MULTI)))
    ev.haplotypes[:n] = np.concatenate((model.events.haplotypes[:n_pre], starts + k_pre))
    ev.populations[:n] = np.concatenate((model.events.populations[:n_pre], ends + k_pre))
    ev.newHaplotypes[:n_pre], ev.newPopulations[:n_pre] = model.events.newHaplotypes[:n_pre], model.events.newPopulations[:n_pre]
    ev.ptr = n
    mv = MultiEvents()
    mv.extend(np.concatenate((model.multievents.times[:k_pre], rows["times"])),
              **{k: np.concatenate((getattr(model.multievents, k)[:k_pre], rows[k])) for k in mv.COLUMNS})
    m.events, m.multievents = ev, mv
    m.user_seed = int(ens.seeds[r])
    return _capi.get_genealogy(m, seed, rng_position=(0, 0))


def assert_batch_equals_host(ens, batch, seed, own_expectation=True):
    """Every row of the batch against Ensemble.tau_genealogy(r, seed_r) and the expectation assembled here: the same dict, or the same
    exception.  Returns the number of healthy rows.  (The expectation assembled here calls vgx_get_genealogy unguarded, which reads
    and writes outside its lists on a row numpy's hypergeometric would refuse: it runs only where tau_genealogy, which walks the
    chain with the device pass's guards first, returned.)"""
    healthy = 0
    for i, r in enumerate(batch.replicates):
        s = _seed_of(seed, i)
        try:
            wants = [ens.tau_genealogy(int(r), s)]
        except RuntimeError as e:
            assert batch.status[i] != 0, "replicate %d: the host path raised %r, the batch did not" % (r, str(e))
            with pytest.raises(RuntimeError) as got:
                batch.replicate(int(r))
            assert str(got.value) == str(e), "replicate %d" % r
            continue
        if own_expectation:
            wants.append(expected(ens, int(r), s))
        assert batch.status[i] == 0, "replicate %d: %s" % (r, batch.message(i))
        got = batch.replicate(int(r))
        for want in wants:
            assert set(got) == set(want)
            for k in KEYS:
                if k in ("nodes_used", "rng_raw"):
                    assert got[k] == want[k], "replicate %d %s" % (r, k)
                else:
                    assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), "replicate %d %s" % (r, k)
        healthy += 1
    return healthy


def seed_forms(n):
    return (None, 4711, np.arange(n, dtype=np.int64) * 7 + 3)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_batch_equals_the_host_pass_on_the_whole_chain(name, path, monkeypatch):
    """A tau call that continues a direct warm-up (the prefix), on both tau paths, for the three seed forms."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    R = 6
    ens = Ensemble(sim, R, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.model.events.ptr > 0 and all(ens.engine.counters(r).restarts == 0 for r in range(R))
    for s in seed_forms(R):
        batch = ens.tau_genealogies(seed=s)
        assert list(batch.replicates) == list(range(R)) and batch.passes >= 1
        assert batch.rng_raw.shape == (R, 6)
        assert assert_batch_equals_host(ens, batch, s) > 0, name
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log; and replicates that restarted (no prefix for them) beside ones
    that did not."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    for s in (None, 99):
        assert_batch_equals_host(ens, ens.tau_genealogies(seed=s), s)
    ens.close()
    sim = _near_critical_warm()
    ens = Ensemble(sim, 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    for s in (None, 99):
        batch = ens.tau_genealogies(seed=s)
        assert_batch_equals_host(ens, batch, s)
    ens.close()


def test_subsets_partial_passes_and_chunks(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    full = ens.tau_genealogies(seed=99)
    assert full.passes == 1 and (full.status == 0).sum() > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_genealogies(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert assert_batch_equals_host(ens, sub, seeds, own_expectation=False) > 30
    same = ens.tau_genealogies(seed=99, replicates=order)
    for i, r in enumerate(order):
        a, b = same.replicate(int(r)), full.replicate(int(r))
        assert all(np.array_equal(a[k], b[k]) for k in KEYS), r
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes
    small = ens.tau_genealogies(seed=99)
    assert small.passes > 1
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_time", "mig_offsets", "mig_node", "mig_time",
              "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    off, allrows = ens.replicate_multievents()
    states = ens.replicate_states_tau()
    inf, sus = queries(ens, states)
    tl = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=50)
    first = ens.tau_genealogies(seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
    off2, allrows2 = ens.replicate_multievents()
    assert np.array_equal(off, off2) and all(np.array_equal(allrows[k], allrows2[k]) for k in allrows)
    tl2 = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=50)
    for k in ("time_points", "infectious", "samples", "susceptible", "last_point"):
        assert np.array_equal(getattr(tl, k), getattr(tl2, k)), k
    for a, b in zip(states, ens.replicate_states_tau()):
        assert np.array_equal(a, b)
    second = ens.tau_genealogies(seed=5)
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
              "mig_offsets", "mig_node", "mig_old", "mig_new", "mig_time", "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    ens.close()


def test_device_sampler_equals_its_host_instance():
    """numpy's hypergeometric sampler as the walk kernel draws it: bit for bit the host build of the same code, final generator state
    included, on the parameter sets the host build is pinned on."""
    from vgsim_amd import _capi
    for good, bad, sample in HYPER_SETS + HYPER_SETS_WIDE:
        for start in hyper_starts(good):
            want, end = _capi.hypergeometric(good, bad, sample, HYPER_DRAWS, start, on_device=False)
            got, end_dev = _capi.hypergeometric(good, bad, sample, HYPER_DRAWS, start, on_device=True)
            assert np.array_equal(got, want) and end_dev == end, (good, bad, sample)


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_genealogies()
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_genealogies()
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_genealogy(0, 1)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_genealogies()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_genealogies(**kw)
    with pytest.raises(ValueError, match="direct chains only"):   # the direct call's pass still refuses tau chains
        ens.genealogies()
    assert len(ens.tau_genealogies(seed=1, replicates=[1])) == 1
    ens.close()
