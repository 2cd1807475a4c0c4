"""vgx_quad_kernel keeps, per replicate, the end-of-tile running sums of ONE multi-tile list in a register (vgx_quad.hip: written
by the long-form rate refresh, read by the next haplotype choice in that population, dropped when the list falls back to the
register path, on a rebuild and on a Restart).  Whole calls on that kernel against the CPU oracle, bit for bit: a model whose four
lists all grow to several tiles (the register moves between populations, migrants are chosen from multi-tile lists), one whose
lists hover around one tile (the register is dropped and refilled), and one that restarts.  Six replicates: one full wavefront and
one with two idle rows."""
import ctypes as C

import numpy as np
import pytest

import helpers
import models
from test_hip_quad_lists import _grow_model, _lists_ok, _oracle_copy

pytestmark = pytest.mark.gpu

R = 6
SEEDS = 300 + np.arange(R, dtype=np.int64)


def _hover_model(seed=2020):
    """The shape of _grow_model with 64 / 63 / 64 / 60 occupied haplotypes of one carrier each (population 0: 63 and the index case
    the first call puts on haplotype 0) and births level with removals: the lists wander around the 64 entries of one tile."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        s = Simulator(number_of_sites=8, populations_number=4, number_of_susceptible_groups=1, seed=seed)
    s.set_transmission_rate(1.0); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1)
    s.set_mutation_rate(0.3); s.set_total_migration_probability(0.05); s.set_population_size(10 ** 6)
    m = s.simulation
    rng = np.random.default_rng(11)
    for pn, occ in enumerate((63, 63, 64, 60)):
        haps = 1 + rng.choice(m.hapNum - 1, size=occ, replace=False)
        m.infectious[pn, haps] = 1
        m.susceptible[pn, 0] -= int(m.infectious[pn].sum())
    m.set_mutation_rate(0.3, None, None)
    return s


def _list_lengths(final, chain, step):
    """The number of occupied haplotypes of every population after every `step` events of a chain that ends in the state `final`
    (rows: time, type, haplotype, population, new haplotype, new population), and the state the chain started from."""
    ty, hp, pp, nh, npp = (chain[i].astype(np.int64) for i in range(1, 6))
    moves = []                                   # (event, population, haplotype, +-1)
    for k in range(chain.shape[1]):
        t = ty[k]
        if t == 0: moves.append((k, pp[k], hp[k], 1))                                # birth
        elif t in (1, 2): moves.append((k, pp[k], hp[k], -1))                        # death, sampling
        elif t == 3: moves += [(k, pp[k], hp[k], -1), (k, pp[k], nh[k], 1)]          # mutation
        elif t == 5: moves.append((k, npp[k], hp[k], 1))                             # migration into the new population
        else: raise AssertionError("event type %d" % t)
    inf = final.copy()
    for _, p, h, d in moves:
        inf[p, h] -= d
    start = inf.copy()
    assert (start >= 0).all()
    nocc = [int(np.count_nonzero(inf[p])) for p in range(inf.shape[0])]
    out, i = [list(nocc)], 0
    for k in range(chain.shape[1]):
        while i < len(moves) and moves[i][0] == k:
            _, p, h, d = moves[i]
            was = int(inf[p, h])
            inf[p, h] = was + d
            nocc[p] += int(was == 0) - int(was + d == 0)
            i += 1
        if (k + 1) % step == 0:
            out.append(list(nocc))
    assert np.array_equal(inf, final)
    return np.array(out), start


def _run_and_compare(oracle_mod, sim, n_events, what):
    """R replicates of `sim` on the row kernel against the oracle's runs, bit for bit; returns the ensemble and the oracle's models."""
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(sim, R, seeds=SEEDS)
    res = ens.simulate(n_events, sample_size=10 ** 9, record_events=True, kernel="quad")
    assert ens.engine.lib.vgx_last_direct_kernel(ens.engine.handle) == 3
    refs = []
    for r in range(R):
        ref = _oracle_copy(sim.simulation, SEEDS[r])
        assert oracle_mod.run_direct(ref, n_events, 10 ** 9, -1, 200, sparse=True) == 0
        chain = ens.replicate_events(r)
        assert res.events[r] == ref.events.ptr
        assert np.array_equal(chain, ref.events.as_array()[:, :ref.events.ptr]), "%s, replicate %d: %s" % (
            what, r, helpers.describe_first_diff(chain, ref.events.as_array(), ref.events.ptr))
        st = ens.replicate_state(r)
        assert np.array_equal(st.infectious, ref.infectious) and np.array_equal(st.susceptible, ref.susceptible)
        assert st.currentTime == ref.currentTime
        refs.append(ref)
    return ens, refs


def _tile_sums_ok(ens, refs):
    """The integer tile sums the call left (what a migrant's haplotype is chosen by, and what the other kernels find) against the
    state's counts: the sum of every 64-entry tile of every list, 0 behind it."""
    eng = ens.engine
    capT = C.c_int64(0)
    eng._check(eng.lib.vgx_get_list_tile_sums(eng.handle, 0, 0, 0, None, C.byref(capT)))
    capT = capT.value
    assert capT > 0
    checked = 0
    for r, ref in enumerate(refs):
        for pn in range(ref.popNum):
            occ = ref.infectious[pn][ref.infectious[pn] != 0]
            n = len(occ)
            out = np.full(capT, -1, dtype=np.int64)
            eng._check(eng.lib.vgx_get_list_tile_sums(eng.handle, r, pn, capT, out.ctypes.data_as(C.POINTER(C.c_int64)), None))
            want = np.zeros(capT, dtype=np.int64)
            for t in range((n + 63) // 64):
                want[t] = occ[64 * t:64 * t + 64].sum()
            assert np.array_equal(out, want), "replicate %d population %d (n = %d): tile sums %r, counts give %r" % (
                r, pn, n, out[:8], want[:8])
            checked += 1
    return checked


def test_tile_cache_growing_lists_vs_oracle(oracle_mod):
    sim = _grow_model()
    N = 4000
    ens, refs = _run_and_compare(oracle_mod, sim, N, "growing lists")
    for r, ref in enumerate(refs):
        lengths, start = _list_lengths(ref.infectious, ref.events.as_array()[:, :ref.events.ptr], 5)
        # several multi-tile lists per replicate: every list starts within one tile, crosses 64, 128 and 192 entries somewhere
        # among the four and ends at 150 entries or more, within four tiles (seed 304's longest ends at 252 entries); the migrants
        # come from multi-tile lists
        assert lengths[0].max() <= 64
        assert (lengths[-1] >= 150).all() and (lengths[-1] <= 256).all(), lengths[-1]
        assert lengths[-1].max() > 192
        assert 100 <= ref.migPlus <= 130, ref.migPlus
    assert _lists_ok(ens, "growing lists") > 192
    assert _tile_sums_ok(ens, refs) == 4 * R
    ens.close()


def test_tile_cache_then_wave_kernel_vs_oracle(oracle_mod):
    """A further call from the state the row kernel left, on the one-replicate-per-wavefront kernel: it reads the 8-byte counts,
    which the row kernel does not keep (they are widened from the 4-byte ones), and the tile sums it rewrote when it left."""
    hip, ref = _grow_model(2021), _grow_model(2021)
    for n, kernel in ((4000, "quad"), (600, "wave")):
        with helpers.quiet():
            hip.simulate(n, sample_size=10 ** 9, kernel=kernel)
        assert oracle_mod.run_direct(ref.simulation, n, 10 ** 9, -1, 200, sparse=True) == 0
    helpers.assert_models_equal(hip.simulation, ref.simulation, "quad, then wave")
    assert max(np.count_nonzero(ref.simulation.infectious[pn]) for pn in range(4)) > 128


def test_tile_cache_hovering_lists_vs_oracle(oracle_mod):
    sim = _hover_model()
    ens, refs = _run_and_compare(oracle_mod, sim, 3000, "hovering lists")
    # Lists cross the 64 entries of one tile in both directions, counted every 5 events along the oracle's chain of the call (the
    # oracle run 5 events at a time opens a new random stream with every call and follows another path): with this start state
    # 18/16, 5/5, 12/12, 2/2, 7/6 and 10/10 times up / down for seeds 300 .. 305.
    for r in range(R):
        lengths, start = _list_lengths(refs[r].infectious, refs[r].events.as_array()[:, :refs[r].events.ptr], 5)
        assert lengths[0].max() <= 64        # (the call starts on the short-list form)
        up = int(((lengths[:-1] <= 64) & (lengths[1:] > 64)).sum())
        down = int(((lengths[:-1] > 64) & (lengths[1:] <= 64)).sum())
        assert up >= 2 and down >= 2, (int(SEEDS[r]), up, down)
    _lists_ok(ens, "hovering lists")
    _tile_sums_ok(ens, refs)
    ens.close()


def test_tile_cache_restarts_vs_oracle(oracle_mod):
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    name, n_events = "extinct_restart", 1000
    with helpers.quiet():
        sim, phases = models.build(Simulator, name)
    phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=SEEDS)
    res = ens.simulate(n_events, sample_size=10 ** 9, record_events=True, kernel="quad")
    _lists_ok(ens, name)
    for r in range(R):
        ctor, ph = models.CASES[name]
        with helpers.quiet():
            one = Simulator(**dict(ctor, seed=int(SEEDS[r])))
        ph[0][0](one)
        m = one.simulation
        assert oracle_mod.run_direct(m, n_events, 10 ** 9, -1, 200) == 0
        assert res.events[r] == m.events.ptr
        assert np.array_equal(ens.replicate_events(r), m.events.as_array()[:, :m.events.ptr]), "replicate %d" % r
    assert res.restarts.sum() > 0
    ens.close()
