"""The replay of tau chains behind Ensemble.tau_timelines (vgsim_amd/csrc/vgx_tline.h: the weighted-row rule and the cut search in
row index space; vgx_tau_timelines.hip: the flattening), compiled for the host and reached through vgx_test_tau_timelines: the
reference's tau golden, the oracle's tau chains (direct warm-up + tau steps, and direct -> tau -> direct) and hand-made chains
against the literal restatement oracle/timelines.py, bit for bit; the 'compartment' semantics against the oracle model's final
state.  No GPU.  Expected values never come from the code under test."""
import os

import numpy as np
import pytest

import helpers
from test_timelines_golden import _run
from test_timelines_replay import STEPS, _chain, _fuzz_chain, assert_equals_oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CHAINS = ("tau_a", "tau_b", "tau_c", "tau_d", "tau_then_direct")
MEV_COLUMNS = ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")
B, D, SA, MU, SC, MI, MULTI = range(7)


def _replay(m, mev, inf, sus, step_num, semantics="reference"):
    from vgsim_amd import _capi
    return _capi.replay_tau_timelines(m, inf, sus, step_num, semantics, mev=mev)


def assert_equals_literal(m, mev, inf, sus, step_num, what):
    """The hook in 'reference' semantics == oracle/timelines.py with the multievent rows, every array, dtype included."""
    from oracle import timelines
    got = _replay(m, mev, inf, sus, step_num)
    for k, (p, h) in enumerate(inf):
        data, sample, tp, _ = timelines.get_data_infectious(m, mev, p, h, step_num)
        assert got["infectious"][k].dtype == data.dtype and np.array_equal(got["infectious"][k], data), (what, "infectious", p, h, step_num)
        assert got["samples"][k].dtype == sample.dtype and np.array_equal(got["samples"][k], sample), (what, "sample", p, h, step_num)
        assert np.array_equal(got["time_points"], np.asarray(tp, dtype=float)), (what, "time_points", step_num)
    for k, (p, s) in enumerate(sus):
        data, tp, _ = timelines.get_data_susceptible(m, mev, p, s, step_num)
        assert got["susceptible"][k].dtype == data.dtype and np.array_equal(got["susceptible"][k], data), (what, "susceptible", p, s, step_num)
        assert np.array_equal(got["time_points"], np.asarray(tp, dtype=float))
    return got


def test_hook_matches_reference_golden(oracle_mod):
    """tau_b: a direct warm-up followed by tau steps, values recorded from the reference."""
    meta, z, m = _run(oracle_mod, os.path.join(GOLDEN, "timeline_tau_b.npz"))
    mev = oracle_mod.get_state(m).mev
    types_ = m.events.types[:m.events.ptr]
    assert (types_ == MULTI).any() and (types_ != MULTI).any()    # a mixed chain
    got = _replay(m, mev, meta["inf"], meta["sus"], meta["steps"])
    for k in range(len(meta["inf"])):
        assert np.array_equal(got["infectious"][k], z["inf%d_data" % k]), (meta["case"], "infectious", k)
        assert np.array_equal(got["samples"][k], z["inf%d_sample" % k]), (meta["case"], "sample", k)
        assert np.array_equal(got["time_points"], z["inf%d_tp" % k]), (meta["case"], "time_points", k)
    for k in range(len(meta["sus"])):
        assert np.array_equal(got["susceptible"][k], z["sus%d_data" % k]), (meta["case"], "susceptible", k)


_CHAIN_CACHE = {}


def _oracle_chain(oracle_mod, name):
    """(model, dense multievent columns, infectious queries, susceptible queries) of a case run on the oracle; made once."""
    if name not in _CHAIN_CACHE:
        m = helpers.run_case_oracle(oracle_mod, name, record_multievents=True).simulation
        mev = oracle_mod.get_state(m).mev
        rng = np.random.default_rng(900 + len(name) + sum(map(ord, name)))
        inf = [(int(rng.integers(0, m.popNum)), int(rng.integers(0, m.hapNum))) for _ in range(6)]
        occupied = np.argwhere(m.infectious > 0)
        assert len(occupied)
        p, h = occupied[int(rng.integers(0, len(occupied)))]
        inf[0] = (int(p), int(h))                                   # a compartment that is occupied at the end
        sus = [(p, s) for p in range(m.popNum) for s in range(m.susNum)]
        _CHAIN_CACHE[name] = (m, mev, inf, sus)
    return _CHAIN_CACHE[name]


@pytest.mark.parametrize("step_num", STEPS)
@pytest.mark.parametrize("name", CHAINS)
def test_hook_equals_literal_replay_on_oracle_chains(oracle_mod, name, step_num):
    m, mev, inf, sus = _oracle_chain(oracle_mod, name)
    t = m.events.types[:m.events.ptr]
    assert (t == MULTI).any() and (t != MULTI).any()
    if name == "tau_then_direct":
        assert t[-1] != MULTI and t[0] != MULTI                     # the tau steps lie inside the chain
    got = assert_equals_literal(m, mev, inf, sus, step_num, name)
    assert got["last_point"] == step_num


@pytest.mark.parametrize("name", CHAINS)
def test_compartment_semantics_end_in_the_final_state(oracle_mod, name):
    m, mev, _, sus = _oracle_chain(oracle_mod, name)
    everything = [(p, h) for p in range(m.popNum) for h in range(m.hapNum)]
    for step_num in STEPS:
        ref = _replay(m, mev, everything[:3], sus, step_num)
        got = _replay(m, mev, everything, sus, step_num, "compartment")
        last = got["last_point"]
        assert last == ref["last_point"] == step_num and np.array_equal(got["time_points"], ref["time_points"])
        assert np.array_equal(got["infectious"][:, last].reshape(m.popNum, m.hapNum), m.infectious), (name, step_num)
        assert np.array_equal(got["susceptible"][:, last].reshape(m.popNum, m.susNum), m.susceptible), (name, step_num)
        assert got["samples"][:, last].sum() == m.sCounter, (name, step_num)


# ---- hand-made chains -----------------------------------------------------------------------------------------------------------
def _tau_chain(events, rows, current_time, **kw):
    """events: (time, type, haplotype, population, newHaplotype, newPopulation), MULTITYPE ones carrying their [start, end) row range
    in (haplotype, population); rows: (num, type, haplotype, population, newHaplotype, newPopulation)."""
    m = _chain([e[0] for e in events], [e[1:] for e in events], current_time, **kw)
    mev = {c: np.array([r[j] for r in rows], dtype=np.int64) for j, c in enumerate(MEV_COLUMNS)}
    return m, mev


INF = [(0, 1), (0, 3), (1, 3), (1, 1), (0, 0), (1, 0)]
SUS = [(0, 0), (0, 1), (1, 1), (1, 0)]


def _both(m, mev, step_num, what):
    ref = assert_equals_literal(m, mev, INF, SUS, step_num, what)
    return ref, _replay(m, mev, INF, SUS, step_num, "compartment")


def test_a_step_without_rows_still_advances_point():
    """The third step lies EARLIER in time than the empty second one: only the empty step can have moved `point` to 3."""
    rows = [(3, B, 1, 0, 0, 0), (2, B, 1, 0, 0, 0)]
    events = [(0.5, MULTI, 0, 1, 0, 0), (2.5, MULTI, 1, 1, 0, 0), (0.6, MULTI, 1, 2, 0, 0)]
    m, mev = _tau_chain(events, rows, 4.0)
    ref, comp = _both(m, mev, 4, "empty step")
    start = float(m.initial_infectious[0, 1])
    assert ref["last_point"] == comp["last_point"] == 3
    assert ref["infectious"][0].tolist() == [start, start + 3, start + 3, start + 5, 0.0]
    assert comp["infectious"][0].tolist() == [start, start + 3, start + 3, start + 5, start + 5]
    # ... and as the chain's only event: last_point moves, no counter does
    m, mev = _tau_chain([(2.5, MULTI, 0, 0, 0, 0)], [], 4.0)
    ref, _ = _both(m, mev, 4, "only an empty step")
    assert ref["last_point"] == 3 and ref["infectious"][0].tolist() == [start] * 4 + [0.0]


def test_migration_row_keys_the_susceptible_series_as_upstream():
    """pyx:2037 tests the row's `haplotypes` against the group; the tau kernels write the migrant's group into newHaplotypes."""
    rows = [(4, MI, 1, 0, 0, 1)]                     # 4 migrants of haplotype 1 from population 0 into group 0 of population 1
    m, mev = _tau_chain([(1.0, MULTI, 0, 1, 0, 0)], rows, 1.0)   # (the chain ends at its only step: grid 0, 0.5, 1, the step in bin 2)
    ref, comp = _both(m, mev, 2, "migration row")
    s10, s11 = float(m.initial_susceptible[1, 0]), float(m.initial_susceptible[1, 1])
    assert ref["susceptible"][2].tolist() == [s11, s11, s11 - 4]           # (1, 1): keyed by haplotypes = 1
    assert ref["susceptible"][3].tolist() == [s10, s10, s10]
    assert comp["susceptible"][3].tolist() == [s10, s10, s10 - 4]          # (1, 0): where the migrants really went
    assert comp["susceptible"][2].tolist() == [s11, s11, s11]
    i11 = float(m.initial_infectious[1, 1])
    assert ref["infectious"][3].tolist() == comp["infectious"][3].tolist() == [i11, i11, i11 + 4]
    # the same record as a DIRECT event keeps the direct rule (pyx:2023: newHaplotypes)
    m, mev = _tau_chain([(1.0, MI, 1, 0, 0, 1)], [], 1.0)
    ref, _ = _both(m, mev, 2, "migration event")
    assert ref["susceptible"][3].tolist() == [s10, s10, s10 - 1] and ref["susceptible"][2].tolist() == [s11, s11, s11]


def test_mutation_row_onto_its_own_haplotype_only_decrements():
    rows = [(5, MU, 1, 0, 1, 0)]
    m, mev = _tau_chain([(1.0, MULTI, 0, 1, 0, 0)], rows, 1.0)
    ref, comp = _both(m, mev, 2, "mutation row")
    i01 = float(m.initial_infectious[0, 1])
    assert ref["infectious"][0].tolist() == [i01, i01, i01 - 5]
    assert comp["infectious"][0].tolist() == [i01, i01, i01]


def test_a_bin_sums_past_32_bits_exactly():
    """One bin receives num = 2^31 + 5 twice and 3 * 2^30, on a keyed counter and on the two query-independent rows."""
    big = 2 ** 31 + 5
    rows = [(big, B, 1, 0, 0, 0), (big, B, 1, 0, 0, 0), (3 * 2 ** 30, B, 1, 0, 0, 0),
            (big, SA, 3, 1, 1, 0), (big, SA, 3, 1, 1, 0), (3 * 2 ** 30, D, 3, 1, 1, 0)]
    events = [(1.0, MULTI, 0, 2, 0, 0), (1.1, MULTI, 2, 5, 0, 0), (1.2, MULTI, 5, 6, 0, 0)]
    m, mev = _tau_chain(events, rows, 4.0)
    total = 2 * big + 3 * 2 ** 30
    assert total > 2 ** 32
    for step_num in (2, 4):
        ref, comp = _both(m, mev, step_num, "wide counters")
        b = 1 if step_num == 2 else 2
        i01, i13 = int(m.initial_infectious[0, 1]), int(m.initial_infectious[1, 3])
        assert comp["infectious"][0][b] == float(i01 + total) and comp["infectious"][2][b] == float(i13 - total)
        assert comp["samples"][2][b] == float(2 * big) and comp["susceptible"][0][b] == float(int(m.initial_susceptible[0, 0]) - total)
        assert ref["infectious"][0][b] == float(i01 + total - total)       # every series takes every DEATH / SAMPLING
        assert ref["samples"][0][b] == float(2 * big)


def test_prefix_times_that_go_back_and_steps_after_them():
    """Direct events whose times go back (a chain continued after a Restart), then tau steps: the cut search over the running
    maximum of the shared times equals the literal loop."""
    direct = [(0.5, B, 1, 0, 0, 0), (3.0, D, 1, 0, 1, 0), (1.0, SA, 2, 1, 0, 0), (1.5, MU, 1, 0, 3, 0), (3.5, SC, 0, 1, 1, 0),
              (0.2, MI, 1, 0, 1, 1), (3.6, B, 3, 0, 1, 0), (3.6, SA, 1, 0, 0, 0)]
    rows = [(2, B, 1, 0, 0, 0), (1, SA, 3, 0, 1, 0), (7, MI, 3, 0, 1, 1), (2, SC, 0, 1, 1, 0), (0, D, 1, 1, 0, 0), (3, MU, 3, 0, 1, 0)]
    steps = [(3.7, MULTI, 0, 2, 0, 0), (5.0, MULTI, 2, 2, 0, 0), (5.5, MULTI, 2, 5, 0, 0), (8.0, MULTI, 5, 6, 0, 0)]
    for current_time in (8.0, 20.0, 3.0, 0.0):
        m, mev = _tau_chain(direct + steps, rows, current_time)
        for step_num in (1, 3, 16, 100):
            ref, comp = _both(m, mev, step_num, "times go back, currentTime %r" % current_time)
            assert ref["last_point"] == comp["last_point"]
    # the same events with a direct one at the end: no own steps, everything is prefix
    m, mev = _tau_chain(direct + steps + [(8.5, D, 1, 0, 1, 0)], rows, 9.0)
    for step_num in (1, 3, 16):
        _both(m, mev, step_num, "tau steps inside the chain")


def test_duplicate_and_empty_queries_and_refusals():
    rows = [(4, MI, 1, 0, 0, 1), (2, B, 1, 0, 0, 0)]
    m, mev = _tau_chain([(1.0, MULTI, 0, 2, 0, 0)], rows, 2.0)
    got = _replay(m, mev, [(0, 1), (1, 1), (0, 1)], [(1, 1), (1, 1)], 5)
    assert np.array_equal(got["infectious"][0], got["infectious"][2]) and np.array_equal(got["susceptible"][0], got["susceptible"][1])
    none = _replay(m, mev, [], [], 5)
    assert none["infectious"].shape == (0, 6) and none["last_point"] == got["last_point"]
    for kw, msg in ((dict(inf=[(2, 0)]), "population index"), (dict(inf=[(0, 4)]), "haplotype index"), (dict(sus=[(0, 2)]), "group index"),
                    (dict(step_num=0), "step_num"), (dict(semantics="other"), "semantics")):
        args = dict(inf=[], sus=[], step_num=5, semantics="reference")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            _replay(m, mev, args["inf"], args["sus"], args["step_num"], args["semantics"])
    bad = dict(mev)
    with pytest.raises(ValueError, match="row range"):
        _replay(_tau_chain([(1.0, MULTI, 0, 3, 0, 0)], rows, 2.0)[0], bad, [(0, 1)], [], 5)


# ---- the direct path is what it was ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(48))
def test_direct_hook_unchanged_on_random_models(oracle_mod, seed):
    """vgx_tl_classify and vgx_test_timelines keep their behaviour next to the weighted-row rule: replay_timelines == the literal
    replay on the fuzz models; and on a direct chain the tau hook gives the same."""
    from vgsim_amd import _capi
    m, inf, sus = _fuzz_chain(oracle_mod, seed)
    empty = {c: np.zeros(0, dtype=np.int64) for c in MEV_COLUMNS}
    for step_num in STEPS:
        got = assert_equals_oracle(m, inf, sus, step_num, "fuzz %d" % seed)
        same = _capi.replay_tau_timelines(m, inf, sus, step_num, mev=empty)
        for k in ("time_points", "infectious", "samples", "susceptible"):
            assert np.array_equal(got[k], same[k]), (seed, step_num, k)
        assert got["last_point"] == same["last_point"]
