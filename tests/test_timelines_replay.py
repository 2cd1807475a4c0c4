"""The log replay of the device pass (vgsim_amd/csrc/vgx_tline.h: which counters an event moves, the cut / bin rule, the query
table), compiled for the host and reached through vgx_test_timelines: the reference's goldens, random models and hand-made
chains against the literal restatement oracle/timelines.py, bit for bit; the 'compartment' semantics against the oracle
model's final state.  No GPU."""
import json
import os
import types

import numpy as np
import pytest

import helpers
from test_hip_fuzz import build as fuzz_build
from test_timelines_golden import _run

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DIRECT = [os.path.join(GOLDEN, "timeline_%s.npz" % c) for c in ("g9_short", "stress_h64")]
STEPS = (1, 7, 100)


def _replay(m, inf, sus, step_num, semantics="reference"):
    from vgsim_amd import _capi
    return _capi.replay_timelines(m, inf, sus, step_num, semantics)


def assert_equals_oracle(m, inf, sus, step_num, what):
    """The hook in 'reference' semantics == oracle/timelines.py, every array, dtype included."""
    from oracle import timelines
    got = _replay(m, inf, sus, step_num)
    for k, (p, h) in enumerate(inf):
        data, sample, tp, _ = timelines.get_data_infectious(m, None, p, h, step_num)
        assert got["infectious"][k].dtype == data.dtype and np.array_equal(got["infectious"][k], data), (what, "infectious", p, h, step_num)
        assert np.array_equal(got["samples"][k], sample), (what, "sample", p, h, step_num)
        assert np.array_equal(got["time_points"], np.asarray(tp, dtype=float)), (what, "time_points", step_num)
    for k, (p, s) in enumerate(sus):
        data, tp, _ = timelines.get_data_susceptible(m, None, p, s, step_num)
        assert got["susceptible"][k].dtype == data.dtype and np.array_equal(got["susceptible"][k], data), (what, "susceptible", p, s, step_num)
        assert np.array_equal(got["time_points"], np.asarray(tp, dtype=float))
    return got


@pytest.mark.parametrize("path", DIRECT, ids=[os.path.basename(p)[9:-4] for p in DIRECT])
def test_hook_matches_reference_golden(oracle_mod, path):
    meta, z, m = _run(oracle_mod, path)
    got = _replay(m, meta["inf"], meta["sus"], meta["steps"])
    for k in range(len(meta["inf"])):
        assert np.array_equal(got["infectious"][k], z["inf%d_data" % k]), (meta["case"], "infectious", k)
        assert np.array_equal(got["samples"][k], z["inf%d_sample" % k]), (meta["case"], "sample", k)
        assert np.array_equal(got["time_points"], z["inf%d_tp" % k]), (meta["case"], "time_points", k)
    for k in range(len(meta["sus"])):
        assert np.array_equal(got["susceptible"][k], z["sus%d_data" % k]), (meta["case"], "susceptible", k)


def _fuzz_chain(oracle_mod, seed):
    sim, n = fuzz_build(seed)
    m = sim.simulation
    assert oracle_mod.run_direct(m, n, 10 ** 9, -1, 200) == 0, "seed %d: the oracle run must succeed (no seed is skipped)" % seed
    rng = np.random.default_rng(5000 + seed)
    inf = [(int(rng.integers(0, m.popNum)), int(rng.integers(0, m.hapNum))) for _ in range(6)]
    sus = [(int(rng.integers(0, m.popNum)), int(rng.integers(0, m.susNum))) for _ in range(3)]
    occupied = np.argwhere(m.infectious > 0)
    if len(occupied):   # at least one compartment that is occupied at the end
        p, h = occupied[int(rng.integers(0, len(occupied)))]
        inf[0] = (int(p), int(h))
    return m, inf, sus


@pytest.mark.parametrize("seed", range(48))
def test_hook_equals_literal_replay_on_random_models(oracle_mod, seed):
    m, inf, sus = _fuzz_chain(oracle_mod, seed)
    for step_num in STEPS:
        got = assert_equals_oracle(m, inf, sus, step_num, "fuzz %d" % seed)
        if m.events.ptr == 0:   # an empty chain (seed 11): Data == [start, 0, 0, ...]
            assert got["last_point"] == 0
            for k, (p, h) in enumerate(inf):
                assert got["infectious"][k].tolist() == [float(m.initial_infectious[p, h])] + [0.0] * step_num


@pytest.mark.parametrize("seed", range(48))
def test_compartment_semantics_end_in_the_final_state(oracle_mod, seed):
    m, inf, sus = _fuzz_chain(oracle_mod, seed)
    everything = [(p, h) for p in range(m.popNum) for h in range(m.hapNum)]
    for step_num in STEPS:
        ref = _replay(m, inf, sus, step_num)
        got = _replay(m, inf, sus, step_num, "compartment")
        last = got["last_point"]
        assert last == ref["last_point"] and np.array_equal(got["time_points"], ref["time_points"])
        assert last == (step_num if m.events.ptr else 0)
        for k, (p, h) in enumerate(inf):
            assert got["infectious"][k, last] == m.infectious[p, h], (seed, "infectious", p, h, step_num)
            assert (got["infectious"][k, last:] == got["infectious"][k, last]).all() and (got["samples"][k, last:] == got["samples"][k, last]).all()
        for k, (p, s) in enumerate(sus):
            assert got["susceptible"][k, last] == m.susceptible[p, s], (seed, "susceptible", p, s, step_num)
            assert (got["susceptible"][k, last:] == got["susceptible"][k, last]).all()
            assert np.array_equal(got["susceptible"][k, :last + 1], ref["susceptible"][k, :last + 1])
        full = _replay(m, everything, [], step_num, "compartment")
        assert full["samples"][:, full["last_point"]].sum() == m.sCounter, (seed, step_num)
        assert np.array_equal(full["infectious"][:, full["last_point"]].reshape(m.popNum, m.hapNum), m.infectious)


# ---- hand-made chains: the cut rule alone ------------------------------------------------------------------------------------
def _chain(times, rows, current_time, P=2, H=4, S=2):
    """A model-shaped object holding a chain: rows = (type, haplotype, population, newHaplotype, newPopulation)."""
    from vgsim_amd._model import Events
    ev = Events()
    ev.CreateEvents(max(len(times), 1))
    ev.times[:len(times)] = times
    for j, name in enumerate(ev.COLUMNS):
        getattr(ev, name)[:len(times)] = [r[j] for r in rows]
    ev.ptr = len(times)
    init_i = np.arange(P * H, dtype=np.int64).reshape(P, H) + 10
    init_s = np.arange(P * S, dtype=np.int64).reshape(P, S) + 100
    loc = types.SimpleNamespace(states=[], times=[], populationsId=[])
    return types.SimpleNamespace(events=ev, currentTime=float(current_time), popNum=P, hapNum=H, susNum=S,
                                 initial_infectious=init_i, initial_susceptible=init_s, loc=loc)


def _compartment_literal(m, step_num, inf, sus):
    """The 'compartment' semantics written out as a loop: the reference's grid walk, the compartment's own events, and the value
    at the last reached index repeated after it."""
    ev = m.events
    tp = [i * m.currentTime / step_num for i in range(step_num + 1)]
    out_i = np.zeros((len(inf), step_num + 1)); out_s = np.zeros((len(inf), step_num + 1)); out_u = np.zeros((len(sus), step_num + 1))
    out_i[:, 0] = [m.initial_infectious[p, h] for p, h in inf]
    out_u[:, 0] = [m.initial_susceptible[p, s] for p, s in sus]
    point = 0
    for i in range(ev.ptr):
        while point != step_num and tp[point] < ev.times[i]:
            out_i[:, point + 1], out_s[:, point + 1], out_u[:, point + 1] = out_i[:, point], out_s[:, point], out_u[:, point]
            point += 1
        t, h, p, nh, npop = (int(getattr(ev, c)[i]) for c in ev.COLUMNS)
        for k, (qp, qh) in enumerate(inf):
            if t == 0 and (p, h) == (qp, qh):
                out_i[k, point] += 1
            if t in (1, 2) and (p, h) == (qp, qh):
                out_i[k, point] -= 1
                out_s[k, point] += t == 2
            if t == 3 and (p, h) == (qp, qh):
                out_i[k, point] -= 1
            if t == 3 and (p, nh) == (qp, qh):
                out_i[k, point] += 1
            if t == 5 and (npop, h) == (qp, qh):
                out_i[k, point] += 1
    for a in (out_i, out_s, out_u):
        a[:, point + 1:] = a[:, point:point + 1]
    return out_i, out_s, point


B, D, SA, MU, SC, MI = range(6)
ROWS = [(B, 1, 0, 0, 0), (D, 1, 0, 1, 0), (SA, 2, 1, 0, 0), (MU, 1, 0, 3, 0), (SC, 0, 1, 1, 0), (MI, 1, 0, 1, 1), (B, 3, 0, 1, 0), (SA, 1, 0, 0, 0),
        (MU, 3, 0, 1, 0), (MI, 3, 0, 0, 1), (D, 3, 1, 1, 0), (B, 1, 1, 1, 0)]
INF = [(0, 1), (0, 3), (1, 3), (1, 1), (0, 0)]
SUS = [(0, 0), (0, 1), (1, 1), (1, 0)]
HAND = {
    "equal_times": ([0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 2.5, 2.5, 2.5, 2.5, 4.0, 4.0], 4.0, (1, 4, 8)),
    "time_on_a_grid_point": ([1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 3.5, 4.0, 4.0, 4.0, 4.0], 4.0, (1, 2, 4, 8)),
    "times_go_back_after_a_restart": ([0.5, 3.0, 1.0, 1.5, 3.5, 0.2, 3.6, 3.7, 1.0, 3.9, 4.0, 4.0], 4.0, (1, 4, 16)),
    "current_time_far_past_the_last_event": ([0.1, 0.2, 0.7, 0.9, 1.1, 1.2, 1.3, 1.9, 2.0, 2.2, 2.3, 2.4], 10.0, (10, 7, 100)),
    "zero_current_time": ([0.0] * 12, 0.0, (1, 3)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_cut_rule_on_hand_made_chains(name):
    times, current_time, steps = HAND[name]
    m = _chain(times, ROWS, current_time)
    for step_num in steps:
        got = assert_equals_oracle(m, INF, SUS, step_num, name)
        comp = _replay(m, INF, SUS, step_num, "compartment")
        want_i, want_s, point = _compartment_literal(m, step_num, INF, SUS)
        assert got["last_point"] == comp["last_point"] == point
        assert np.array_equal(comp["infectious"], want_i) and np.array_equal(comp["samples"], want_s), (name, step_num)
        assert np.array_equal(comp["susceptible"][:, :point + 1], got["susceptible"][:, :point + 1])
        assert (comp["susceptible"][:, point:] == comp["susceptible"][:, point:point + 1]).all()
        if name == "current_time_far_past_the_last_event":
            assert 0 < point < step_num
            assert (got["infectious"][:, point + 1:] == 0).all() and (got["susceptible"][:, point + 1:] == 0).all()   # upstream's trailing zeros
            assert (comp["infectious"][:, point + 1:] == comp["infectious"][:, point:point + 1]).all()


def test_duplicate_and_empty_queries():
    m = _chain(HAND["equal_times"][0], ROWS, 4.0)
    got = _replay(m, [(0, 1), (1, 3), (0, 1)], [(1, 1), (1, 1)], 5)
    assert np.array_equal(got["infectious"][0], got["infectious"][2]) and np.array_equal(got["susceptible"][0], got["susceptible"][1])
    one = _replay(m, [(0, 1)], [], 5)
    assert np.array_equal(one["infectious"][0], got["infectious"][0]) and one["susceptible"].shape == (0, 6)
    none = _replay(m, [], [], 5)
    assert none["infectious"].shape == (0, 6) and none["last_point"] == got["last_point"] and np.array_equal(none["time_points"], got["time_points"])


def test_refusals():
    m = _chain(HAND["equal_times"][0], ROWS, 4.0)
    for kw, msg in ((dict(infectious=[(2, 0)]), "population index"), (dict(infectious=[(0, 4)]), "haplotype index"),
                    (dict(susceptible=[(0, 2)]), "group index"), (dict(step_num=0), "step_num"), (dict(semantics="other"), "semantics")):
        with pytest.raises(ValueError, match=msg):
            from vgsim_amd import _capi
            _capi.replay_timelines(m, **kw)


def test_tau_chain_is_refused(oracle_mod):
    """A MULTITYPE event with rows is not a direct chain (the tau golden's case is the input)."""
    z = np.load(os.path.join(GOLDEN, "timeline_tau_b.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    m = helpers.run_case_oracle(oracle_mod, meta["case"], record_multievents=True).simulation
    assert (m.events.types[:m.events.ptr] == 6).any()
    with pytest.raises(ValueError, match="MULTITYPE"):
        _replay(m, meta["inf"], meta["sus"], meta["steps"])
