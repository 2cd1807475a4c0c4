"""Lineages on a grid for TAU chains (vgsim_amd/csrc/vgx_tau_lineages.h, vgx_gwalk_tau.h) against a pure-Python
restatement of the tau walk that records lineage records as it goes.  The restatement draws from numpy's PCG64 (``hypergeometric``
and ``random``) and is pinned twice: its tree is the one ``_capi.tau_genealogy_walk`` returns for the same chain and seed, and
``_capi.replay_tau_lineages`` (the device's walk, observer, tile walk and suffix sum compiled for the host) gives its values, root
and record count exactly.  Chains and seeds: the (chain, seed) pairs on which test_tau_genealogy_walk.py asserts that the walk
equals the libm host pass (the three reference tau trees, its continued chains, its 16 random models).  No GPU."""
import copy
import functools
import math
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import load
from test_hip_fuzz import build as fuzz_build
from test_lineages_rule import MOVE, MUT, SPLIT, TIP, _div, alive, cuts, grids, maps, py_lineages
from test_tau_genealogy_walk import FUZZ, GOLD, _more_migrants_than_sources, decanonicalised, trailing_steps

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION, MULTI = range(7)


def numpy_generator(seed, raw=None):
    """numpy's generator where the walk starts: seeded as the reference seeds it, or set to six raw words (PCG64 state hi, lo,
    increment hi, lo, has_uint32, uinteger)."""
    bg = np.random.PCG64(np.random.SeedSequence(0 if seed is None else seed, spawn_key=(0,)))
    if seed is None:
        s = bg.state
        s["state"]["state"], s["state"]["inc"] = (int(raw[0]) << 64) | int(raw[1]), (int(raw[2]) << 64) | int(raw[3])
        s["has_uint32"], s["uinteger"] = int(raw[4]), int(raw[5])
        bg.state = s
    return np.random.Generator(bg)


def py_tau_walk(m, seed, raw=None):
    """The backward walk of GetGenealogy over a chain with MULTITYPE events, with numpy's generator: a direct event as
    test_lineages_rule.py_walk takes it, a MULTITYPE event row by row (pyx:873-994) with the arrivals of a row pushed after the row
    in reverse order and the count deltas applied after the row.  The rows are taken as they lie (canonical).  Returns the tree
    (parent, population, event index per node) and the lineage records (kind, hap, pop, newHap, newPop, ev) in the walk's order."""
    gen = numpy_generator(seed, raw)
    ev, mv, n = m.events, m.multievents, int(m.events.ptr)
    cols = [c[:n].tolist() for c in (ev.types, ev.haplotypes, ev.populations, ev.newHaplotypes, ev.newPopulations)]
    rows = [c[:mv.ptr].tolist() for c in (mv.num, mv.types, mv.haplotypes, mv.populations, mv.newHaplotypes, mv.newPopulations)]
    cnt, lin = {}, {}
    inf = np.asarray(m.infectious)

    def count(p, h):
        return cnt.setdefault((p, h), int(inf[p, h]))

    def lst(p, h):
        return lin.setdefault((p, h), [])
    nodes = 2 * int(m.sCounter) - 1
    parent, pop_of, ev_of = [0] * nodes, [0] * nodes, [-1] * nodes
    records = []
    ptr = 0

    def node(p, e):
        nonlocal ptr
        assert ptr < nodes, "tree overflow"
        parent[ptr], pop_of[ptr], ev_of[ptr] = -1, p, e
        ptr += 1

    def swap_pop(s, i):
        s[i] = s[-1]
        s.pop()

    def hyper(good, bad, sample):
        assert good >= 0 and bad >= 0 and sample <= good + bad, "a row numpy's hypergeometric refuses"
        return int(gen.hypergeometric(good, bad, sample))

    def row(num, t, hap, pop, nh, npop, e):
        fresh, deltas, sa = [], [], None
        if t == BIRTH:
            s = lst(pop, hap)
            lbs, lbs_e = len(s), count(pop, hap)
            kk = 0
            if not (num == 0 or lbs == 0):
                kk = hyper(int(lbs * (lbs - 1.0) / 2.0), lbs_e * (lbs_e - 1) // 2 - lbs * (lbs - 1) // 2, num)
            sa = (pop, hap)
            for _ in range(kk):
                assert lbs >= 2
                n1 = int(math.floor(lbs * gen.random()))
                n2 = int(math.floor((lbs - 1) * gen.random()))
                if n2 >= n1:
                    n2 += 1
                id1, id2, id3 = s[n1], s[n2], ptr
                fresh.append(id3)
                if n1 == lbs - 1:
                    s[n2] = s[lbs - 2]
                elif n2 == lbs - 1:
                    s[n1] = s[lbs - 2]
                else:
                    s[n1] = s[lbs - 1]
                    s[n2] = s[lbs - 2]   # (one after the other, as the reference: with n1 = lbs - 2 the second reads the first's write)
                del s[-2:]
                parent[id1] = parent[id2] = id3
                node(pop, e)
                records.append((SPLIT, hap, pop, hap, pop, e))
                lbs -= 2
            deltas = [((pop, hap), -num)]
        elif t == DEATH:
            deltas = [((pop, hap), num)]
        elif t == SAMPLING:
            sa = (pop, hap)
            deltas = [((pop, hap), num)]
            for _ in range(num):
                fresh.append(ptr)
                node(pop, e)
                records.append((TIP, hap, pop, hap, pop, e))
        elif t == MUTATION:
            s = lst(pop, nh)
            sa = (pop, hap)
            lbs = len(s)
            kk = 0 if num == 0 or lbs == 0 else hyper(lbs, count(pop, nh) - lbs, num)
            for _ in range(kk):
                n1 = int(math.floor(lbs * gen.random()))
                id1 = s[n1]
                swap_pop(s, n1)
                fresh.append(id1)
                records.append((MUT, hap, pop, nh, pop, e))
                lbs -= 1
            deltas = [((pop, nh), -num), ((pop, hap), num)]
        elif t == MIGRATION:
            ss, st = lst(pop, hap), lst(npop, hap)
            sa = (pop, hap)
            lbs = len(st)
            if not (num == 0 or lbs == 0):
                kk = hyper(lbs, count(npop, hap) - lbs, num)
                lbss = len(ss)
                k2 = 0 if kk == 0 or lbss == 0 else hyper(lbss, count(pop, hap) - lbss, kk)
                for _ in range(k2):
                    nt = int(math.floor(lbs * gen.random()))
                    ns = int(math.floor(lbss * gen.random()))
                    idt, ids, id3 = st[nt], ss[ns], ptr
                    swap_pop(ss, ns)
                    swap_pop(st, nt)
                    fresh.append(id3)
                    parent[idt] = parent[ids] = id3
                    node(pop, e)
                    records.append((SPLIT, hap, npop, hap, npop, e))
                    lbss -= 1
                    lbs -= 1
                for _ in range(kk - k2):
                    nt = int(math.floor(lbs * gen.random()))
                    fresh.append(st[nt])
                    swap_pop(st, nt)
                    records.append((MOVE, hap, pop, hap, npop, e))
                    lbs -= 1
            deltas = [((npop, hap), -num)]
        else:
            assert t == SUSCCHANGE, "row type %d" % t
        for (p, h), d in deltas:
            cnt[(p, h)] = count(p, h) + d
        for x in reversed(fresh):
            lst(*sa).append(x)

    for e in range(n - 1, -1, -1):
        t, hap, pop, nh, npop = (c[e] for c in cols)
        if t == MULTI:
            for j in range(hap, pop):
                row(*(c[j] for c in rows), e)
        elif t == BIRTH:
            s = lst(pop, hap)
            lbs, lbs_e = len(s), count(pop, hap)
            p = _div(_div(float(lbs) * (float(lbs) - 1.0), float(lbs_e)), float(lbs_e) - 1.0)
            if gen.random() < p:
                n1 = int(math.floor(lbs * gen.random()))
                n2 = int(math.floor((lbs - 1) * gen.random()))
                if n2 >= n1:
                    n2 += 1
                id1, id2, id3 = s[n1], s[n2], ptr
                s[n1] = id3
                swap_pop(s, n2)
                parent[id1] = parent[id2] = id3
                node(pop, e)
                records.append((SPLIT, hap, pop, hap, pop, e))
            cnt[(pop, hap)] = lbs_e - 1
        elif t == DEATH:
            cnt[(pop, hap)] = count(pop, hap) + 1
        elif t == SAMPLING:
            cnt[(pop, hap)] = count(pop, hap) + 1
            lst(pop, hap).append(ptr)
            node(pop, e)
            records.append((TIP, hap, pop, hap, pop, e))
        elif t == MUTATION:
            sn, sh = lst(pop, nh), lst(pop, hap)
            lbs, c_n, c_h = len(sn), count(pop, nh), count(pop, hap)
            if gen.random() < _div(float(lbs), float(c_n)):
                n1 = int(math.floor(lbs * gen.random()))
                id1 = sn[n1]
                swap_pop(sn, n1)
                sh.append(id1)
                records.append((MUT, hap, pop, nh, pop, e))
            cnt[(pop, nh)] = c_n - 1
            cnt[(pop, hap)] = c_h + 1
        elif t == MIGRATION:
            st, ss = lst(npop, hap), lst(pop, hap)
            lbs, c_t = len(st), count(npop, hap)
            if gen.random() < _div(float(lbs), float(c_t)):
                nt = int(math.floor(lbs * gen.random()))
                lbss = len(ss)
                if gen.random() < _div(float(lbss), float(count(pop, hap))):
                    ns = int(math.floor(lbss * gen.random()))
                    idt, ids, id3 = st[nt], ss[ns], ptr
                    ss[ns] = id3
                    swap_pop(st, nt)
                    parent[idt] = parent[ids] = id3
                    node(pop, e)
                    records.append((SPLIT, hap, npop, hap, npop, e))
                else:
                    ss.append(st[nt])
                    swap_pop(st, nt)
                    records.append((MOVE, hap, pop, hap, npop, e))
            cnt[(npop, hap)] = c_t - 1
        else:
            assert t == SUSCCHANGE, "event type %d" % t
    assert ptr == nodes and all(0 <= p < nodes for p in parent[:-1]) and parent[-1] == -1, "the walk did not coalesce"
    return {"tree": np.array(parent), "tree_pop": np.array(pop_of), "node_ev": np.array(ev_of), "records": records}


def node_times(m):
    """What the walk writes for a node of event e: the time of a MULTITYPE event's first row, else the event's time."""
    ev, mv, n = m.events, m.multievents, int(m.events.ptr)
    t = ev.times[:n].copy()
    for e in range(n):
        if ev.types[e] == MULTI and ev.populations[e] > ev.haplotypes[e]:
            t[e] = mv.times[int(ev.haplotypes[e])]
    return t


def check_chain(m, seed, raw, what, scramble_seed=5):
    """Everything the rule promises on one chain and generator start (a seed, or None and six raw words): both pins on a healthy chain, the host pass's message on one whose walk
    fails.  Returns whether the chain is healthy."""
    from vgsim_amd import _capi
    n = int(m.events.ptr)
    times = m.events.times[:n].copy()
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)
    try:
        g = _capi.tau_genealogy_walk(copy.deepcopy(m), seed, rng_raw=raw)
    except RuntimeError as e:
        for twin in (copy.deepcopy(m), decanonicalised(m, scramble_seed)):
            with pytest.raises(ValueError) as got:
                _capi.replay_tau_lineages(twin, seed, [float(times[n // 2])], ident, H, rng_raw=raw)
            assert str(got.value) == str(e), what
        return False
    w = py_tau_walk(m, seed, raw)
    # pin 1: the restatement's tree is the tau walk's
    assert np.array_equal(w["tree"], g["tree"]) and np.array_equal(w["tree_pop"], g["tree_pop"]), what + " tree"
    assert np.array_equal(np.where(w["node_ev"] >= 0, node_times(m)[np.maximum(w["node_ev"], 0)], 0.0), g["times"]), what + " node events"
    ev_desc = [r[5] for r in w["records"]]
    assert ev_desc == sorted(ev_desc, reverse=True), what + ": records in descending event order"
    raw_rows = decanonicalised(m, scramble_seed)
    for grid in grids(times):
        for vo, V in maps(H):
            want_v, want_r = py_lineages(w["records"], times, grid, vo, P, V)
            for tile in (0, 1, 7, 64):
                twin = copy.deepcopy(m)
                out = _capi.replay_tau_lineages(twin, seed, grid, vo, V, tile=tile, rng_raw=raw)
                # pin 2: the library's walk, observer, tile walk and scan give the restatement's block
                assert out["values"].dtype == np.int32 and np.array_equal(out["values"], want_v), "%s values T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert np.array_equal(out["root"], want_r), "%s root T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert out["records"] == len(w["records"]) and out["rng_raw"] == g["rng_raw"] and out["nodes_used"] == g["nodes_used"], what
            # the order and granularity of the trailing steps' rows change nothing
            out = _capi.replay_tau_lineages(copy.deepcopy(raw_rows), seed, grid, vo, V, tile=7, rng_raw=raw)
            assert np.array_equal(out["values"], want_v) and np.array_equal(out["root"], want_r), what + " split and shuffled rows"
            assert out["records"] == len(w["records"]) and out["rng_raw"] == g["rng_raw"], what + " split and shuffled rows"
            if V == H:   # every haplotype tracked
                assert int(want_r.sum()) == 1, what + " root"
                # (the nodes of one step share a time: such zero-length branches are alive nowhere, in the tree and in the block)
                assert np.array_equal(want_v.sum(axis=(-1, -2)), alive(g, grid)), what + " lineages through time"
    return True


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_lineages_on_reference_tau_chains(oracle_mod, path):
    meta, _ = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"], record_multievents=True).simulation
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    assert trailing_steps(m) < m.events.ptr
    raw = tuple(st.rng_final) + (0, 0) if meta["genealogy_seed"] is None else None
    assert check_chain(m, meta["genealogy_seed"], raw, meta["case"])


def test_continued_chains(oracle_mod):
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    assert 0 < trailing_steps(m) < m.events.ptr
    assert check_chain(m, 31, None, "tau_d")
    m = helpers.run_case_oracle(oracle_mod, "tau_then_direct", record_multievents=True).simulation
    assert oracle_mod.run_tau(m, 25, 10 ** 12, -1, 200, record_multievents=True) == 0
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    first = trailing_steps(m)
    t = m.events.types[:first]
    assert first < m.events.ptr and (t == MULTI).any() and t[0] != MULTI and t[-1] != MULTI   # rows of an earlier tau call in the prefix
    for seed, raw in ((32, None), (None, tuple(st.rng_final) + (0, 0)), (None, tuple(st.rng_final) + (1, 0x9E3779B9))):
        assert check_chain(m, seed, raw, "tau_then_direct + tau")


@functools.lru_cache(maxsize=None)
def _fuzz(seed):
    from oracle import oracle
    sim, n = fuzz_build(seed)
    m = sim.simulation
    assert oracle.run_direct(m, n, 10 ** 9, -1, 200) == 0
    assert oracle.run_tau(m, 20, 10 ** 12, -1, 200, record_multievents=True) == 0
    st = oracle.get_state(m)
    helpers.sparse_multievents(m, st)
    assert trailing_steps(m) < m.events.ptr
    return m, tuple(st.rng_final) + (0, 0)


@pytest.mark.parametrize("seed", FUZZ)
def test_lineages_on_random_models(oracle_mod, seed):
    m, final = _fuzz(seed)
    for gseed, raw in ((None, final), (1000 + seed, None)):
        check_chain(m, gseed, raw, "fuzz %d seed %r" % (seed, gseed), scramble_seed=seed)


def test_most_random_models_walk_cleanly(oracle_mod):
    """The replay itself goes through on most of the random models (a guard on the fixtures: test_lineages_on_random_models
    checks the message of the others)."""
    from vgsim_amd import _capi
    healthy = 0
    for seed in FUZZ:
        m = _fuzz(seed)[0]
        t = m.events.times[:m.events.ptr]
        try:
            out = _capi.replay_tau_lineages(copy.deepcopy(m), 1000 + seed, [float(t[len(t) // 2])], np.arange(m.hapNum, dtype=np.int32), m.hapNum)
            healthy += int(out["root"].sum()) == 1
        except ValueError:
            pass
    assert healthy >= 12, healthy


def test_a_grid_point_at_a_step_time_has_the_step_applied(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    n, first = int(m.events.ptr), trailing_steps(m)
    t = m.events.times[:n]
    H = int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)
    w = py_tau_walk(m, 31)
    steps_with_records = sorted({r[5] for r in w["records"] if first <= r[5] < n - 1 and t[r[5] - 1] < t[r[5]] < t[r[5] + 1]})
    assert steps_with_records
    k = steps_with_records[len(steps_with_records) // 2]
    at = _capi.replay_tau_lineages(copy.deepcopy(m), 31, [float(t[k])], ident, H)
    after = _capi.replay_tau_lineages(copy.deepcopy(m), 31, [0.5 * (float(t[k]) + float(t[k + 1]))], ident, H)
    before = _capi.replay_tau_lineages(copy.deepcopy(m), 31, [0.5 * (float(t[k - 1]) + float(t[k]))], ident, H)
    assert np.array_equal(at["values"], after["values"]) and not np.array_equal(at["values"], before["values"])
    want_v, _ = py_lineages(w["records"], t, [float(t[k])], ident, int(m.popNum), H)
    assert np.array_equal(at["values"], want_v)


def test_a_row_numpy_would_refuse_is_the_status_12_text():
    from vgsim_amd import _capi
    m = _more_migrants_than_sources()
    with pytest.raises(ValueError) as got:
        _capi.replay_tau_lineages(m, 3, [0.15], np.zeros(1, dtype=np.int32), 1)
    assert str(got.value) == _capi.genealogy_message(12, 0) and str(got.value).startswith("vgx_get_tau_genealogies:")


def test_refusals(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)

    def call(grid, vo, V):
        return _capi.replay_tau_lineages(copy.deepcopy(m), 1000, grid, vo, V)
    with pytest.raises(ValueError, match=r"vgx_test_tau_lineages: grid must increase strictly \(grid\[1\]\)"):
        call([0.5, 0.5], ident, H)
    with pytest.raises(ValueError, match=r"vgx_test_tau_lineages: grid\[0\] is not finite"):
        call([np.nan], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tau_lineages: T = 0 must be at least 1"):
        call([], ident, H)
    with pytest.raises(ValueError, match="vgx_test_tau_lineages: V = 0 must be at least 1"):
        call([0.5], np.full(H, -1, dtype=np.int32), 0)
    bad = ident.copy()
    bad[1] = H
    with pytest.raises(ValueError, match=r"vgx_test_tau_lineages: variant_of\[1\] = %d is outside \[-1, %d\)" % (H, H)):
        call([0.5], bad, H)
    with pytest.raises(ValueError, match="variant_of must hold hapNum values"):
        call([0.5], ident[:-1], H)
    V = 16384 // P + 1   # P V 4 bytes of cells just above 64 KiB
    with pytest.raises(ValueError, match="bytes of cells, above the 65536 bytes of LDS"):
        call([0.5], np.zeros(H, dtype=np.int32), V)
    m.sCounter = 1
    with pytest.raises(ValueError, match="Less than two cases were sampled"):
        call([0.5], ident, H)
