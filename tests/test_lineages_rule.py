"""Lineages on a grid (vgsim_amd/csrc/vgx_lineages.h) against a pure-Python restatement of the backward walk that
counts lineages as it goes.  The restatement draws from numpy's PCG64 and is pinned twice: its tree is the one
``_capi.get_genealogy`` returns for the same model and seed, and ``_capi.replay_lineages`` (the device's walk, observer, tile walk
and suffix sum compiled for the host) gives its values and root exactly.  Chains: the reference's direct genealogy fixtures and
the 48 random models of test_hip_fuzz.  No GPU."""
import copy
import functools
import glob
import math
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import load
from test_hip_fuzz import build as fuzz_build

GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "genealogy_*.npz"))
              if not os.path.basename(p).startswith("genealogy_tau_"))
BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
TIP, SPLIT, MUT, MOVE = range(4)


def _div(a, b):
    """a / b as IEEE doubles divide (the walk divides by counts that a broken chain can take to zero)."""
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def py_walk(m, seed):
    """The backward walk of GetGenealogy over a direct chain, event by event, with numpy's generator.  Returns the tree (parent,
    population, event index per node) and the lineage records (kind, hap, pop, newHap, newPop, ev) in the order of the walk."""
    gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(0,))))
    ev, n, H = m.events, int(m.events.ptr), int(m.hapNum)
    cols = [c[:n].tolist() for c in (ev.types, ev.haplotypes, ev.populations, ev.newHaplotypes, ev.newPopulations)]
    cnt = {}
    inf = np.asarray(m.infectious)

    def count(p, h):
        return cnt.setdefault((p, h), int(inf[p, h]))
    lin = {}
    nodes = 2 * int(m.sCounter) - 1
    parent, pop_of, ev_of = [0] * nodes, [0] * nodes, [-1] * nodes
    records = []
    ptr = 0

    def node(p, e):
        nonlocal ptr
        assert ptr < nodes, "tree overflow"
        parent[ptr], pop_of[ptr], ev_of[ptr] = -1, p, e
        ptr += 1

    def swap_pop(lst, i):
        lst[i] = lst[-1]
        lst.pop()
    for e in range(n - 1, -1, -1):
        t, hap, pop, nh, npop = (c[e] for c in cols)
        if t == BIRTH:
            s = lin.setdefault((pop, hap), [])
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
            lin.setdefault((pop, hap), []).append(ptr)
            node(pop, e)
            records.append((TIP, hap, pop, hap, pop, e))
        elif t == MUTATION:
            sn, sh = lin.setdefault((pop, nh), []), lin.setdefault((pop, hap), [])
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
            st, ss = lin.setdefault((npop, hap), []), lin.setdefault((pop, hap), [])
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
    assert H >= 1
    return {"tree": np.array(parent), "tree_pop": np.array(pop_of), "node_ev": np.array(ev_of), "records": records}


def cuts(times, grid):
    """cut[j] = first event index i with grid[j] < t_i (strict; the position never goes back), n if none."""
    T, n = len(grid), len(times)
    cut, point = [n] * T, 0
    for i, t in enumerate(times):
        while point < T and grid[point] < t:
            cut[point] = i
            point += 1
    return cut


def py_lineages(records, times, grid, variant_of, P, V):
    """values [T, P, V] and root [P, V] from the lineage records by the rule: the net change of every interval read forward in
    time, values[j] = -(net of the intervals j + 1 .. T), root = -(net of all)."""
    T = len(grid)
    cut = cuts(times, grid)
    net = np.zeros((T + 1, P, V), dtype=np.int64)
    for kind, hap, pop, nh, npop, e in records:
        k = sum(1 for c in cut if c <= e)   # cut[k - 1] <= e < cut[k]
        c, c2 = int(variant_of[hap]), int(variant_of[nh])
        if kind == TIP and c >= 0:
            net[k, pop, c] -= 1
        elif kind == SPLIT and c >= 0:
            net[k, pop, c] += 1
        elif kind == MUT and c != c2:
            if c >= 0:
                net[k, pop, c] -= 1
            if c2 >= 0:
                net[k, pop, c2] += 1
        elif kind == MOVE and c >= 0:
            net[k, pop, c] -= 1
            net[k, npop, c] += 1
    values = np.stack([-net[j + 1:].sum(axis=0) for j in range(T)])
    return values.astype(np.int32), (-net.sum(axis=0)).astype(np.int32)


def grids(times):
    """The grids every chain is checked on: one with a point below the first event time, two points inside one gap between events,
    a point exactly at an event time and one above the last event time; and a single point (T = 1) at an event time."""
    t = np.asarray(times, dtype=np.float64)
    n = len(t)
    gap = next(i for i in range(n // 3, n - 1) if t[i] < t[i + 1])
    d = t[gap + 1] - t[gap]
    full = sorted({t[0] - 1.0, t[gap] + d / 3.0, t[gap] + 2.0 * d / 3.0, float(t[(2 * n) // 3]), t[-1] + 1.0})
    return [np.array(full), np.array([float(t[n // 2])])]


def maps(H):
    """(variant_of, V): every haplotype its own class, and three classes with one haplotype untracked."""
    three = (np.arange(H) % 3).astype(np.int32)
    three[H // 2] = -1
    return [(np.arange(H, dtype=np.int32), H), (three, 3)]


def alive(g, grid):
    """Nodes of a genealogy with t_parent <= grid[j] < t_node for every j (the root's parent time is -inf)."""
    t_node = np.asarray(g["times"], dtype=np.float64)
    par = np.asarray(g["tree"])
    t_par = np.where(par >= 0, t_node[np.maximum(par, 0)], -np.inf)
    grid = np.asarray(grid)[:, None]
    return ((t_par[None, :] <= grid) & (grid < t_node[None, :])).sum(axis=1)


def check_chain(m, seed, what):
    """Everything the rule promises on one healthy chain."""
    from vgsim_amd import _capi
    n = int(m.events.ptr)
    times = m.events.times[:n].copy()
    P, H = int(m.popNum), int(m.hapNum)
    g = _capi.get_genealogy(copy.deepcopy(m), seed)
    w = py_walk(m, seed)
    # pin 1: the restatement's tree is the host pass's
    assert np.array_equal(w["tree"], g["tree"]) and np.array_equal(w["tree_pop"], g["tree_pop"]), what + " tree"
    assert np.array_equal(np.where(w["node_ev"] >= 0, times[np.maximum(w["node_ev"], 0)], 0.0), g["times"]), what + " node events"
    for grid in grids(times):
        for vo, V in maps(H):
            want_v, want_r = py_lineages(w["records"], times, grid, vo, P, V)
            first = None
            for tile in (0, 1, 7, 64):
                twin = copy.deepcopy(m)
                out = _capi.replay_lineages(twin, seed, grid, vo, V, tile=tile)
                # pin 2: the library's walk, observer, tile walk and scan give the restatement's block
                assert out["values"].dtype == np.int32 and np.array_equal(out["values"], want_v), "%s values T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert np.array_equal(out["root"], want_r), "%s root T=%d V=%d tile=%d" % (what, len(grid), V, tile)
                assert out["records"] == len(w["records"]) and out["rng_raw"][:4] == g["rng_raw"][:4], what
                first = first or out
                assert np.array_equal(out["values"], first["values"]) and np.array_equal(out["root"], first["root"])
            if V == H:   # every haplotype tracked
                assert int(want_r.sum()) == 1, what + " root"
                assert np.array_equal(want_v.sum(axis=(-1, -2)), alive(g, grid)), what + " lineages through time"


@pytest.mark.parametrize("k,path", list(enumerate(GOLD)), ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_lineages_on_reference_chains(oracle_mod, k, path):
    meta, _ = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"]).simulation
    check_chain(m, 1000 + k, meta["case"])


@functools.lru_cache(maxsize=None)
def _fuzz(seed):
    """(model after the oracle's run or None, the host pass's message or None) of random model `seed`."""
    from oracle import oracle
    from vgsim_amd import _capi
    sim, n = fuzz_build(seed)
    if oracle.run_direct(sim.simulation, n, 10 ** 9, -1, 200) != 0:
        return None, "no chain"
    m = sim.simulation
    try:
        _capi.get_genealogy(copy.deepcopy(m), 1000 + seed)
    except RuntimeError as e:
        return m, str(e)
    return m, None


@pytest.mark.parametrize("seed", range(48))
def test_lineages_on_random_models(oracle_mod, seed):
    from vgsim_amd import _capi
    m, message = _fuzz(seed)
    if m is None:
        return   # the reference aborts on a zero weight: no chain (counted as not healthy below)
    if message is not None:   # the walk fails: the host pass's message
        t = m.events.times[:m.events.ptr]
        grid = np.array([float(t[len(t) // 2]) if len(t) else 0.5])
        with pytest.raises(ValueError) as got:
            _capi.replay_lineages(copy.deepcopy(m), 1000 + seed, grid, np.arange(m.hapNum, dtype=np.int32), m.hapNum)
        assert str(got.value) == message
        return
    check_chain(m, 1000 + seed, "fuzz %d" % seed)


def test_most_random_models_walk_cleanly(oracle_mod):
    healthy = sum(1 for seed in range(48) if _fuzz(seed)[0] is not None and _fuzz(seed)[1] is None)
    assert healthy >= 40, healthy


def test_refusals(oracle_mod):
    from vgsim_amd import _capi
    m = helpers.run_case_oracle(oracle_mod, "g9_short").simulation
    P, H = int(m.popNum), int(m.hapNum)
    ident = np.arange(H, dtype=np.int32)

    def call(grid, vo, V):
        return _capi.replay_lineages(copy.deepcopy(m), 1000, grid, vo, V)
    with pytest.raises(ValueError, match=r"vgx_test_lineages: grid must increase strictly \(grid\[1\]\)"):
        call([0.5, 0.5], ident, H)
    with pytest.raises(ValueError, match=r"vgx_test_lineages: grid\[0\] is not finite"):
        call([np.nan], ident, H)
    with pytest.raises(ValueError, match="vgx_test_lineages: T = 0 must be at least 1"):
        call([], ident, H)
    with pytest.raises(ValueError, match="vgx_test_lineages: V = 0 must be at least 1"):
        call([0.5], np.full(H, -1, dtype=np.int32), 0)
    bad = ident.copy()
    bad[1] = H
    with pytest.raises(ValueError, match=r"vgx_test_lineages: variant_of\[1\] = %d is outside \[-1, %d\)" % (H, H)):
        call([0.5], bad, H)
    bad[1] = -2
    with pytest.raises(ValueError, match=r"vgx_test_lineages: variant_of\[1\] = -2 is outside"):
        call([0.5], bad, H)
    with pytest.raises(ValueError, match="variant_of must hold hapNum values"):
        call([0.5], ident[:-1], H)
    V = 16384 // P + 1   # P V 4 bytes of cells just above 64 KiB
    with pytest.raises(ValueError, match="bytes of cells, above the 65536 bytes of LDS"):
        call([0.5], np.zeros(H, dtype=np.int32), V)
    m.sCounter = 1
    with pytest.raises(ValueError, match="Less than two cases were sampled"):
        call([0.5], ident, H)
