"""The rule of vgx_introductions.h on the host (``_capi.introductions``, the sequential sweep behind ``Ensemble.introductions``)
against a plain-Python restatement written here that walks from every tip towards the root, closed forms for small, caterpillar,
nested and balanced trees, the identities that tie the blocks together on random labelled trees, the closing-pass migration records
of the host walk over the reference's golden chains, the trees and labels it refuses, and the derived values of ``Introductions``
against a scalar restatement.  No GPU.

Every output is a count, a sum or a maximum of integers: everything here is asserted with equality; the derived values (float64
from the integer blocks by a fixed sequence of operations) are asserted bit for bit."""
import functools
import glob
import math
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import load
from test_tree_shape_rule import balanced, caterpillar, random_tree
from vgsim_amd import _capi
from vgsim_amd.ensemble import Introductions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIRECT_GOLD = sorted(p for p in glob.glob(os.path.join(GOLDEN, "genealogy_*.npz")) if not os.path.basename(p).startswith("genealogy_tau_"))
INTO, STATS = _capi.INTRODUCTIONS_INTO, _capi.INTRODUCTIONS_STATS
NAMES = ("tips_by_pop", "imports", "into", "spectrum", "stats", "clade", "local")
THREE = np.array([2, 2, -1])


def random_labels(tree, P, rng, move=0.2):
    """Labels from the root down: a child keeps its parent's population, or with probability ``move`` draws one anew."""
    N = len(tree)
    pop = np.zeros(N, dtype=np.int64)
    pop[N - 1] = rng.integers(P)
    for i in range(N - 2, -1, -1):   # (parents have higher ids)
        pop[i] = rng.integers(P) if rng.random() < move else pop[tree[i]]
    return pop


@functools.lru_cache(maxsize=None)
def random_cases(count=200, seed=61):
    """(tree, pop, P) of ``count`` random labelled trees: 2 .. 120 tips, 1 .. 9 populations, rare to constant moves."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        t = random_tree(int(rng.integers(2, 121)), rng)
        P = int(rng.integers(1, 10))
        out.append((t, random_labels(t, P, rng, move=(0.0, 0.05, 0.2, 0.6, 1.0)[k % 5]), P))
    return tuple(out)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def restate(tree, pop, P):
    """The five blocks, clade and local in Python integers: every tip walks to the root and counts itself in the clade of every
    node on the way, and in ``local`` of every node up to and including the first one below a crossing branch."""
    N = len(tree)
    has_kid = [False] * N
    for i in range(N - 1):
        has_kid[int(tree[i])] = True
    clade, local = [0] * N, [0] * N
    tips_by_pop = [0] * P
    for t in range(N):
        if has_kid[t]:
            continue
        tips_by_pop[int(pop[t])] += 1
        v, inside = t, True
        while v >= 0:
            clade[v] += 1
            local[v] += inside
            up = int(tree[v])
            if up >= 0 and pop[up] != pop[v]:
                inside = False
            v = up
    imports = [[0] * P for _ in range(P)]
    into = [[0] * 6 for _ in range(P)]
    spectrum = [[0] * 32 for _ in range(P)]
    intro = empty = max_clade = 0
    max_local = local[N - 1]
    for i in range(N - 1):
        src, dst = int(pop[tree[i]]), int(pop[i])
        if src == dst:
            continue
        c, l = clade[i], local[i]
        imports[src][dst] += 1
        q = into[dst]
        q[0], q[1], q[2], q[3], q[4], q[5] = q[0] + 1, q[1] + c, q[2] + l, q[3] + l * l, q[4] + (l == 0), max(q[5], l)
        if l:
            spectrum[dst][l.bit_length() - 1] += 1
        intro, empty, max_clade, max_local = intro + 1, empty + (l == 0), max(max_clade, c), max(max_local, l)
    stats = [clade[N - 1], intro, int(pop[N - 1]), local[N - 1], max_local, max_clade, empty, sum(1 for x in tips_by_pop if x)]
    i64 = lambda x: np.array(x, dtype=np.int64)
    return (i64(tips_by_pop), i64(imports), i64(into), i64(spectrum), i64(stats), np.array(clade, dtype=np.int32), np.array(local, dtype=np.int32))


def assert_blocks_equal(got, want, what):
    for g, w, k in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k, g, w)


def assert_identities(blocks, what=None):
    """What ties the five blocks of one row together."""
    tips_by_pop, imports, into, spectrum, stats = blocks[:5]
    st = dict(zip(STATS, stats.tolist()))
    root = np.arange(len(tips_by_pop)) == st["root_pop"]
    assert tips_by_pop.sum() == st["tips"], what
    assert np.array_equal(tips_by_pop, into[:, 2] + root * st["root_local"]), what
    assert np.array_equal(imports.sum(axis=0), into[:, 0]), what
    assert np.array_equal(spectrum.sum(axis=1) + into[:, 4], into[:, 0]), what
    assert st["introductions"] == imports.sum() and not np.diagonal(imports).any(), what
    assert st["empty"] == into[:, 4].sum() and st["pops_with_tips"] == (tips_by_pop > 0).sum(), what
    assert st["max_local"] == max(st["root_local"], into[:, 5].max()) and not spectrum[:, 31].any(), what


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_three_nodes_with_zero_one_and_two_crossings():
    tips, imports, into, spectrum, stats = _capi.introductions(THREE, [0, 0, 0], 2)
    assert tips.tolist() == [2, 0] and not imports.any() and not into.any() and not spectrum.any()
    assert stats.tolist() == [2, 0, 0, 2, 2, 0, 0, 1]
    tips, imports, into, spectrum, stats, clade, local = _capi.introductions(THREE, [1, 0, 0], 2, with_nodes=True)
    assert tips.tolist() == [1, 1] and imports.tolist() == [[0, 1], [0, 0]] and into.tolist() == [[0] * 6, [1, 1, 1, 1, 0, 1]]
    assert spectrum[1, 0] == 1 and spectrum.sum() == 1 and stats.tolist() == [2, 1, 0, 1, 1, 1, 0, 2]
    assert clade.tolist() == [1, 1, 2] and local.tolist() == [1, 1, 1] and clade.dtype == local.dtype == np.int32
    tips, imports, into, spectrum, stats, clade, local = _capi.introductions(THREE, [1, 1, 0], 2, with_nodes=True)
    assert tips.tolist() == [0, 2] and imports.tolist() == [[0, 2], [0, 0]] and into.tolist() == [[0] * 6, [2, 2, 2, 2, 0, 1]]
    assert spectrum[1, 0] == 2 and stats.tolist() == [2, 2, 0, 0, 1, 1, 0, 1] and local.tolist() == [1, 1, 0]
    tips, imports, into, spectrum, stats = _capi.introductions(THREE, [2, 0, 1], 3)   # two sources are told apart by direction
    assert imports.tolist() == [[0, 0, 0], [1, 0, 1], [0, 0, 0]] and stats.tolist() == [2, 2, 1, 0, 1, 1, 0, 2]
    assert all(a.dtype == np.int64 for a in (tips, imports, into, spectrum, stats))
    assert into.shape == (3, 6) and spectrum.shape == (3, 32) and stats.shape == (8,)


def test_one_population_is_one_lineage():
    rng = np.random.default_rng(3)
    for s in (2, 3, 40, 129):
        t = random_tree(s, rng)
        tips, imports, into, spectrum, stats, clade, local = _capi.introductions(t, np.zeros(len(t), int), 1, with_nodes=True)
        assert tips.tolist() == [s] and not imports.any() and not into.any() and not spectrum.any()
        assert stats.tolist() == [s, 0, 0, s, s, 0, 0, 1] and np.array_equal(clade, local)


def test_caterpillar_with_alternating_labels():
    """70 tips, label = node id mod 2: every branch crosses but the one above tip 0, so every lineage has size 0 or 1."""
    t = caterpillar(70)
    N = len(t)
    pop = np.arange(N) % 2
    tips, imports, into, spectrum, stats, clade, local = _capi.introductions(t, pop, 2, with_nodes=True)
    assert_blocks_equal((tips, imports, into, spectrum, stats, clade, local), restate(t, pop, 2), "caterpillar")
    assert local.max() == 1 and local[70] == 1 and not local[71:].any() and local[:70].tolist() == [1] * 70
    assert stats.tolist() == [70, 137, 0, 0, 1, 69, 67, 2]   # root 138 is even; nodes 71 .. 137 head empty lineages
    assert spectrum[:, 0].sum() == 70 and not spectrum[:, 1:].any() and into[:, 4].sum() == 67 and into[:, 5].tolist() == [1, 1]
    assert tips.tolist() == [35, 35] and imports[0, 1] + imports[1, 0] == 137
    assert_identities((tips, imports, into, spectrum, stats))


def test_nested_introductions_reset_local_but_not_clade():
    """((0, 1) 4, 2) 5, 3) 6 with a crossing 0 -> 1 above node 5 and a crossing 1 -> 2 above node 4 inside it."""
    t = np.array([4, 4, 5, 6, 5, 6, -1])
    pop = np.array([2, 2, 1, 0, 2, 1, 0])
    tips, imports, into, spectrum, stats, clade, local = _capi.introductions(t, pop, 3, with_nodes=True)
    assert clade.tolist() == [1, 1, 1, 1, 2, 3, 4] and local.tolist() == [1, 1, 1, 1, 2, 1, 1]
    assert imports.tolist() == [[0, 1, 0], [0, 0, 1], [0, 0, 0]]
    assert into.tolist() == [[0] * 6, [1, 3, 1, 1, 0, 1], [1, 2, 2, 4, 0, 2]]
    assert spectrum[1, 0] == 1 and spectrum[2, 1] == 1 and spectrum.sum() == 2
    assert tips.tolist() == [1, 1, 2] and stats.tolist() == [4, 2, 0, 1, 2, 3, 0, 3]


@pytest.mark.parametrize("k,d", [(1, 1), (3, 1), (6, 2), (6, 6), (5, 0)])
def test_balanced_tree_split_at_depth(k, d):
    """2^k tips; every node at depth >= d carries the label 1 + (index of its ancestor at depth d), everything above label 0: 2^d
    introductions out of 0, each of 2^(k - d) tips, and an empty root lineage (for d = 0 nothing crosses)."""
    t = balanced(k)
    N = len(t)
    depth, label = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    nxt = 1
    for i in range(N - 2, -1, -1):
        depth[i] = depth[t[i]] + 1
        if depth[i] == d:
            label[i], nxt = nxt, nxt + 1
        elif depth[i] > d:
            label[i] = label[t[i]]
    if d == 0:
        label[:] = 0
    P = 2 ** d + 1
    tips, imports, into, spectrum, stats = _capi.introductions(t, label, P)
    size = 2 ** (k - d)
    if d == 0:
        assert stats.tolist() == [2 ** k, 0, 0, 2 ** k, 2 ** k, 0, 0, 1] and not imports.any()
        return
    assert stats.tolist() == [2 ** k, 2 ** d, 0, 0, size, size, 0, 2 ** d]
    assert imports[0, 1:].tolist() == [1] * 2 ** d and imports.sum() == 2 ** d
    assert into[1:].tolist() == [[1, size, size, size * size, 0, size]] * 2 ** d and not into[0].any()
    assert spectrum[1:, k - d].tolist() == [1] * 2 ** d and spectrum.sum() == 2 ** d
    assert tips.tolist() == [0] + [size] * 2 ** d


def test_random_labelled_trees_equal_the_restatement_and_keep_the_identities():
    crossings = 0
    for k, (t, pop, P) in enumerate(random_cases()):
        got = _capi.introductions(t, pop, P, with_nodes=True)
        assert_blocks_equal(got, restate(t, pop, P), k)
        assert_identities(got, k)
        assert len(_capi.introductions(t, pop, P)) == 5
        crossings += int(got[4][1])
    assert len(random_cases()) == 200 and crossings > 1000


# ---- the closing pass of the walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", DIRECT_GOLD, ids=[os.path.basename(p)[10:-4] for p in DIRECT_GOLD])
def test_crossing_branches_are_the_closing_records_of_the_host_walk(oracle_mod, path):
    """The walk's migration records end with one record per branch whose two ends differ in population, in node order (its closing
    pass): those are the crossing branches of the rule, as (node, old, new) = (i, src, dst)."""
    meta, z = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"]).simulation
    st = oracle_mod.get_state(m)
    raw = tuple(st.rng_final) + (0, 0) if meta["genealogy_seed"] is None else None
    g = _capi.genealogy_walk(m, meta["genealogy_seed"], rng_raw=raw)
    tree, pop = np.asarray(g["tree"], dtype=np.int64), np.asarray(g["tree_pop"], dtype=np.int64)
    assert np.array_equal(tree, z["tree"])
    P = int(m.popNum)
    blocks = _capi.introductions(tree, pop, P)
    assert_identities(blocks, meta["case"])
    nodes = [i for i in range(len(tree) - 1) if pop[tree[i]] != pop[i]]
    K = len(nodes)
    assert K == blocks[4][1] <= len(g["mig_node"])
    tail = slice(len(g["mig_node"]) - K, None)
    assert np.asarray(g["mig_node"])[tail].tolist() == nodes
    assert np.asarray(g["mig_old"])[tail].tolist() == [int(pop[tree[i]]) for i in nodes]
    assert np.asarray(g["mig_new"])[tail].tolist() == [int(pop[i]) for i in nodes]
    want = np.zeros((P, P), dtype=np.int64)
    np.add.at(want, (pop[tree[nodes]], pop[nodes]), 1)
    assert np.array_equal(blocks[1], want)
    if meta["case"] in ("c3_s5_p16", "p70", "stress_h64"):
        assert K > 0, meta["case"]
    print("%s: %d crossing branches of %d migration records" % (meta["case"], K, len(g["mig_node"])))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_labels_are_refused_with_the_node():
    rng = np.random.default_rng(7)
    t = random_tree(20, rng)
    N, P = len(t), 3
    pop = random_labels(t, P, rng)
    for v in (-1, P, 2 ** 31 - 1, -2 ** 31):
        for i in (0, 17, N - 1):
            bad = pop.copy()
            bad[i] = v
            with pytest.raises(ValueError, match=r"label of node %d is %d\b" % (i, v)):
                _capi.introductions(t, bad, P)
    bad = pop.copy()
    bad[30], bad[12], bad[25] = P, -4, 99
    with pytest.raises(ValueError, match=r"label of node 12 "):   # (the lowest of several)
        _capi.introductions(t, bad, P)
    for pops in (0, -1, _capi.INTRODUCTIONS_POPS_MAX + 1):
        with pytest.raises(ValueError, match="populations"):
            _capi.introductions(t, pop, pops)
    with pytest.raises(ValueError, match="one entry per node"):
        _capi.introductions(t, pop[:-1], P)
    assert _capi.introductions(t, pop, P)[4][0] == 20
    assert _capi.introductions(t, np.full(N, 255), 256)[0][255] == 20 and _capi.introductions(t, pop, 1024)[1].shape == (1024, 1024)
    assert _capi.genealogy_message(_capi.GW_BAD_LABEL, 12).startswith("vgx_get_introductions: the label of node 12 ")
    assert (_capi.GW_BAD_TREE, _capi.GW_BAD_RECORD, _capi.GW_BAD_LABEL) == (13, 14, 15)
    assert _capi.genealogy_message(14, 3).startswith("vgx_get_mutation_spectrum: mutation record 3 ")   # (no existing text changed)


def test_malformed_trees_are_refused_with_the_node_before_the_labels():
    for name in ("forest_recomb_a_seed21.npz", "forest_recomb_pos_seed22.npz"):
        z = np.load(os.path.join(GOLDEN, name))
        with pytest.raises(ValueError, match=r"node \d+"):
            _capi.introductions(z["tree"], np.zeros(len(z["tree"]), int), 1)

    def refused(tree, node, pop=None):
        with pytest.raises(ValueError, match=r"node %d\b" % node):
            _capi.introductions(tree, np.zeros(len(tree), int) if pop is None else pop, 2)
    refused([3, 1, 3, 4, -1], 1)          # tree[i] <= i
    refused([3, 5, 3, 4, -1], 1)          # a parent outside the tree
    refused([2, 3, 3, 4, 4], 4)           # the last node is not a root
    refused([2, 3, 3, 4, -1], 2)          # node 2 has one child
    refused([3, 3, 3, 4, -1], 3)          # node 3 has three children
    refused([2, 2, 3, -1], 4)             # an even number of nodes
    refused([-1], 1)                      # one node
    with pytest.raises(ValueError, match=r"node 2 has 1 children"):   # the tree is judged first: node 0's label is bad as well
        _capi.introductions([2, 3, 3, 4, -1], [7, 0, 0, 0, 0], 2)


# ---- the derived values ----------------------------------------------------------------------------------------------------------
def introductions_of(cases, status=None):
    """An Introductions over given (tree, pop, P) cases of ONE P, built from the host hook's blocks."""
    blocks = [_capi.introductions(*c) for c in cases]
    it = Introductions()
    it.pops = cases[0][2]
    it.replicates = np.arange(len(cases), dtype=np.int64)
    it.tips_by_pop, it.imports, it.into, it.spectrum, it.stats = (np.stack([b[k] for b in blocks]) for k in range(5))
    it.status = np.zeros(len(cases), dtype=np.int64) if status is None else np.asarray(status, dtype=np.int64)
    it.status_arg = np.zeros(len(cases), dtype=np.int64)
    for i in np.nonzero(it.status)[0]:   # (a failed walk's row: zeros)
        it.tips_by_pop[i], it.imports[i], it.into[i], it.spectrum[i], it.stats[i] = 0, 0, 0, 0, 0
    return it


class _Flows:   # what observed_share() reads of a Flows
    def __init__(self, replicates, imports):
        self.replicates, self._imports = replicates, imports

    def imports(self):
        return self._imports


def scalar_derived(it, i, p, true_imports):
    """The ratios of row i and population p in Python floats, in the operation order of Introductions."""
    nan = float("nan")
    keys = ("mean_lineage_size", "size_weighted_mean", "singleton_share", "empty_share", "observed_share")
    if it.status[i] != 0:
        return dict.fromkeys(keys, nan)
    div = lambda x, y: float(x) / float(y) if y != 0 else nan
    q = [int(v) for v in it.into[i, p]]
    return dict(mean_lineage_size=div(q[2], q[0]), size_weighted_mean=div(q[3], q[2]), singleton_share=div(int(it.spectrum[i, p, 0]), q[0]),
                empty_share=div(q[4], q[0]), observed_share=div(int(it.imports[i, :, p].sum()), int(true_imports[i, :, p, :].sum())))


def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def test_derived_values_bit_for_bit():
    rng = np.random.default_rng(77)
    P = 4
    cases = []
    for s, move in ((2, 1.0), (3, 0.0), (9, 0.5), (40, 0.3), (200, 0.1), (64, 0.9), (120, 0.02)):
        t = random_tree(s, rng)
        cases.append((t, random_labels(t, P, rng, move), P))
    status = [0, 0, 0, 4, 0, 0, 0]
    it = introductions_of(cases, status)
    true_imports = rng.integers(0, 40, (len(cases), 3, P, 2)).astype(np.int64)   # [n, T, dst, V]
    true_imports[4, :, 1, :] = 0
    flows = _Flows(it.replicates.copy(), true_imports)
    got = dict(mean_lineage_size=it.mean_lineage_size(), size_weighted_mean=it.size_weighted_mean(), singleton_share=it.singleton_share(),
               empty_share=it.empty_share(), observed_share=it.observed_share(flows))
    finite = 0
    for i in range(len(cases)):
        for p in range(P):
            want = scalar_derived(it, i, p, true_imports)
            for k in want:
                assert got[k].shape == (len(cases), P) and got[k].dtype == np.float64
                assert same_bits(got[k][i, p], want[k]), (i, p, k, got[k][i, p], want[k])
                finite += math.isfinite(want[k])
    assert finite > 40
    assert all(np.isnan(got[k][3]).all() for k in got) and np.isnan(got["mean_lineage_size"][1]).all()   # not ok; no introduction
    assert np.isnan(got["observed_share"][4, 1])
    with pytest.raises(ValueError, match="same replicates"):
        it.observed_share(_Flows(it.replicates[::-1].copy(), true_imports))
    # the integer views
    assert it.bin_edges().tolist() == [2 ** b for b in range(32)] and it.bin_edges().dtype == np.int64
    assert np.array_equal(it.imports_into(), it.imports.sum(1)) and np.array_equal(it.imports_into(), it.into[:, :, 0])
    assert np.array_equal(it.exports_from(), it.imports.sum(2)) and np.array_equal(it.net_flow(), it.imports.sum(1) - it.imports.sum(2))
    assert not it.net_flow().sum(axis=1).any() and it.net_flow().dtype == np.int64
    lin = it.lineages()
    for i in range(len(cases)):
        want = it.into[i, :, 0].copy()
        if status[i] == 0:
            want[it.stats[i, 2]] += 1
        assert lin[i].tolist() == want.tolist()
    assert np.array_equal(lin.sum(1), np.where(it.ok, it.introductions + 1, 0)) and lin.dtype == np.int64
    for k, name in enumerate(STATS):
        assert np.array_equal(getattr(it, name), it.stats[:, k]), name
    assert it.message(3) != "" and it.message(0) == "" and it.ok.tolist() == [True, True, True, False, True, True, True]
    assert Introductions.INTO == INTO and len(INTO) == 6 and len(STATS) == 8 and Introductions.BINS == 32
