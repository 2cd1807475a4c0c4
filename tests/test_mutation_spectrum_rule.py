"""The rule of vgx_mutation_spectrum.h on the host (``_capi.mutation_spectrum``, the sequential sweep behind
``Ensemble.mutation_spectrum``) against a plain-Python restatement written here that finds every clade by walking from every tip to
the root and marking its ancestors, closed forms for caterpillar and balanced trees, the figures of the genealogy goldens, the
records and trees it refuses, and the derived values of ``MutationSpectrum`` against a scalar restatement.  No GPU.

Every output is a count, a sum or a maximum of integers: everything here is asserted with equality; the derived values (float64
from the integer blocks by a fixed sequence of operations) are asserted bit for bit."""
import functools
import glob
import math
import os

import numpy as np
import pytest

from test_tree_shape_rule import balanced, caterpillar, random_tree
from vgsim_amd import _capi
from vgsim_amd.ensemble import MutationSpectrum

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUMS, STATS = _capi.MUTATION_SPECTRUM_SUMS, _capi.MUTATION_SPECTRUM_STATS
GOLDEN_SITES = {"c3_s5_p16_seed15": 5, "stress_h64_seed14": 3, "tau_b_seed19": 2}   # (the models' sites; elsewhere: the highest site used)


def golden(name):
    """(tree, mut_node, mut_AS, mut_DS, mut_site, sites) of tests/golden/genealogy_<name>.npz."""
    z = np.load(os.path.join(GOLDEN, "genealogy_%s.npz" % name))
    site = z["mut_site"].astype(np.int64)
    sites = GOLDEN_SITES.get(name, int(site.max()) + 1 if len(site) else 1)
    return z["tree"].astype(np.int64), z["mut_node"].astype(np.int64), z["mut_AS"].astype(np.int64), z["mut_DS"].astype(np.int64), site, sites


def random_records(N, M, S, rng):
    """M records on random nodes (the root included, repeats on one node) of a tree of N nodes and a model of S sites."""
    return (rng.integers(0, N, M), rng.integers(0, 4, M), rng.integers(0, 4, M), rng.integers(0, S, M))


@functools.lru_cache(maxsize=None)
def hand_made_cases():
    """(label, tree, mut_node, mut_AS, mut_DS, mut_site, sites) of every case of this file."""
    rng = np.random.default_rng(31)
    out = []
    for s in (2, 3, 5, 70):
        t = caterpillar(s)
        out.append(("caterpillar_%d" % s, t, np.arange(len(t)), np.zeros(len(t), int), np.ones(len(t), int), np.zeros(len(t), int), 1))
    for k in (1, 2, 6):
        t = balanced(k)
        out.append(("balanced_%d" % 2 ** k, t, np.arange(len(t)), np.zeros(len(t), int), np.ones(len(t), int), np.zeros(len(t), int), 1))
    for s, M, S in ((2, 0, 1), (2, 5, 3), (3, 64, 15), (32, 63, 1), (33, 65, 3), (64, 300, 15), (65, 1, 2), (200, 1197, 15)):
        t = random_tree(s, rng)
        out.append(("random_%d_%d_%d" % (s, M, S), t) + random_records(len(t), M, S, rng) + (S,))
    for path in sorted(glob.glob(os.path.join(GOLDEN, "genealogy_*.npz"))):
        name = os.path.basename(path)[len("genealogy_"):-len(".npz")]
        out.append((name,) + golden(name))
    return tuple(out)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def brute_clades(tree):
    """Tips below every node: from every tip up to the root, every node on the way gains one."""
    N = len(tree)
    has_kid = np.zeros(N, dtype=bool)
    has_kid[np.asarray(tree[:-1], dtype=np.int64)] = True
    clade = [0] * N
    for i in np.nonzero(~has_kid)[0]:
        v = int(i)
        while v >= 0:
            clade[v] += 1
            v = int(tree[v])
    return clade


def restate(tree, mut_node, mut_AS, mut_DS, mut_site, sites):
    """The four blocks in Python integers (the sums reduced to int64 as the rule's wrapping sums are)."""
    clade = brute_clades(tree)
    tips = clade[len(tree) - 1]
    spectrum = [[0] * 32 for _ in range(sites)]
    subs = [[[0] * 4 for _ in range(4)] for _ in range(sites)]
    sums = [[0] * 3 for _ in range(sites)]
    fixed = max_clade = 0
    for node, a, d, s in zip(mut_node, mut_AS, mut_DS, mut_site):
        c = clade[int(node)]
        spectrum[s][c.bit_length() - 1] += 1
        subs[s][a][d] += 1
        sums[s][0] += c
        sums[s][1] += c * c
        sums[s][2] += c * (tips - c)
        fixed += c == tips
        max_clade = max(max_clade, c)
    wrap = lambda x: (x + 2 ** 63) % 2 ** 64 - 2 ** 63
    return (np.array(spectrum, dtype=np.int64), np.array(subs, dtype=np.int64), np.array([[wrap(x) for x in r] for r in sums], dtype=np.int64),
            np.array([tips, len(mut_node), fixed, max_clade], dtype=np.int64), np.array(clade, dtype=np.int32))


def assert_blocks_equal(got, want, what):
    for g, w, k in zip(got, want, ("spectrum", "substitutions", "sums", "stats", "clade")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k, g, w)


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_every_case_equals_the_restatement():
    for label, *case in hand_made_cases():
        got = _capi.mutation_spectrum(*case, with_clade=True)
        assert_blocks_equal(got, restate(*case), label)
        spectrum, subs, sums, stats = got[:4]
        M, tips = len(case[1]), (len(case[0]) + 1) // 2
        assert stats[0] == tips and stats[1] == M == spectrum.sum() == subs.sum(), label
        assert not spectrum[:, 31].any() and stats[2] <= M and 0 <= stats[3] <= tips, label
        assert np.array_equal(sums[:, 0] * tips - sums[:, 1], sums[:, 2]), label   # sum c (tips - c) = tips sum c - sum c^2
        assert _capi.mutation_spectrum(*case)[3].tolist() == stats.tolist() and len(_capi.mutation_spectrum(*case)) == 4


@pytest.mark.parametrize("s", [2, 3, 5, 70])
def test_caterpillar_closed_forms(s):
    """One record on every node: clade sizes 1 (s times) and 2 .. s once each."""
    t = caterpillar(s)
    N = len(t)
    spectrum, subs, sums, stats = _capi.mutation_spectrum(t, np.arange(N), np.zeros(N, int), np.ones(N, int), np.zeros(N, int), 1)
    want = [0] * 32
    want[0] = s
    for c in range(2, s + 1):
        want[c.bit_length() - 1] += 1
    assert spectrum[0].tolist() == want
    assert stats.tolist() == [s, N, 1, s]
    sizes = [1] * s + list(range(2, s + 1))
    assert sums[0].tolist() == [sum(sizes), sum(c * c for c in sizes), sum(c * (s - c) for c in sizes)]
    assert subs[0, 0, 1] == N and subs.sum() == N


@pytest.mark.parametrize("k", [1, 2, 6])
def test_balanced_closed_forms(k):
    """One record on every node of a balanced tree of 2^k tips: 2^(k - j) records of clade size 2^j, in bin j."""
    t = balanced(k)
    N = len(t)
    spectrum, subs, sums, stats = _capi.mutation_spectrum(t, np.arange(N), np.zeros(N, int), np.ones(N, int), np.zeros(N, int), 1)
    assert spectrum[0].tolist() == [2 ** (k - j) for j in range(k + 1)] + [0] * (31 - k)
    assert stats.tolist() == [2 ** k, N, 1, 2 ** k]
    assert sums[0, 0] == (k + 1) * 2 ** k and sums[0, 1] == sum(2 ** (k - j) * 4 ** j for j in range(k + 1))


def _figures(name):
    spectrum, subs, sums, stats = _capi.mutation_spectrum(*golden(name))
    bins = spectrum.sum(axis=0).tolist()
    while bins and bins[-1] == 0:
        bins.pop()
    return dict(tips=int(stats[0]), M=int(stats[1]), fixed=int(stats[2]), max_clade=int(stats[3]), bins=bins, sums=sums.sum(axis=0).tolist(),
                per_site=spectrum.sum(axis=1).tolist(), subs=subs)


def test_golden_figures():
    """The figures of the genealogy goldens, pinned."""
    f = _figures("c3_s5_p16_seed15")
    assert (f["tips"], f["M"], f["bins"], f["sums"], f["max_clade"], f["fixed"]) == (175, 11, [7, 2, 0, 1, 1], [47, 813, 7412], 27, 0)
    assert f["per_site"] == [2, 3, 2, 3, 1] and f["subs"].sum(axis=0)[0].tolist() == [0, 5, 3, 3]
    f = _figures("stress_h64_seed14")
    assert (f["tips"], f["M"], f["bins"], f["sums"], f["max_clade"], f["fixed"]) == \
        (1262, 1955, [1310, 385, 111, 67, 39, 9, 8, 5, 14, 1, 6], [20073, 12551729, 12780397], 1261, 0)
    assert f["per_site"] == [611, 671, 673]
    z = np.load(os.path.join(GOLDEN, "genealogy_stress_h64_seed14.npz"))
    assert len(z["mut_node"]) - len(np.unique(z["mut_node"])) == 820   # (several records on one node are several records)
    f = _figures("p70_seed17")
    assert (f["tips"], f["M"], f["bins"], f["sums"], f["max_clade"]) == (195, 58, [39, 14, 3, 1, 0, 0, 1], [155, 4477, 25748], 65)
    f = _figures("g9_short_seed13")
    assert (f["tips"], f["M"], f["bins"]) == (233, 3, [1, 0, 1, 0, 0, 0, 0, 1])
    f = _figures("tau_b_seed19")
    assert (f["tips"], f["M"], f["bins"], f["sums"][0], f["sums"][2], f["per_site"]) == (230, 7, [4, 1, 2], 19, 4283, [2, 5])
    f = _figures("tau_c_seed20")
    assert (f["tips"], f["M"], f["bins"], f["sums"][2]) == (396, 7, [7], 2765)


@pytest.mark.parametrize("name", ["tau_a_seed18", "g1_short_seed11", "g7_short_seed12", "continuation_seed16"])
def test_goldens_without_records_give_zero_blocks_with_tips(name):
    case = golden(name)
    assert len(case[1]) == 0
    spectrum, subs, sums, stats = _capi.mutation_spectrum(*case)
    assert not spectrum.any() and not subs.any() and not sums.any()
    assert stats.tolist() == [(len(case[0]) + 1) // 2, 0, 0, 0]


def test_bad_records_are_refused_with_the_record():
    rng = np.random.default_rng(7)
    tree = random_tree(20, rng)
    N, S = len(tree), 3
    cols = [np.array(c) for c in random_records(N, 50, S, rng)]
    for col, values in ((0, (-1, N, 2 ** 31 - 1)), (1, (-1, 4)), (2, (-1, 4)), (3, (-1, S, 15))):
        for v in values:
            for k in (0, 17, 49):
                bad = [c.copy() for c in cols]
                bad[col][k] = v
                with pytest.raises(ValueError, match=r"record %d\b" % k):
                    _capi.mutation_spectrum(tree, *bad, S)
    bad = [c.copy() for c in cols]
    bad[3][40], bad[0][12], bad[1][30] = S, N, 9
    with pytest.raises(ValueError, match=r"record 12\b"):   # (the lowest of several)
        _capi.mutation_spectrum(tree, *bad, S)
    for sites in (-1, 16):
        with pytest.raises(ValueError, match="sites"):
            _capi.mutation_spectrum(tree, *cols, sites)
    with pytest.raises(ValueError, match=r"record 0\b"):   # a model without sites accepts no record ...
        _capi.mutation_spectrum(tree, *cols, 0)
    none = _capi.mutation_spectrum(tree, *[c[:0] for c in cols], 0)   # ... and gives empty per-site blocks with tips set
    assert none[0].shape == (0, 32) and none[1].shape == (0, 4, 4) and none[2].shape == (0, 3) and none[3].tolist() == [20, 0, 0, 0]
    assert _capi.mutation_spectrum(tree, *cols, S)[3][1] == 50


def test_malformed_trees_are_refused_with_the_node():
    none = (np.zeros(0, int),) * 4
    for name in ("forest_recomb_a_seed21.npz", "forest_recomb_pos_seed22.npz"):
        z = np.load(os.path.join(GOLDEN, name))
        with pytest.raises(ValueError, match=r"node \d+"):
            _capi.mutation_spectrum(z["tree"], *none, 1)

    def refused(tree, node):
        with pytest.raises(ValueError, match=r"node %d\b" % node):
            _capi.mutation_spectrum(tree, *none, 1)
    refused([3, 1, 3, 4, -1], 1)          # tree[i] <= i
    refused([3, 5, 3, 4, -1], 1)          # a parent outside the tree
    refused([2, 3, 3, 4, 4], 4)           # the last node is not a root
    refused([2, 3, 3, 4, -1], 2)          # node 2 has one child
    refused([3, 3, 3, 4, -1], 3)          # node 3 has three children
    refused([2, 2, 3, -1], 4)             # an even number of nodes
    refused([-1], 1)                      # one node
    spectrum, subs, sums, stats, clade = _capi.mutation_spectrum([2, 2, -1], [0, 2, 2], [0, 1, 1], [1, 2, 3], [0, 1, 1], 2, with_clade=True)
    assert clade.tolist() == [1, 1, 2] and stats.tolist() == [2, 3, 2, 2]
    assert spectrum[0, 0] == 1 and spectrum[1, 1] == 2 and spectrum.sum() == 3
    assert subs[0, 0, 1] == 1 and subs[1, 1, 2] == 1 and subs[1, 1, 3] == 1 and sums.tolist() == [[1, 1, 1], [4, 8, 0]]
    assert _capi.genealogy_message(_capi.GW_BAD_RECORD, 12).startswith("vgx_get_mutation_spectrum: mutation record 12 ")
    assert _capi.GW_BAD_RECORD == 14 and _capi.GW_BAD_TREE == 13


# ---- the derived values ----------------------------------------------------------------------------------------------------------
def spectrum_of(cases, status=None):
    """A MutationSpectrum over given (tree, mut_*, sites) cases of ONE sites value, built from the host hook's blocks."""
    blocks = [_capi.mutation_spectrum(*c) for c in cases]
    ms = MutationSpectrum()
    ms.sites = cases[0][5]
    ms.replicates = np.arange(len(cases), dtype=np.int64)
    ms.spectrum, ms.substitutions, ms.sums, ms.stats = (np.stack([b[k] for b in blocks]) for k in range(4))
    ms.status = np.zeros(len(cases), dtype=np.int64) if status is None else np.asarray(status, dtype=np.int64)
    ms.status_arg = np.zeros(len(cases), dtype=np.int64)
    for i in np.nonzero(ms.status)[0]:   # (a failed walk's row: zeros)
        ms.spectrum[i], ms.substitutions[i], ms.sums[i], ms.stats[i] = 0, 0, 0, 0
    return ms


def scalar_derived(ms, i):
    """Row i's derived values in Python floats, in the operation order of MutationSpectrum."""
    nan = float("nan")
    if ms.status[i] != 0:
        return dict.fromkeys(("singleton_share", "pi", "watterson", "theta_h", "fay_wu_h", "tajimas_d"), nan)
    n, S = float(ms.stats[i, 0]), float(ms.stats[i, 1])
    pairs = n * (n - 1.0)
    a1 = a2 = 0.0
    for j in range(1, int(ms.stats[i, 0])):
        a1, a2 = a1 + 1.0 / float(j), a2 + 1.0 / (float(j) * float(j))
    div = lambda x, y: x / y if y != 0 else nan
    out = dict(singleton_share=div(float(int(ms.spectrum[i, :, 0].sum())), S),
               pi=div(2.0 * float(int(ms.sums[i, :, 2].sum())), pairs),
               watterson=div(S, a1),
               theta_h=div(2.0 * float(int(ms.sums[i, :, 1].sum())), pairs))
    out["fay_wu_h"] = out["pi"] - out["theta_h"]
    out["tajimas_d"] = nan
    if n > 1 and a1 != 0:
        b1 = (n + 1.0) / (3.0 * (n - 1.0))
        b2 = 2.0 * (n * n + n + 3.0) / (9.0 * n * (n - 1.0))
        c1 = b1 - 1.0 / a1
        c2 = b2 - (n + 2.0) / (a1 * n) + a2 / (a1 * a1)
        e1 = c1 / a1
        e2 = c2 / (a1 * a1 + a2)
        var = e1 * S + e2 * S * (S - 1.0)
        d = out["pi"] - out["watterson"]
        if math.isfinite(var) and var > 0 and math.isfinite(d):
            out["tajimas_d"] = d / math.sqrt(var)
    return out


def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def test_derived_values_bit_for_bit():
    rng = np.random.default_rng(77)
    S = 3
    cases = []
    for s, M in ((2, 4), (3, 0), (9, 30), (40, 7), (200, 900), (64, 1)):
        t = random_tree(s, rng)
        cases.append((t,) + random_records(len(t), M, S, rng) + (S,))
    cases.append(golden("stress_h64_seed14"))
    status = [0, 0, 0, 4, 0, 0, 0]
    ms = spectrum_of(cases, status)
    got = dict(singleton_share=ms.singleton_share(), pi=ms.pi(), watterson=ms.watterson(), theta_h=ms.theta_h(), fay_wu_h=ms.fay_wu_h(),
               tajimas_d=ms.tajimas_d())
    for i in range(len(cases)):
        want = scalar_derived(ms, i)
        for k in want:
            assert same_bits(got[k][i], want[k]), (i, k, got[k][i], want[k])
    # NaN cases: a replicate that is not ok, and no records
    assert all(math.isnan(got[k][3]) for k in got)
    assert math.isnan(got["singleton_share"][1]) and math.isnan(got["tajimas_d"][1]) and got["pi"][1] == 0.0 == got["watterson"][1]
    assert np.isfinite(got["tajimas_d"][[2, 4, 6]]).all()
    # the integer views
    assert ms.bin_edges().tolist() == [2 ** b for b in range(32)] and ms.bin_edges().dtype == np.int64
    assert np.array_equal(ms.per_site(), ms.spectrum.sum(-1)) and np.array_equal(ms.singletons(), ms.spectrum[:, :, 0].sum(-1))
    assert np.array_equal(ms.substitution_matrix(), ms.substitutions.sum(1)) and ms.substitution_matrix().shape == (len(cases), 4, 4)
    assert np.array_equal(ms.tips, ms.stats[:, 0]) and np.array_equal(ms.mutations, ms.stats[:, 1])
    assert np.array_equal(ms.fixed, ms.stats[:, 2]) and np.array_equal(ms.max_clade, ms.stats[:, 3])
    per = ms.pi(per_site=True)
    assert per.shape == (len(cases), S) and np.isnan(per[3]).all()
    for i in (0, 2, 4, 6):
        n = float(ms.tips[i])
        assert all(same_bits(per[i, s], 2.0 * float(ms.sums[i, s, 2]) / (n * (n - 1.0))) for s in range(S))
    assert ms.message(3) != "" and ms.message(0) == "" and ms.ok.tolist() == [True, True, True, False, True, True, True]
