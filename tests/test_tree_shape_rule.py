"""The rule of vgx_tree_shape.h on the host (``_capi.tree_shape``, the sequential sweep behind ``Ensemble.tree_shapes``) against a
pure-Python restatement of its recurrences written here, closed forms for caterpillar and balanced trees, a brute-force walk from
every tip to the root, and numpy for the lengths; the trees it refuses.  No GPU.

The four length sums are sums of m <= N non-negative correctly rounded terms: two summations of them in any order differ by at
most 2 (m + 2) 2^-53 S, so they are held to |got - want| <= 2 (N + 2) 2^-53 want against numpy's sum.  Everything else is
asserted with equality."""
import functools
import glob
import os

import numpy as np
import pytest

from vgsim_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS, LENGTHS = _capi.TREE_SHAPE_STATS, _capi.TREE_SHAPE_LENGTHS
EXACT, SUMS = (0, 1, 6), (2, 3, 4, 5)


# ---- trees in creation order: every parent has a higher id than its children, the root is the last node -------------------------
def _dress(tree, rng=None):
    """(tree, node_ev, times): decreasing event indices and node times that do not increase with the id (some equal)."""
    N = len(tree)
    if rng is None:
        steps = np.ones(N)
    else:
        steps = rng.exponential(1.0, N) * (rng.random(N) > 0.15)   # (ties: several nodes at one time)
    times = np.cumsum(steps)[::-1].copy()
    node_ev = (np.cumsum(1 + (np.zeros(N, dtype=np.int64) if rng is None else rng.integers(0, 5, N)))[::-1] - 1).copy()
    return np.asarray(tree, dtype=np.int64), node_ev, times


def caterpillar(s):
    """Tips 0 .. s-1 first, then the s - 1 internal nodes: tips 0 and 1 under node s, tip k and node s + k - 2 under node s + k - 1."""
    tree = np.full(2 * s - 1, -1, dtype=np.int64)
    tree[0] = tree[1] = s
    for k in range(2, s):
        tree[k] = tree[s + k - 2] = s + k - 1
    return tree


def balanced(k):
    """2^k tips, then level after level."""
    tree, level, nxt = [-1] * (2 ** (k + 1) - 1), list(range(2 ** k)), 2 ** k
    while len(level) > 1:
        up = []
        for a, b in zip(level[::2], level[1::2]):
            tree[a] = tree[b] = nxt
            up.append(nxt)
            nxt += 1
        level = up
    return np.asarray(tree, dtype=np.int64)


def random_tree(s, rng):
    """A random binary tree of s tips the way a backward walk makes one: a new node is a sampled tip or joins two random lineages."""
    tree, active, left = [], [], s
    while left > 0 or len(active) > 1:
        node = len(tree)
        tree.append(-1)
        if left > 0 and (len(active) < 2 or rng.random() < 0.5):
            left -= 1
        else:
            for _ in range(2):
                tree[active.pop(int(rng.integers(len(active))))] = node
        active.append(node)
    return np.asarray(tree, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def hand_made_trees():
    """(label, tree, node_ev, times) of every tree of this file: the closed forms, the random trees (N on both sides of the 64-node
    and 128-node round borders of the kernel) and the genealogy goldens."""
    rng = np.random.default_rng(29)
    out = []
    for s in (2, 3, 5, 70):
        out.append(("caterpillar_%d" % s,) + _dress(caterpillar(s)))
    for k in (1, 2, 6):
        out.append(("balanced_%d" % 2 ** k,) + _dress(balanced(k)))
    for s in (2, 3, 32, 33, 64, 65, 200):
        out.append(("random_%d" % s,) + _dress(random_tree(s, rng), rng))
    for path in sorted(glob.glob(os.path.join(GOLDEN, "genealogy_*.npz"))):
        z = np.load(path)
        N = len(z["tree"])
        out.append((os.path.basename(path), z["tree"].astype(np.int64), np.arange(N, 0, -1, dtype=np.int64) * 3, z["times"].astype(np.float64)))
    return tuple(out)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def restate(tree, node_ev):
    """The integer block by the recurrences of the rule, node after node in ascending id, in Python integers."""
    N = len(tree)
    kids = [[] for _ in range(N)]
    for i in range(N - 1):
        kids[int(tree[i])].append(i)
    n, A, B, h, lad = [0] * N, [0] * N, [0] * N, [0] * N, [0] * N
    st = dict.fromkeys(STATS, 0)
    for v in range(N):
        c = kids[v]
        if not c:
            n[v] = 1
            st["tips"] += 1
            continue
        assert len(c) == 2 and all(x < v for x in c)
        n[v] = sum(n[x] for x in c)
        A[v] = sum(A[x] + n[x] for x in c)
        B[v] = sum(B[x] + 2 * A[x] + n[x] for x in c)
        h[v] = 1 + max(h[x] for x in c)
        tipkids = sum(1 for x in c if not kids[x])
        lad[v] = 1 + max(lad[x] for x in c) if tipkids == 1 else 0
        st["internal"] += 1
        st["cherries"] += tipkids == 2
        st["pitchforks"] += n[v] == 3
        st["colless"] += n[v] - 2 * min(n[x] for x in c)
        st["ladder_nodes"] += tipkids == 1
        st["max_ladder"] = max(st["max_ladder"], lad[v])
    st["sackin"], st["depth_sumsq"], st["max_depth"] = A[N - 1], B[N - 1], h[N - 1]
    st["root_event"], st["last_tip_event"] = int(node_ev[N - 1]), int(node_ev[0])
    return np.array([st[k] for k in STATS], dtype=np.int64)


def brute_depths(tree):
    """Depth of every tip by walking up to the root."""
    N = len(tree)
    has_kid = np.zeros(N, dtype=bool)
    has_kid[tree[:-1]] = True
    depths = []
    for i in np.nonzero(~has_kid)[0]:
        d, v = 0, int(i)
        while tree[v] >= 0:
            v, d = int(tree[v]), d + 1
        depths.append(d)
    return np.array(depths, dtype=np.int64)


def numpy_lengths(tree, times):
    N = len(tree)
    has_kid = np.zeros(N, dtype=bool)
    has_kid[tree[:-1]] = True
    b = times[:-1] - times[tree[:-1]]
    tip = ~has_kid[:-1]
    return np.array([times[N - 1], times[0], b.sum(), b[tip].sum(), (b * b).sum(), (times[:-1][tip] - times[N - 1]).sum(), b.max()])


def assert_lengths(got, want, N, what):
    """The exact lengths bit for bit, the sums within 2 (N + 2) 2^-53 of numpy's."""
    for k in EXACT:
        assert got[k] == want[k], (what, LENGTHS[k], got[k], want[k])
    for k in SUMS:
        assert abs(got[k] - want[k]) <= 2 * (N + 2) * 2.0 ** -53 * want[k], (what, LENGTHS[k], got[k], want[k])


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_every_tree_equals_the_restatement_the_brute_force_walk_and_numpy():
    for label, tree, node_ev, times in hand_made_trees():
        stats, lengths = _capi.tree_shape(tree, node_ev, times)
        assert stats.dtype == np.int64 and stats.shape == (12,) and lengths.dtype == np.float64 and lengths.shape == (7,)
        assert np.array_equal(stats, restate(tree, node_ev)), label
        st = dict(zip(STATS, (int(x) for x in stats)))
        d = brute_depths(tree)
        assert (st["tips"], st["sackin"], st["depth_sumsq"], st["max_depth"]) == (len(d), d.sum(), (d * d).sum(), d.max()), label
        assert np.all(np.diff(times) <= 0), label   # (the rule's precondition: branches are non-negative)
        assert_lengths(lengths, numpy_lengths(tree, times), len(tree), label)
        # identities of every binary tree
        ln = dict(zip(LENGTHS, lengths))
        assert st["tips"] == st["internal"] + 1 == (len(tree) + 1) // 2, label
        assert st["cherries"] >= 1 and st["ladder_nodes"] + st["cherries"] <= st["internal"], label
        assert ln["length"] >= ln["external_length"] >= 0 and ln["max_branch"] <= ln["length"], label


@pytest.mark.parametrize("s", [2, 3, 5, 70])
def test_caterpillar_closed_forms(s):
    st = dict(zip(STATS, _capi.tree_shape(*_dress(caterpillar(s)))[0]))
    assert st["tips"] == s and st["sackin"] == s * (s + 1) // 2 - 1 and st["colless"] == (s - 1) * (s - 2) // 2
    assert st["cherries"] == 1 and st["max_ladder"] == s - 2 == st["ladder_nodes"] and st["max_depth"] == s - 1
    assert st["pitchforks"] == (1 if s >= 3 else 0)
    assert st["depth_sumsq"] == sum(d * d for d in range(1, s)) + (s - 1) ** 2


@pytest.mark.parametrize("k", [1, 2, 6])
def test_balanced_closed_forms(k):
    st = dict(zip(STATS, _capi.tree_shape(*_dress(balanced(k)))[0]))
    assert st["tips"] == 2 ** k and st["colless"] == 0 and st["sackin"] == k * 2 ** k and st["cherries"] == 2 ** (k - 1)
    assert st["max_depth"] == k and st["depth_sumsq"] == k * k * 2 ** k and st["ladder_nodes"] == 0 == st["max_ladder"]
    assert st["pitchforks"] == 0


def test_golden_tree_figures():
    """The figures of genealogy_c3_s5_p16_seed15.npz, re-derived by the restatement here and equal to the hook's."""
    z = np.load(os.path.join(GOLDEN, "genealogy_c3_s5_p16_seed15.npz"))
    tree = z["tree"].astype(np.int64)
    node_ev = np.arange(len(tree), 0, -1)
    want = dict(zip(STATS, (int(x) for x in restate(tree, node_ev))))
    assert {k: want[k] for k in ("tips", "cherries", "pitchforks", "colless", "sackin", "depth_sumsq", "max_depth", "ladder_nodes", "max_ladder")} == \
        dict(tips=175, cherries=55, pitchforks=29, colless=874, sackin=1786, depth_sumsq=20096, max_depth=17, ladder_nodes=65, max_ladder=3)
    assert np.array_equal(_capi.tree_shape(tree, node_ev, z["times"])[0], restate(tree, node_ev))


def test_malformed_trees_are_refused_with_the_node():
    for name in ("forest_recomb_a_seed21.npz", "forest_recomb_pos_seed22.npz"):
        z = np.load(os.path.join(GOLDEN, name))
        with pytest.raises(ValueError, match=r"node \d+"):
            _capi.tree_shape(z["tree"], np.arange(len(z["tree"]), 0, -1), z["times"])

    def refused(tree, node):
        N = len(tree)
        with pytest.raises(ValueError, match=r"node %d\b" % node):
            _capi.tree_shape(tree, np.arange(N, 0, -1), np.arange(N, 0, -1, dtype=np.float64))
    refused([3, 1, 3, 4, -1], 1)          # tree[i] <= i
    refused([3, 3, 1, 4, -1], 2)          # a parent of a lower id
    refused([3, 5, 3, 4, -1], 1)          # a parent outside the tree
    refused([2, 3, 3, 4, 4], 4)           # the last node is not a root
    refused([2, 3, 3, 4, -1], 2)          # node 2 has one child
    refused([3, 3, 3, 4, -1], 3)          # node 3 has three children
    refused([2, 2, 3, -1], 4)             # an even number of nodes
    refused([-1], 1)                      # one node
    good = _capi.tree_shape([2, 2, -1], [5, 4, 1], [3.0, 2.0, 0.5])   # (the smallest tree passes)
    assert list(good[0]) == [2, 1, 1, 0, 2, 0, 1, 2, 0, 0, 1, 5] and list(good[1]) == [0.5, 3.0, 4.0, 4.0, 8.5, 4.0, 2.5]
