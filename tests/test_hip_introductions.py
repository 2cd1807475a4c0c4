"""Ensemble.introductions(): the lineage kernel (vgx_introductions.hip) on hand-made labelled trees through
``_capi.introductions_device`` and on the trees of ensembles, against the host sweep ``_capi.introductions`` (the definition)
applied to what ``genealogies()`` returns; both forms of the kernel (per-destination cells in LDS up to 32 populations, in the
row in global memory beyond); status, generator and messages of ``genealogies()``; skipped, malformed and badly labelled trees
among good ones; subsets, order, several passes and refusals.

Counts, sums and maxima of integers: every comparison is for equality."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _ensemble
from test_introductions_rule import assert_identities, random_labels
from test_tree_shape_rule import balanced, caterpillar, random_tree
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu

BLOCKS = ("tips_by_pop", "imports", "into", "spectrum", "stats")
FIELDS = BLOCKS + ("status", "status_arg", "rng_raw", "replicates")
LDS_POPS = 32   # VGX_IN_LDS_POPS: the last P whose per-destination cells lie in LDS


def assert_rows_equal_host(cases, P, out, rows=None):
    status = out[5]
    for i in (range(len(cases)) if rows is None else rows):
        want = _capi.introductions(*cases[i], P)
        assert tuple(status[i]) == (0, 0), (i, status[i])
        for got, w, k in zip((b[i] for b in out[:5]), want, BLOCKS):
            assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w), (i, k, got, w)
        assert_identities(tuple(b[i] for b in out[:5]), i)


def assert_zero_row(out, i):
    assert not any(b[i].any() for b in out[:5]), i


def chain_of_lineages(sizes, dst=1):
    """A caterpillar whose spine has population 0 and to which one subtree per entry of ``sizes`` is attached, itself a caterpillar
    of that many tips in population ``dst``: one introduction 0 -> dst of exactly that local size each (size 0: an internal node in
    dst whose two children are tips back in population 0)."""
    tree, pop = [], []

    def leaf(p):
        tree.append(-1)
        pop.append(p)
        return len(tree) - 1

    def join(a, b, p):
        tree.append(-1)
        pop.append(p)
        tree[a] = tree[b] = len(tree) - 1
        return len(tree) - 1

    spine = leaf(0)
    for s in sizes:
        if s == 0:
            sub = join(leaf(0), leaf(0), dst)
        else:
            sub = leaf(dst)
            for _ in range(s - 1):
                sub = join(sub, leaf(dst), dst)
        spine = join(spine, sub, 0)
    return np.asarray(tree, dtype=np.int64), np.asarray(pop, dtype=np.int64)


@pytest.mark.parametrize("P", [2, LDS_POPS + 6])
def test_smallest_trees_round_borders_and_the_caterpillar(P):
    rng = np.random.default_rng(41)
    three = np.array([2, 2, -1])
    cases = [(three, np.array(p)) for p in ([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1])]
    for N in (63, 65, 127, 129):   # both sides of the 64-node and 128-node round borders
        t = random_tree((N + 1) // 2, rng)
        assert len(t) == N
        cases += [(t, random_labels(t, P, rng, 0.3)), (t, random_labels(t, P, rng, 1.0)), (t, np.full(N, P - 1))]
    cat, bal = caterpillar(70), balanced(6)   # 64 iterations in a round; every clade a power of two
    cases += [(cat, np.arange(len(cat)) % 2), (cat, np.zeros(len(cat), int)), (bal, random_labels(bal, P, rng, 0.4))]
    out = _capi.introductions_device(cases, P)
    assert out[0].shape == (len(cases), P) and out[1].shape == (len(cases), P, P) and out[2].shape == (len(cases), P, 6)
    assert out[3].shape == (len(cases), P, 32) and out[4].shape == (len(cases), 8) and all(a.dtype == np.int64 for a in out)
    assert_rows_equal_host(cases, P, out)
    assert out[4][0].tolist() == [2, 0, 0, 2, 2, 0, 0, 1] and out[4][1].tolist() == [2, 1, 0, 1, 1, 1, 0, 2]
    assert out[4][2].tolist() == [2, 2, 0, 0, 1, 1, 0, 1]
    assert out[4][-3].tolist() == [70, 137, 0, 0, 1, 69, 67, 2]   # the caterpillar with alternating labels: lineages of size 0 or 1


@pytest.mark.parametrize("P", [1, 2, 16, 70, 256])
def test_random_trees_partial_workgroup(P):
    rng = np.random.default_rng(131 + P)
    tips = rng.integers(2, 201, 130)
    tips[:4] = (2, 3, 200, 31)
    cases = []
    for k, s in enumerate(tips):
        t = random_tree(int(s), rng)
        cases.append((t, random_labels(t, P, rng, (0.0, 0.05, 0.2, 0.6, 1.0)[k % 5])))
    assert len(cases) % 4 != 0
    out = _capi.introductions_device(cases, P)
    assert_rows_equal_host(cases, P, out)
    if P > 1:
        assert out[4][:, 1].sum() > 1000   # (the comparison is not of zeros)


@pytest.mark.parametrize("P", [3, LDS_POPS, LDS_POPS + 1])
def test_local_sizes_at_powers_of_two_contention_and_empty_lineages(P):
    """Local sizes 2^b - 1 and 2^b; 5000 introductions into one destination; every introduction empty.  P = 32 and 33: the last
    population count of the LDS form and the first of the global one."""
    dst = P - 1
    sizes = [c for b in range(1, 8) for c in (2 ** b - 1, 2 ** b)]
    sizes += sizes[::3]
    cases = [chain_of_lineages(sizes, dst), chain_of_lineages([1] * 5000, dst), chain_of_lineages([0] * 300, dst),
             chain_of_lineages([0, 3, 0, 0, 64, 1, 0], dst)]
    out = _capi.introductions_device(cases, P)
    assert_rows_equal_host(cases, P, out)
    tips_by_pop, imports, into, spectrum, stats = out[:5]
    assert spectrum[0, dst].tolist() == [sum(1 for c in sizes if c.bit_length() - 1 == b) for b in range(32)]
    assert into[0, dst].tolist() == [len(sizes), sum(sizes), sum(sizes), sum(c * c for c in sizes), 0, 128]
    assert imports[1, 0, dst] == 5000 and into[1, dst].tolist() == [5000, 5000, 5000, 5000, 0, 1] and spectrum[1, dst, 0] == 5000
    assert stats[1].tolist() == [5001, 5000, 0, 1, 1, 1, 0, 2]
    # every introduction empty: 300 into dst, and the 600 tips below them back into 0 as singletons
    assert into[2, dst].tolist() == [300, 600, 0, 0, 300, 0] and not spectrum[2, dst].any() and into[2, 0].tolist() == [600, 600, 600, 600, 0, 1]
    assert stats[2].tolist() == [601, 900, 0, 1, 1, 2, 300, 1]


def test_skipped_malformed_and_badly_labelled_trees_among_good_ones():
    rng = np.random.default_rng(5)
    for P in (3, LDS_POPS + 6):
        good = []
        for s in (40, 3, 70, 12, 90, 33):
            t = random_tree(s, rng)
            good.append((t, random_labels(t, P, rng, 0.3)))
        one_child = (np.array([2, 3, 3, 4, -1]), np.array([9999, 0, 0, 0, 0]))   # node 2 has one child; node 0's label is bad too: 13 wins
        t = random_tree(100, rng)
        N = len(t)
        bad_kinds = []
        for v, i in ((P, 150), (-1, 70), (2 ** 31 - 1, 0), (-2 ** 31, N - 1), (P + 1000, 64), (P, 63)):
            pop = random_labels(t, P, rng, 0.3)
            pop[i] = v
            bad_kinds.append(((t, pop), i))
        pop = random_labels(t, P, rng, 0.3)   # four bad labels in different 64-node steps: the lowest is reported
        pop[190], pop[129], pop[77], pop[198] = P, -3, 2 ** 20, P
        cases = [good[0], one_child, good[1]] + [good[2]] + [c for c, _ in bad_kinds[:3]] + [good[3]] + [c for c, _ in bad_kinds[3:]] + \
            [good[4], (t, pop), good[5]]
        walk = np.zeros((len(cases), 2), dtype=np.int64)
        walk[3] = (4, 17)   # good[2] is skipped: a walk that failed with status 4
        out = _capi.introductions_device(cases, P, walk_status=walk)
        status = out[5]
        assert tuple(status[1]) == (_capi.GW_BAD_TREE, 2) and "node 2" in _capi.genealogy_message(*status[1])
        assert tuple(status[3]) == (4, 17)
        rejected = [4, 5, 6, 8, 9, 10]
        for i, (_, k) in zip(rejected, bad_kinds):
            assert tuple(status[i]) == (_capi.GW_BAD_LABEL, k), (i, status[i])
            assert "node %d " % k in _capi.genealogy_message(*status[i])
        assert tuple(status[12]) == (_capi.GW_BAD_LABEL, 77)
        for i in [1, 3, 12] + rejected:
            assert_zero_row(out, i)
        assert_rows_equal_host(cases, P, out, rows=[0, 2, 7, 11, 13])   # the neighbours are unharmed
        again = _capi.introductions_device(cases, P)                    # without walk statuses nothing is skipped
        assert_rows_equal_host(cases, P, again, rows=[0, 2, 3, 7, 11, 13])
        with pytest.raises(ValueError, match="tree 1: the parent of node 1"):   # parents outside the tree never reach the device
            _capi.introductions_device([good[0], (np.array([3, 7, 3, 4, -1]), np.zeros(5, int))], P)
        with pytest.raises(ValueError, match="tree 0 has 4 nodes"):
            _capi.introductions_device([(np.array([2, 2, 3, -1]), np.zeros(4, int))], P)
    for pops in (0, _capi.INTRODUCTIONS_POPS_MAX + 1):
        with pytest.raises(ValueError, match="populations"):
            _capi.introductions_device([good[0]], pops)
    assert len(_capi.introductions_device([], 2)[0]) == 0


# ---- rows of ensembles -----------------------------------------------------------------------------------------------------------
def assert_rows_equal_genealogies(ens, it, batch):
    """Every row against the host sweep over the tree and labels genealogies() returns for the same walk.  Returns (healthy rows,
    introductions in them)."""
    healthy = intro = 0
    P = int(ens.model.popNum)
    n = len(it.replicates)
    assert it.pops == P and it.tips_by_pop.shape == (n, P) and it.imports.shape == (n, P, P) and it.into.shape == (n, P, 6)
    assert it.spectrum.shape == (n, P, 32) and it.stats.shape == (n, 8)
    assert np.array_equal(it.status, batch.status) and np.array_equal(it.status_arg, batch.status_arg)
    assert np.array_equal(it.rng_raw, batch.rng_raw) and np.array_equal(it.replicates, batch.replicates)
    for i, r in enumerate(it.replicates):
        assert it.message(i) == batch.message(i)
        if not it.ok[i]:
            assert not any(getattr(it, k)[i].any() for k in BLOCKS), r
            continue
        g = batch.replicate(int(r))
        want = _capi.introductions(g["tree"], g["tree_pop"], P)
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(it, k)[i], w), (r, k, getattr(it, k)[i], w)
        assert_identities(tuple(getattr(it, k)[i] for k in BLOCKS), r)
        assert it.tips[i] == ens.engine.counters(int(r)).reserved[4], r
        healthy += 1
        intro += int(it.introductions[i])
    return healthy, intro


def assert_derived_values(it):
    for f in (it.mean_lineage_size, it.size_weighted_mean, it.singleton_share, it.empty_share):
        assert np.isnan(f()[~it.ok]).all(), f.__name__
    assert np.array_equal(it.imports_into(), it.into[:, :, 0]) and not it.net_flow().sum(axis=1).any()
    assert np.array_equal(it.lineages().sum(axis=1), np.where(it.ok, it.introductions + 1, 0))


@pytest.mark.parametrize("name", ["c3_s5_p16", "p70", "stress_h64"])   # (p70: the global form; the others the LDS form)
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_rows_equal_the_host_sweep_over_genealogies(name, seed):
    R = 6
    ens = _ensemble(name, R)
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    log = [ens.replicate_events(r).copy() for r in range(R)]
    mismatches = ens.engine.lib.vgx_clock_mismatches(ens.engine.handle)
    it = ens.introductions(seed=s)
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == mismatches   # (no host clock runs)
    assert all(getattr(it, k).dtype == np.int64 for k in BLOCKS) and it.passes >= 1 and len(it.kernel_ms) == 2
    healthy, intro = assert_rows_equal_genealogies(ens, it, ens.genealogies(seed=s))
    print("%s seed %s: %d healthy of %d, %d introductions" % (name, seed, healthy, R, intro))
    assert 4 * healthy >= 3 * R, name
    assert intro > 0, name   # (the comparison is not of zeros)
    assert all(np.array_equal(log[r], ens.replicate_events(r)) for r in range(R))
    assert_derived_values(it)
    ens.close()


@pytest.mark.parametrize("name,chunk", [("c3_s5_p16", "400000"), ("p70", "1500000")])
def test_subsets_order_and_passes(name, chunk, monkeypatch):
    R = 40
    ens = _ensemble(name, R, seeds0=7000)
    full = ens.introductions(seed=99)
    healthy, intro = assert_rows_equal_genealogies(ens, full, ens.genealogies(seed=99))
    assert 4 * healthy >= 3 * R and intro > 0
    order = np.random.default_rng(3).permutation(R)[:13]
    seeds = 1000 + np.arange(13, dtype=np.int64)
    sub = ens.introductions(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    healthy, intro = assert_rows_equal_genealogies(ens, sub, ens.genealogies(seed=seeds, replicates=order))
    assert 4 * healthy >= 3 * 13 and intro > 0
    same = ens.introductions(seed=99, replicates=order)
    for k in FIELDS[:-1]:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", chunk)   # several device passes: same kernel, same tree, same order
    small = ens.introductions(seed=99)
    assert small.passes > 1 and full.passes == 1
    for k in FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    for name, R, kw, seed, code, text in (("recomb_a", 8, dict(n_max=3000), 21, 4, "never coalesced"),
                                          ("extinct", 24, dict(n_max=50, seeds0=1), 5, 1, "Less than two")):
        ens = _ensemble(name, R, **kw)
        it = ens.introductions(seed=seed)
        assert (it.status == code).any(), it.status
        i = int(np.nonzero(it.status == code)[0][0])
        assert text in it.message(i)
        assert_rows_equal_genealogies(ens, it, ens.genealogies(seed=seed))
        assert_derived_values(it)
        ens.close()


def test_refusals():
    ens = _ensemble("g9_short", 3, n_max=500)
    with pytest.raises(ValueError, match="out of range"):
        ens.introductions(replicates=[0, 3])
    with pytest.raises(ValueError, match="distinct"):
        ens.introductions(replicates=[1, 1])
    with pytest.raises(ValueError, match="one seed per selected replicate"):
        ens.introductions(seed=[1, 2, 3], replicates=[0, 2])
    P = int(ens.model.popNum)
    none = ens.introductions(replicates=[])
    assert none.imports.shape == (0, P, P) and none.stats.shape == (0, 8) and none.passes == 0
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"introductions\(\).*record_events"):
        ens.introductions()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"introductions\(\) walks direct chains only.*tau"):
        ens.introductions()
    ens.close()
