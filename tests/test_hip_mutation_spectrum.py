"""Ensemble.mutation_spectrum(): the spectrum kernel (vgx_mutation_spectrum.hip) on hand-made trees and records through
``_capi.mutation_spectrum_device`` and on the trees of ensembles, against the host sweep ``_capi.mutation_spectrum`` (the definition)
applied to what ``genealogies()`` returns; status, generator and messages of ``genealogies()``; skipped, malformed and rejected
trees among good ones; subsets, order, several passes, failed walks and refusals.

Counts, sums and one maximum of integers: every comparison is for equality."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _ensemble
from test_mutation_spectrum_rule import hand_made_cases, random_records
from test_tree_shape_rule import balanced, caterpillar, random_tree
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu

BLOCKS = ("spectrum", "substitutions", "sums", "stats")
FIELDS = BLOCKS + ("status", "status_arg", "rng_raw", "replicates")


def on_nodes(tree, nodes, S=1, rng=None):
    """(tree, mut_*) with one record per entry of ``nodes``."""
    M = len(nodes)
    if rng is None:
        return (tree, np.asarray(nodes, dtype=np.int64), np.zeros(M, int), np.ones(M, int), np.zeros(M, int))
    return (tree, np.asarray(nodes, dtype=np.int64), rng.integers(0, 4, M), rng.integers(0, 4, M), rng.integers(0, S, M))


def assert_rows_equal_host(cases, S, out, rows=None):
    spectrum, subs, sums, stats, status, clade = out
    for i in (range(len(cases)) if rows is None else rows):
        want = _capi.mutation_spectrum(*cases[i], S, with_clade=True)
        assert tuple(status[i]) == (0, 0), (i, status[i])
        for got, w, k in zip((spectrum[i], subs[i], sums[i], stats[i], clade[i]), want, BLOCKS + ("clade",)):
            assert got.dtype == w.dtype and np.array_equal(got, w), (i, k, got, w)


def assert_zero_row(out, i):
    assert not out[0][i].any() and not out[1][i].any() and not out[2][i].any() and not out[3][i].any(), i


def test_hand_made_cases():
    """Every case of the rule test, one launch per sites value."""
    by_sites = {}
    for label, *case in hand_made_cases():
        by_sites.setdefault(case[5], []).append(tuple(case[:5]))
    for S, cases in sorted(by_sites.items()):
        out = _capi.mutation_spectrum_device(cases, S)
        assert out[0].shape == (len(cases), S, 32) and out[1].shape == (len(cases), S, 4, 4) and out[2].shape == (len(cases), S, 3)
        assert all(a.dtype == np.int64 for a in out[:5])
        assert_rows_equal_host(cases, S, out)


def test_smallest_trees_round_borders_and_power_of_two_clades():
    rng = np.random.default_rng(41)
    three = np.array([2, 2, -1])
    cases = [on_nodes(three, []), on_nodes(three, [0, 1]), on_nodes(three, [2, 2, 2]), on_nodes(three, [1, 2, 0, 0])]
    for N in (63, 65, 127, 129):   # both sides of the 64-node and 128-node round borders
        t = random_tree((N + 1) // 2, rng)
        assert len(t) == N
        cases.append(on_nodes(t, rng.integers(0, N, 2 * N)))
        cases.append(on_nodes(t, np.arange(N)))
    cat, bal = caterpillar(70), balanced(6)   # 64 iterations in a round; every clade a power of two
    cases += [on_nodes(cat, np.arange(len(cat))), on_nodes(bal, np.arange(len(bal)))]
    # clade sizes 2^b - 1 and 2^b: internal node 70 + c - 2 of the caterpillar holds c tips
    sizes = [c for b in range(1, 7) for c in (2 ** b - 1, 2 ** b) if c >= 2]
    sizes += sizes[::2]
    cases.append(on_nodes(cat, [70 + c - 2 for c in sizes]))
    out = _capi.mutation_spectrum_device(cases, 1)
    assert_rows_equal_host(cases, 1, out)
    assert out[3][0].tolist() == [2, 0, 0, 0] and out[3][1].tolist() == [2, 2, 0, 1] and out[3][2].tolist() == [2, 3, 3, 2]
    assert out[0][-1][0].tolist() == [sum(1 for c in sizes if c.bit_length() - 1 == b) for b in range(32)]


@pytest.mark.parametrize("S", [1, 3, 15])
def test_random_trees_partial_workgroup(S):
    rng = np.random.default_rng(131 + S)
    tips = rng.integers(2, 201, 130)
    tips[:4] = (2, 3, 200, 31)
    cases = []
    for s in tips:
        t = random_tree(int(s), rng)
        N = len(t)
        M = int(rng.choice([0, 1, 63, 64, 65, int(rng.integers(0, 3 * N + 1)), 3 * N]))
        cases.append((t,) + random_records(N, M, S, rng))
    assert len(cases) % 4 != 0
    assert_rows_equal_host(cases, S, _capi.mutation_spectrum_device(cases, S))


def test_many_records_in_one_cell_and_spread():
    rng = np.random.default_rng(8)
    three = np.array([2, 2, -1])
    M = 5000
    one_cell = (three, np.full(M, 2), np.full(M, 1), np.full(M, 3), np.full(M, 14))     # every lane adds to the same cells
    spread = (three,) + random_records(3, M, 15, rng)
    cases = [one_cell, spread, one_cell]
    out = _capi.mutation_spectrum_device(cases, 15)
    assert_rows_equal_host(cases, 15, out)
    assert out[0][0][14, 1] == M and out[1][0][14, 1, 3] == M and out[2][0][14].tolist() == [2 * M, 4 * M, 0] and out[3][0].tolist() == [2, M, M, 2]


def test_skipped_malformed_and_rejected_trees_among_good_ones():
    rng = np.random.default_rng(5)
    S = 3
    good = []
    for s, M in ((40, 200), (3, 7), (70, 64), (12, 130), (90, 300), (33, 65)):
        t = random_tree(s, rng)
        good.append((t,) + random_records(len(t), M, S, rng))
    one_child = (np.array([2, 3, 3, 4, -1]),) + random_records(5, 9, S, rng)   # node 2 has one child: every parent is inside the tree
    t = random_tree(50, rng)
    N, M = len(t), 300
    bad_kinds = []
    for col, v, k in ((0, N, 150), (0, -1, 70), (1, 4, 200), (2, -1, 64), (3, S, 299), (3, -2, 0)):
        rec = [np.array(c) for c in random_records(N, M, S, rng)]
        rec[col][k] = v
        bad_kinds.append(((t,) + tuple(rec), k))
    rec = [np.array(c) for c in random_records(N, M, S, rng)]   # four bad records in different 64-record steps: the lowest is reported
    rec[0][290], rec[3][129], rec[1][77], rec[2][200] = 2 ** 31 - 1, 15, 7, 4
    cases = [good[0], one_child, good[1]] + [good[2]] + [c for c, _ in bad_kinds[:3]] + [good[3]] + [c for c, _ in bad_kinds[3:]] + \
        [good[4], (t,) + tuple(rec), good[5]]
    walk = np.zeros((len(cases), 2), dtype=np.int64)
    walk[3] = (4, 17)   # good[2] is skipped: a walk that failed with status 4
    out = _capi.mutation_spectrum_device(cases, S, walk_status=walk)
    status = out[4]
    assert tuple(status[1]) == (_capi.GW_BAD_TREE, 2) and "node 2" in _capi.genealogy_message(*status[1])
    assert tuple(status[3]) == (4, 17) and not out[5][3].any()
    rejected = [4, 5, 6, 8, 9, 10]
    for i, (_, k) in zip(rejected, bad_kinds):
        assert tuple(status[i]) == (_capi.GW_BAD_RECORD, k), (i, status[i])
        assert "record %d " % k in _capi.genealogy_message(*status[i])
    assert tuple(status[12]) == (_capi.GW_BAD_RECORD, 77)
    for i in [1, 3, 12] + rejected:
        assert_zero_row(out, i)
    assert_rows_equal_host(cases, S, out, rows=[0, 2, 7, 11, 13])   # the neighbours are unharmed
    again = _capi.mutation_spectrum_device(cases, S)                # without walk statuses nothing is skipped
    assert_rows_equal_host(cases, S, again, rows=[0, 2, 3, 7, 11, 13])
    with pytest.raises(ValueError, match="tree 1: the parent of node 1"):   # parents outside the tree never reach the device
        _capi.mutation_spectrum_device([good[0], (np.array([3, 7, 3, 4, -1]),) + good[1][1:]], S)
    with pytest.raises(ValueError, match="tree 0 has 4 nodes"):
        _capi.mutation_spectrum_device([on_nodes(np.array([2, 2, 3, -1]), [])], 1)
    with pytest.raises(ValueError, match="sites"):
        _capi.mutation_spectrum_device([good[0]], 16)
    assert len(_capi.mutation_spectrum_device([], 2)[0]) == 0


# ---- rows of ensembles -----------------------------------------------------------------------------------------------------------
def assert_rows_equal_genealogies(ens, ms, batch):
    """Every row against the host sweep over the tree and records genealogies() returns for the same walk.  Returns (healthy rows,
    records in them)."""
    healthy = records = 0
    S = int(ens.model.sites)
    assert ms.sites == S and ms.spectrum.shape == (len(ms.replicates), S, 32)
    assert np.array_equal(ms.status, batch.status) and np.array_equal(ms.status_arg, batch.status_arg)
    assert np.array_equal(ms.rng_raw, batch.rng_raw) and np.array_equal(ms.replicates, batch.replicates)
    for i, r in enumerate(ms.replicates):
        assert ms.message(i) == batch.message(i)
        if not ms.ok[i]:
            assert not any(getattr(ms, k)[i].any() for k in BLOCKS), r
            continue
        g = batch.replicate(int(r))
        want = _capi.mutation_spectrum(g["tree"], g["mut_node"], g["mut_AS"], g["mut_DS"], g["mut_site"], S)
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(ms, k)[i], w), (r, k, getattr(ms, k)[i], w)
        assert ms.tips[i] == ens.engine.counters(int(r)).reserved[4], r
        assert ms.spectrum[i].sum() == ms.mutations[i] == len(g["mut_node"]), r
        healthy += 1
        records += len(g["mut_node"])
    return healthy, records


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70"])
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_rows_equal_the_host_sweep_over_genealogies(name, seed):
    R = 6
    ens = _ensemble(name, R)
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    log = [ens.replicate_events(r).copy() for r in range(R)]
    mismatches = ens.engine.lib.vgx_clock_mismatches(ens.engine.handle)
    ms = ens.mutation_spectrum(seed=s)
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == mismatches   # (no host clock runs)
    assert all(getattr(ms, k).dtype == np.int64 for k in BLOCKS) and ms.passes >= 1 and len(ms.kernel_ms) == 2
    healthy, records = assert_rows_equal_genealogies(ens, ms, ens.genealogies(seed=s))
    assert healthy >= 1
    if name != "g9_short":   # (the comparison is not of zeros)
        assert records >= 1, name
    assert all(np.array_equal(log[r], ens.replicate_events(r)) for r in range(R))
    ok = ms.ok
    assert np.array_equal(ms.singletons()[ok], ms.spectrum[ok][:, :, 0].sum(-1)) and np.isnan(ms.pi()[~ok]).all()
    assert np.all(ms.pi()[ok] >= 0) and np.array_equal(ms.per_site().sum(-1), ms.mutations)
    ens.close()


def test_subsets_order_and_passes(monkeypatch):
    R = 130
    ens = _ensemble("g9_short", R, n_max=1500, seeds0=7000)
    full = ens.mutation_spectrum(seed=99)
    assert assert_rows_equal_genealogies(ens, full, ens.genealogies(seed=99))[0] > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.mutation_spectrum(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_rows_equal_genealogies(ens, sub, ens.genealogies(seed=seeds, replicates=order))
    same = ens.mutation_spectrum(seed=99, replicates=order)
    for k in FIELDS[:-1]:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order]), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "200000")   # several device passes: same kernel, same tree, same order
    small = ens.mutation_spectrum(seed=99)
    assert small.passes > 1 and full.passes == 1
    for k in FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k)), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    for name, R, kw, seed, code, text in (("recomb_a", 8, dict(n_max=3000), 21, 4, "never coalesced"),
                                          ("extinct", 24, dict(n_max=50, seeds0=1), 5, 1, "Less than two")):
        ens = _ensemble(name, R, **kw)
        ms = ens.mutation_spectrum(seed=seed)
        assert (ms.status == code).any(), ms.status
        i = int(np.nonzero(ms.status == code)[0][0])
        assert text in ms.message(i)
        assert_rows_equal_genealogies(ens, ms, ens.genealogies(seed=seed))
        bad = ~ms.ok
        for f in (ms.singleton_share, ms.pi, ms.watterson, ms.theta_h, ms.fay_wu_h, ms.tajimas_d):
            assert np.isnan(f()[bad]).all(), f.__name__
        ens.close()


def test_refusals():
    ens = _ensemble("g9_short", 3, n_max=500)
    with pytest.raises(ValueError, match="out of range"):
        ens.mutation_spectrum(replicates=[0, 3])
    with pytest.raises(ValueError, match="distinct"):
        ens.mutation_spectrum(replicates=[1, 1])
    with pytest.raises(ValueError, match="one seed per selected replicate"):
        ens.mutation_spectrum(seed=[1, 2, 3], replicates=[0, 2])
    none = ens.mutation_spectrum(replicates=[])
    assert none.spectrum.shape == (0, ens.model.sites, 32) and none.stats.shape == (0, 4) and none.passes == 0
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"mutation_spectrum\(\).*record_events"):
        ens.mutation_spectrum()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"mutation_spectrum\(\) walks direct chains only.*tau"):
        ens.mutation_spectrum()
    ens.close()
