"""Ensemble.tree_shapes(): the shape kernel (vgx_tree_shapes.hip) on hand-made trees through ``_capi.tree_shape_device`` and on the
trees of ensembles, against the host sweep ``_capi.tree_shape`` applied to what ``genealogies()`` returns: integers and the exact
lengths bit for bit, the four length sums within 2 (N + 2) 2^-53 of numpy's sum (the bound derived in test_tree_shape_rule.py);
status, generator and messages of ``genealogies()``; subsets, order, several passes, failed walks and refusals."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_genealogy import _ensemble
from test_tree_shape_rule import EXACT, _dress, assert_lengths, hand_made_trees, numpy_lengths, random_tree
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu


def assert_rows_equal_host(trees, stats, lengths, status):
    for i, (tree, node_ev, times) in enumerate(trees):
        want_stats, want_lengths = _capi.tree_shape(tree, node_ev, times)
        assert tuple(status[i]) == (0, 0), i
        assert np.array_equal(stats[i], want_stats), (i, stats[i], want_stats)
        assert all(lengths[i][k] == want_lengths[k] for k in EXACT), i
        assert_lengths(lengths[i], numpy_lengths(np.asarray(tree), np.asarray(times)), len(tree), i)


def test_hand_made_trees_in_one_launch():
    trees = [t[1:] for t in hand_made_trees()]
    stats, lengths, status = _capi.tree_shape_device(trees)
    assert stats.shape == (len(trees), 12) and lengths.shape == (len(trees), 7)
    assert_rows_equal_host(trees, stats, lengths, status)


def test_random_trees_partial_workgroup_and_short_wavefronts():
    rng = np.random.default_rng(131)
    tips = rng.integers(2, 201, 130)
    tips[:4] = (2, 3, 200, 31)   # (a wavefront with fewer nodes than lanes, and the largest)
    trees = [_dress(random_tree(int(s), rng), rng) for s in tips]
    assert len(trees) % 4 != 0
    stats, lengths, status = _capi.tree_shape_device(trees)
    assert_rows_equal_host(trees, stats, lengths, status)


def test_malformed_tree_among_good_ones():
    rng = np.random.default_rng(5)
    good = [_dress(random_tree(s, rng), rng) for s in (40, 3, 70)]
    one_child = _dress(np.array([2, 3, 3, 4, -1]))   # node 2 has one child, node 3 two, node 4 one: every parent is inside the tree
    trees = [good[0], one_child, good[1], good[2]]
    stats, lengths, status = _capi.tree_shape_device(trees)
    assert tuple(status[1]) == (_capi.GW_BAD_TREE, 2)
    assert not stats[1].any() and np.isnan(lengths[1]).all()
    assert "node 2" in _capi.genealogy_message(*status[1])
    keep = [0, 2, 3]
    assert_rows_equal_host(good, stats[keep], lengths[keep], status[keep])
    with pytest.raises(ValueError, match="tree 1: the parent of node 1"):   # parents outside the tree never reach the device
        _capi.tree_shape_device([good[0], _dress(np.array([3, 7, 3, 4, -1]))])
    with pytest.raises(ValueError, match="tree 0 has 4 nodes"):
        _capi.tree_shape_device([_dress(np.array([2, 2, 3, -1]))])


def assert_rows_equal_genealogies(ens, ts, batch):
    """Every row against the host sweep over the tree genealogies() returns for the same walk."""
    healthy = 0
    assert np.array_equal(ts.status, batch.status) and np.array_equal(ts.status_arg, batch.status_arg)
    assert np.array_equal(ts.rng_raw, batch.rng_raw) and np.array_equal(ts.replicates, batch.replicates)
    for i, r in enumerate(ts.replicates):
        assert ts.message(i) == batch.message(i)
        if not ts.ok[i]:
            assert not ts.stats[i].any() and np.isnan(ts.lengths[i]).all(), r
            continue
        g = batch.replicate(int(r))
        N = len(g["tree"])
        want_stats, want_lengths = _capi.tree_shape(g["tree"], np.zeros(N, dtype=np.int64), g["times"])
        assert np.array_equal(ts.stats[i, :10], want_stats[:10]), (r, ts.stats[i], want_stats)
        assert all(ts.lengths[i][k] == want_lengths[k] for k in EXACT), r
        assert_lengths(ts.lengths[i], numpy_lengths(g["tree"], g["times"]), N, r)
        chain = ens.replicate_events(int(r))
        for ev, t in ((ts.root_event[i], ts.root_time[i]), (ts.last_tip_event[i], ts.last_tip_time[i])):
            assert -1 <= ev < chain.shape[1] and t == (chain[0][ev] if ev >= 0 else 0.0), (r, ev, t)
        assert ts.tips[i] == ens.engine.counters(int(r)).reserved[4], r
        healthy += 1
    return healthy


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70"])
@pytest.mark.parametrize("seed", ["none", "int", "array"])
def test_rows_equal_the_host_sweep_over_genealogies(name, seed):
    R = 6
    ens = _ensemble(name, R)
    s = {"none": None, "int": 4711, "array": np.arange(R, dtype=np.int64) * 7 + 3}[seed]
    log = [ens.replicate_events(r).copy() for r in range(R)]
    ts = ens.tree_shapes(seed=s)
    assert ts.stats.shape == (R, 12) and ts.stats.dtype == np.int64 and ts.lengths.shape == (R, 7) and ts.lengths.dtype == np.float64
    assert ts.passes >= 1 and len(ts.kernel_ms) == 2
    assert assert_rows_equal_genealogies(ens, ts, ens.genealogies(seed=s)) >= 1
    assert all(np.array_equal(log[r], ens.replicate_events(r)) for r in range(R))
    ok = ts.ok
    assert np.array_equal(ts.height()[ok], (ts.last_tip_time - ts.root_time)[ok]) and np.array_equal(ts.mean_depth()[ok], ts.sackin[ok] / ts.tips[ok])
    assert np.all(ts.depth_variance()[ok] >= -1e-9) and np.all(ts.external_share()[ok] <= 1.0)
    assert np.allclose(ts.mean_branch()[ok] * (2 * ts.tips[ok] - 2), ts.length[ok], rtol=1e-12)
    cn = ts.colless_normalized()
    assert np.all((cn[ok & (ts.tips > 2)] >= 0) & (cn[ok & (ts.tips > 2)] <= 1)) and np.isnan(cn[ok & (ts.tips == 2)]).all()
    ens.close()


def test_subsets_order_and_passes(monkeypatch):
    R = 130
    ens = _ensemble("g9_short", R, n_max=1500, seeds0=7000)
    full = ens.tree_shapes(seed=99)
    assert assert_rows_equal_genealogies(ens, full, ens.genealogies(seed=99)) > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tree_shapes(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_rows_equal_genealogies(ens, sub, ens.genealogies(seed=seeds, replicates=order))
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "200000")   # several device passes: same kernel, same tree, same order
    small = ens.tree_shapes(seed=99)
    assert small.passes > 1 and full.passes == 1
    for k in ("stats", "lengths", "status", "status_arg", "rng_raw", "replicates"):
        assert np.array_equal(getattr(small, k), getattr(full, k), equal_nan=k == "lengths"), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    for name, R, kw, seed, code, text in (("recomb_a", 8, dict(n_max=3000), 21, 4, "never coalesced"),
                                          ("extinct", 24, dict(n_max=50, seeds0=1), 5, 1, "Less than two")):
        ens = _ensemble(name, R, **kw)
        ts = ens.tree_shapes(seed=seed)
        assert (ts.status == code).any(), ts.status
        i = int(np.nonzero(ts.status == code)[0][0])
        assert text in ts.message(i)
        assert_rows_equal_genealogies(ens, ts, ens.genealogies(seed=seed))
        bad = ~ts.ok
        for f in (ts.height, ts.mean_depth, ts.depth_variance, ts.colless_normalized, ts.mean_branch, ts.external_share):
            assert np.isnan(f()[bad]).all(), f.__name__
        ens.close()


def test_refusals():
    ens = _ensemble("g9_short", 3, n_max=500)
    with pytest.raises(ValueError, match="out of range"):
        ens.tree_shapes(replicates=[0, 3])
    with pytest.raises(ValueError, match="distinct"):
        ens.tree_shapes(replicates=[1, 1])
    with pytest.raises(ValueError, match="one seed per selected replicate"):
        ens.tree_shapes(seed=[1, 2, 3], replicates=[0, 2])
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"tree_shapes\(\).*record_events"):
        ens.tree_shapes()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"tree_shapes\(\).*tau"):
        ens.tree_shapes()
    ens.close()
