"""Ensemble.tau_tree_shapes(): the node-time kernel (vgx_tau_tree_shapes.hip) alone through ``_capi.tau_node_times_device`` against
the host hook, bit for bit; and the rows of tau ensembles against the host sweep ``_capi.tree_shape`` applied to the trees
``tau_genealogies()`` returns for the same walks: integers and the exact lengths bit for bit, the four length sums within
2 (N + 2) 2^-53 of numpy's sum (the bound derived in test_tree_shape_rule.py); status, generator words and messages of
``tau_genealogies()``; both tau paths, the three seed forms, chains with and without a prefix, restarted replicates, subsets,
order, several passes, failed walks, refusals and what the call must leave alone."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_tau_genealogies import PATHS, SEEDS, _fresh, _near_critical_warm, seed_forms, warm
from test_hip_tau_lineages import _few_samples_ensemble
from test_tree_shape_rule import EXACT, assert_lengths, numpy_lengths
from vgsim_amd import _capi

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
FIELDS = ("stats", "lengths", "status", "status_arg", "rng_raw", "replicates")
ZERO_BRANCH_CASE = "tau_a"   # its trees hold coalescences inside one step: branches of length 0 (7 in genealogy_tau_a_seed18.npz)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the node-time kernel alone ----------------------------------------------------------------------------------------------------
def test_node_time_kernel_equals_the_host_hook():
    rng = np.random.default_rng(30)
    t = np.cumsum(rng.exponential(1.0, 90)) + 1.0 / 3.0
    pre = t[:90].copy()
    sizes = [3, 255, 256, 257, 1025] + [int(s) for s in rng.integers(1, 402, 125)]
    assert len(sizes) == 130
    trees = []
    for k, N in enumerate(sizes):
        n_pre = 0 if k % 3 == 1 else len(pre)          # restarted replicates beside ones that share the prefix table
        n_steps = 0 if k == 6 else int(rng.integers(1, 300))
        st = pre[-1] + np.cumsum(rng.exponential(1.0, n_steps) * (rng.random(n_steps) > 0.2))   # (equal step times among them)
        ev = rng.integers(-1, n_pre + n_steps, N)
        ev[0], ev[-1] = n_pre + n_steps - 1, -1        # the chain's last event, and a node no event made
        trees.append((ev, n_pre, st))
    assert trees[6][1] == len(pre) and len(trees[6][2]) == 0 and trees[1][1] == 0 and trees[0][1] == len(pre)
    # tree 3 (257 nodes): a single index beyond its chain in the middle; tree 4 (1025 nodes): four of them, in several wavefronts
    # and rounds of the stride loop, of which the lowest node is reported
    beyond = {3: [128], 4: [900, 333, 70, 1000]}
    for k, nodes in beyond.items():
        chain = trees[k][1] + len(trees[k][2])
        trees[k][0][nodes] = [chain, chain + 1, INT32_MAX, chain][:len(nodes)]
    times, bad = _capi.tau_node_times_device(trees, pre)
    assert bad.dtype == np.int32 and bad[3] == 128 and bad[4] == 70 and (np.delete(bad, [3, 4]) == INT32_MAX).all(), bad
    for k, (ev, n_pre, st) in enumerate(trees):
        good = ev.copy()
        for node in beyond.get(k, ()):
            assert times[k][node] == 0.0 and not np.signbit(times[k][node])
            good[node] = -1
        assert same_bits(times[k], _capi.tau_node_times(good, pre[:n_pre], st)), k
    # offsets and prefix lengths the kernel could not bound are refused before anything is uploaded
    with pytest.raises(ValueError, match="n_pre = 91"):
        _capi.tau_node_times_device([(np.array([0]), 91, np.array([1.0]))], pre)
    empty_times, empty_bad = _capi.tau_node_times_device([], pre)
    assert empty_times == [] and len(empty_bad) == 0


# ---- rows of ensembles -----------------------------------------------------------------------------------------------------------
def assert_rows_equal_genealogies(ens, ts, batch):
    """Every row against the host sweep over the tree tau_genealogies() returns for the same walk.  Returns (healthy rows, branches
    of length 0 in trees with max_branch > 0)."""
    healthy = zero = 0
    assert np.array_equal(ts.status, batch.status) and np.array_equal(ts.status_arg, batch.status_arg)
    assert ts.rng_raw.shape == (len(ts.replicates), 6) and np.array_equal(ts.rng_raw, batch.rng_raw)
    assert np.array_equal(ts.replicates, batch.replicates)
    n_model = int(ens.model.events.ptr)
    for i, r in enumerate(ts.replicates):
        assert ts.message(i) == batch.message(i)
        if not ts.ok[i]:
            assert not ts.stats[i].any() and np.isnan(ts.lengths[i]).all(), r
            continue
        g = batch.replicate(int(r))
        N = len(g["tree"])
        want_stats, want_lengths = _capi.tree_shape(g["tree"], np.zeros(N, dtype=np.int64), g["times"])
        assert np.array_equal(ts.stats[i, :10], want_stats[:10]), (r, ts.stats[i], want_stats)
        assert all(same_bits(ts.lengths[i][k:k + 1], want_lengths[k:k + 1]) for k in EXACT), (r, ts.lengths[i], want_lengths)
        assert_lengths(ts.lengths[i], numpy_lengths(g["tree"], g["times"]), N, r)
        c = ens.engine.counters(int(r))
        assert ts.tips[i] == c.reserved[4], r
        chain = ens.replicate_events(int(r))
        n_pre = 0 if c.restarts > 0 else n_model
        assert c.ev_first_new == n_pre
        for ev, t in ((ts.root_event[i], ts.root_time[i]), (ts.last_tip_event[i], ts.last_tip_time[i])):
            assert -1 <= ev < chain.shape[1], (r, ev, chain.shape)
            if ev < 0:
                assert t == 0.0
            elif ev >= n_pre:   # one of the replicate's own steps: the time of its MULTITYPE record
                assert t == chain[0][ev], (r, ev, t)
        b = g["times"][:-1] - g["times"][g["tree"][:-1]]
        if ts.max_branch[i] > 0:
            zero += int((b == 0).sum())
        healthy += 1
    return healthy, zero


def assert_derived_values(ts):
    ok = ts.ok
    assert np.array_equal(ts.height()[ok], (ts.last_tip_time - ts.root_time)[ok]) and np.array_equal(ts.mean_depth()[ok], ts.sackin[ok] / ts.tips[ok])
    for f in (ts.height, ts.mean_depth, ts.depth_variance, ts.colless_normalized, ts.mean_branch, ts.external_share):
        assert np.isnan(f()[~ok]).all(), f.__name__


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_rows_equal_the_host_sweep_over_tau_genealogies(name, path, monkeypatch):
    """A tau call that continues a direct warm-up (the prefix), on both tau paths, for the three seed forms."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    R = 6
    ens = Ensemble(sim, R, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.model.events.ptr > 0 and all(ens.engine.counters(r).restarts == 0 for r in range(R))
    zeros = 0
    for s in seed_forms(R):
        ts = ens.tau_tree_shapes(seed=s)
        assert ts.stats.shape == (R, 12) and ts.stats.dtype == np.int64 and ts.lengths.shape == (R, 7) and ts.lengths.dtype == np.float64
        assert list(ts.replicates) == list(range(R)) and ts.passes >= 1 and len(ts.kernel_ms) == 2 and len(ts.stage_ms) == 4
        healthy, zero = assert_rows_equal_genealogies(ens, ts, ens.tau_genealogies(seed=s))
        assert healthy >= 1, name
        zeros += zero
        assert_derived_values(ts)
    print("%s %s: %d branches of length 0" % (name, path, zeros))
    if name == ZERO_BRANCH_CASE:
        assert zeros > 0
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix_and_restarted_replicates(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log; and replicates that restarted (no prefix for them) beside ones
    that did not, in one launch."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    for s in (None, 99):
        assert_rows_equal_genealogies(ens, ens.tau_tree_shapes(seed=s), ens.tau_genealogies(seed=s))
    ens.close()
    ens = Ensemble(_near_critical_warm(), 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    for s in (None, 99):
        ts = ens.tau_tree_shapes(seed=s)
        assert ts.passes == 1
        assert_rows_equal_genealogies(ens, ts, ens.tau_genealogies(seed=s))
    ens.close()


def test_subsets_order_and_passes(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    R = 130
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    full = ens.tau_tree_shapes(seed=99)
    assert full.passes == 1
    assert assert_rows_equal_genealogies(ens, full, ens.tau_genealogies(seed=99))[0] > 100
    order = np.random.default_rng(3).permutation(R)[:40]
    seeds = 1000 + np.arange(40, dtype=np.int64)
    sub = ens.tau_tree_shapes(seed=seeds, replicates=order)
    assert list(sub.replicates) == list(order)
    assert assert_rows_equal_genealogies(ens, sub, ens.tau_genealogies(seed=seeds, replicates=order))[0] > 30
    same = ens.tau_tree_shapes(seed=99, replicates=order)
    for k in FIELDS[:-1]:
        assert np.array_equal(getattr(same, k), getattr(full, k)[order], equal_nan=k == "lengths"), k
    monkeypatch.setenv("VGX_GENEALOGY_CHUNK_BYTES", "4000000")   # several device passes: same kernels, same trees, same order
    small = ens.tau_tree_shapes(seed=99)
    assert small.passes > 1
    for k in FIELDS:
        assert np.array_equal(getattr(small, k), getattr(full, k), equal_nan=k == "lengths"), k
    ens.close()


def test_failed_walks_do_not_fail_the_call():
    ens = _few_samples_ensemble()
    ts = ens.tau_tree_shapes(seed=5)
    batch = ens.tau_genealogies(seed=5)
    assert (ts.status == 1).any() and ts.ok.any() and np.array_equal(ts.status, batch.status), ts.status
    assert "Less than two" in ts.message(int(np.nonzero(ts.status == 1)[0][0]))
    assert_rows_equal_genealogies(ens, ts, batch)
    bad = ~ts.ok
    assert not ts.stats[bad].any() and np.isnan(ts.lengths[bad]).all()
    assert_derived_values(ts)
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match=r"tau_tree_shapes\(\).*simulate_tau"):
        ens.tau_tree_shapes()
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match=r"tau_tree_shapes\(\).*tau chains only"):
        ens.tau_tree_shapes()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match=r"tau_tree_shapes\(\).*record_events"):
        ens.tau_tree_shapes()
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    for kw, msg in ((dict(replicates=[0, 2]), "out of range"), (dict(replicates=[-1]), "out of range"), (dict(replicates=[1, 1]), "distinct"),
                    (dict(seed=[1, 2, 3]), "one seed per selected replicate")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_tree_shapes(**kw)
    with pytest.raises(ValueError, match=r"tree_shapes\(\) walks direct chains only: the last call was simulate_tau"):
        ens.tree_shapes()   # the direct call still refuses tau chains with its own text
    one = ens.tau_tree_shapes(seed=1, replicates=[1])
    assert one.stats.shape == (1, 12) and list(one.replicates) == [1]
    none = ens.tau_tree_shapes(replicates=[])
    assert none.stats.shape == (0, 12) and none.lengths.shape == (0, 7) and none.passes == 0
    ens.close()


def test_the_call_leaves_rows_and_read_outs_alone():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    rows = [ens.engine.multievents(r) for r in range(ens.R)]
    chains = [ens.replicate_events(r).copy() for r in range(ens.R)]
    before = ens.tau_genealogies(seed=5)
    first = ens.tau_tree_shapes(seed=5)
    for r in range(ens.R):
        again = ens.engine.multievents(r)
        assert all(np.array_equal(rows[r][k], again[k]) for k in rows[r]), r
        assert np.array_equal(chains[r], ens.replicate_events(r)), r
    after = ens.tau_genealogies(seed=5)
    for k in ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
              "mig_offsets", "mig_node", "mig_old", "mig_new", "mig_time", "nodes_used", "rng_raw"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    second = ens.tau_tree_shapes(seed=5)
    for k in FIELDS:
        assert np.array_equal(getattr(first, k), getattr(second, k), equal_nan=k == "lengths"), k
    ens.close()
