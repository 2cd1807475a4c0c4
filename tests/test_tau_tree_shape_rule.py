"""The node-time rule of vgx_tau_tree_shape.h on the host (``_capi.tau_node_times``, what the node-time kernel behind
``Ensemble.tau_tree_shapes`` computes per node) against ``np.where`` written here, bit for bit; the index it refuses; and the trees
of the tau genealogy goldens, which hold branches of length 0 (coalescences inside one step), through the host sweep
``_capi.tree_shape`` that the rows of ``tau_tree_shapes()`` are compared with.  No GPU."""
import os

import numpy as np
import pytest

from test_tree_shape_rule import GOLDEN, assert_lengths, numpy_lengths
from vgsim_amd import _capi


def where_times(ev, pre, st):
    """0.0 below 0, the prefix table below n_pre, the step table behind it (indices clipped where the branch is not taken; NaN
    behind either table, which no index inside the chain selects)."""
    ev = np.asarray(ev, dtype=np.int64)
    pre, st = np.asarray(pre, dtype=np.float64), np.asarray(st, dtype=np.float64)
    n_pre = len(pre)
    from_pre = np.concatenate((pre, [np.nan]))[np.clip(ev, 0, n_pre)]
    from_st = np.concatenate((st, [np.nan]))[np.clip(ev - n_pre, 0, len(st))]
    return np.where(ev < 0, 0.0, np.where(ev < n_pre, from_pre, from_st))


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def tables(rng, n_pre, n_steps):
    """Times that do not decrease, a fifth of them equal to their neighbour, with all 52 mantissa bits in use."""
    t = np.cumsum(rng.exponential(1.0, n_pre + n_steps) * (rng.random(n_pre + n_steps) > 0.2)) + 1.0 / 3.0
    return t[:n_pre].copy(), t[n_pre:].copy()


@pytest.mark.parametrize("n_pre,n_steps", [(0, 1), (1, 1), (7, 5), (300, 1000), (0, 64), (50, 0), (1, 0)])
def test_host_hook_equals_numpy_bit_for_bit(n_pre, n_steps):
    rng = np.random.default_rng(1000 * n_pre + n_steps)
    pre, st = tables(rng, n_pre, n_steps)
    n = n_pre + n_steps
    by_hand = [-1, 0, n_pre - 1, n_pre, n - 1, -2, -2 ** 31]
    ev = np.concatenate((np.array([e for e in by_hand if e < n], dtype=np.int64), rng.integers(-1, n, 700)))
    got = _capi.tau_node_times(ev, pre, st)
    assert got.shape == ev.shape and same_bits(got, where_times(ev, pre, st))
    assert not got[ev < 0].any() and not np.signbit(got[ev < 0]).any()


def test_edges_by_hand():
    pre, st = np.array([0.5, 0.75, 2.0]), np.array([2.5, 2.5, 2.5, 9.0])   # equal step times
    ev = [-1, 0, 2, 3, 6, 5, 4, 1, -2]
    assert list(_capi.tau_node_times(ev, pre, st)) == [0.0, 0.5, 2.0, 2.5, 9.0, 2.5, 2.5, 0.75, 0.0]
    assert list(_capi.tau_node_times([-1, 0, 3], [], st)) == [0.0, 2.5, 9.0]          # n_pre = 0: a restarted replicate
    assert list(_capi.tau_node_times([-1, 0, 2], pre, [])) == [0.0, 0.5, 2.0]         # n_steps = 0
    assert list(_capi.tau_node_times([-1, -5], [], [])) == [0.0, 0.0]
    assert len(_capi.tau_node_times([], pre, st)) == 0


def test_an_index_beyond_the_chain_is_refused_with_the_node():
    pre, st = np.array([0.5, 0.75, 2.0]), np.array([2.5, 3.5])
    with pytest.raises(ValueError, match=r"node 2\b.*index 5\b"):
        _capi.tau_node_times([4, -1, 5, 6], pre, st)          # ev = n_pre + n_steps, and the first such node is named
    with pytest.raises(ValueError, match=r"node 0\b"):
        _capi.tau_node_times([3], pre, [])                    # n_steps = 0: ev = n_pre
    with pytest.raises(ValueError, match=r"node 1\b"):
        _capi.tau_node_times([-1, 0], [], [])
    with pytest.raises(ValueError, match=r"node 0\b"):
        _capi.tau_node_times([2 ** 31 - 1], pre, st)
    assert list(_capi.tau_node_times([-2, 4], pre, st)) == [0.0, 3.5]   # -2 is not refused


@pytest.mark.parametrize("name,zero_branches", [("genealogy_tau_a_seed18.npz", 7), ("genealogy_tau_b_seed19.npz", 0), ("genealogy_tau_c_seed20.npz", 1)])
def test_tau_goldens_through_the_host_sweep(name, zero_branches):
    """What the rows of tau_tree_shapes() are compared with: the host sweep takes branches of length 0 as any other branch."""
    z = np.load(os.path.join(GOLDEN, name))
    tree, times = z["tree"].astype(np.int64), z["times"].astype(np.float64)
    N = len(tree)
    b = times[:-1] - times[tree[:-1]]
    assert (b == 0).sum() == zero_branches and b.min() >= 0
    stats, lengths = _capi.tree_shape(tree, np.zeros(N, dtype=np.int64), times)
    ln = dict(zip(_capi.TREE_SHAPE_LENGTHS, lengths))
    assert np.isfinite(lengths).all() and ln["max_branch"] >= 0 and ln["max_branch"] == b.max()
    assert 0 <= ln["external_length"] <= ln["length"]
    assert_lengths(lengths, numpy_lengths(tree, times), N, name)
    assert stats[0] == (N + 1) // 2 and stats[1] == stats[0] - 1
