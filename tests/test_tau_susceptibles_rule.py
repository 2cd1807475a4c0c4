"""The susceptible rule of tau chains (vgsim_amd/csrc/vgx_tau_susceptible.h: the cells of vgx_susceptible.h changed by sign * num;
rows, bounds, `outside`, the prefix counted once and the 64-bit running sum are vgx_tau_prevalence.h's), compiled for the host and
reached through vgx_test_tau_susceptibles: the CPU oracle's tau chains with their final susceptible states, every split of a chain
into prefix and own steps, tile sizes, hand-made chains, against the literal restatement below (never against the code under
test), all with array_equal on integers.  No GPU."""
import numpy as np
import pytest

from test_susceptibles_rule import deltas, fold
from test_tau_incidence_rule import CHAINS, make, oracle_chain
from test_tau_prevalence_rule import rows_of_events

B, D, SA, MU, SC, MI, MULTI = range(7)
DIRECT = 0x100                                               # VGX_TL_ROW_DIRECT


def restate_weighted(events, mev, P, grid, class_of, G, start, rows=None):
    """The rule as Python loops: the events in order, `point` advanced with grid[point] < t (strictly), every row of an event
    applied num times through class_of (exact Python integers).  Returns (values [T, P, G] int64, final [P, G], outside [2])."""
    times = np.asarray(events[0], dtype=np.float64)
    rows = rows_of_events(events, mev) if rows is None else rows
    T, point = len(grid), 0
    state = [[int(v) for v in row] for row in np.asarray(start).reshape(P, G)]
    values = np.zeros((T, P, G), dtype=np.int64)
    outside = [0, 0]
    for i, t in enumerate(times):
        while point < T and grid[point] < t:
            values[point] = state
            point += 1
        for num, *rec in rows[i]:
            if num <= 0:
                continue
            if point == 0:
                outside[0] += num                            # a row before cut[0]
            if point == T:
                outside[1] += num                            # a row from cut[T - 1] on
            if rec[0] >= 0:
                rec[0] &= ~DIRECT                            # the direct flag of a flattened row
            rec = [v if 0 <= v < 2 ** 31 else -1 for v in rec]   # a field that is not a 32-bit index matches nothing
            for p, c, d in deltas(rec, P, class_of):
                state[p][c] += d * num
    values[point:] = state
    return values, np.array(state, dtype=np.int64), np.array(outside, dtype=np.int64)


def hook(events, mev, P, S, grid, class_of, G, start, tile=0, n_own=-1):
    from vgsim_amd import _capi
    return _capi.replay_tau_susceptibles(events, mev, P, S, grid, class_of, G, start, tile, n_own)


def assert_hook_equals(events, mev, P, S, grid, class_of, G, start, tile=0, n_own=-1, what="", want=None, rows=None):
    got = hook(events, mev, P, S, grid, class_of, G, start, tile, n_own)
    want = restate_weighted(events, mev, P, grid, class_of, G, start, rows) if want is None else want
    assert all(g.dtype == np.int64 for g in got) and got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what
    return got


def maps_of(S):
    """Identity, and (with two groups or more) the groups g % 2 with the last group not tracked, G as group_map forms it."""
    out = [(np.arange(S), S)]
    if S >= 2:
        partial = np.arange(S) % 2
        partial[S - 1] = -1
        out.append((partial, int(partial.max()) + 1))
    return out


# ---- the oracle's chains
@pytest.mark.parametrize("name", CHAINS)
def test_hook_equals_restatement_on_oracle_chains(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    types = ev[1]
    assert (types == MULTI).any() and (types != MULTI).any()
    P, S, tl = m.popNum, m.susNum, ev[0][-1]
    rows = rows_of_events(ev, mev)
    for k, (co, G) in enumerate(maps_of(S)):
        start = fold(m.initial_susceptible, co, G)
        for T in (100, 7, 1):
            grid = np.linspace(ev[0][len(types) // 10], 0.9 * tl, T)   # events lie before, between and behind the grid times
            values, final, outside = assert_hook_equals(ev, mev, P, S, grid, co, G, start, what=(name, k, T), rows=rows)
            assert outside.all() and (T == 1 or not np.array_equal(values[0], values[-1]))
            assert np.array_equal(final, fold(m.susceptible, co, G))   # with the identity map: the oracle's final susceptible state
            assert values.min() >= 0


def _mixed_slice(oracle_mod, n=160):
    m, ev, mev = oracle_chain(oracle_mod, "tau_then_direct")       # direct, tau steps, direct again: a mixed chain
    a = int(np.argmax(ev[1] == MULTI))
    lo = max(0, a - n // 2)
    ev = [c[lo:lo + n] for c in ev]
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any() and len(ev[0]) == n
    return m, ev, mev


def test_every_split_into_prefix_and_own_events_gives_the_whole_chain(oracle_mod):
    m, ev, mev = _mixed_slice(oracle_mod)
    n, P, S = len(ev[0]), m.popNum, m.susNum
    co = np.arange(S)
    start = np.full((P, S), 10 ** 7)                              # (a slice of a chain: far from zero)
    for T in (9, 1):
        grid = np.linspace(ev[0][n // 5], ev[0][4 * n // 5], T)
        want = restate_weighted(ev, mev, P, grid, co, S, start)
        assert want[2].all() and (T == 1 or not np.array_equal(want[0][0], want[0][-1]))
        for k in range(n + 1):
            assert_hook_equals(ev, mev, P, S, grid, co, S, start, tile=7, n_own=k, what=(T, k), want=want)


def test_tile_sizes_give_the_same_block(oracle_mod):
    m, ev, mev = oracle_chain(oracle_mod, "tau_b")
    n_direct = int(np.argmax(ev[1] == MULTI))
    keep = slice(max(0, n_direct - 40), n_direct + 2)        # (the oracle's multievent log is dense: hundreds of rows per step)
    ev = [c[keep] for c in ev]
    steps = ev[1] == MULTI
    rows = int((~steps).sum() + (ev[3][steps] - ev[2][steps]).sum())
    assert 100 < rows < 2000 and steps.sum() == 2
    P, S = m.popNum, m.susNum
    grid = np.linspace(ev[0][10], 0.5 * (ev[0][-2] + ev[0][-1]), 8)   # the last step lies behind the grid
    for co, G in maps_of(S):
        start = np.full((P, G), 10 ** 7)
        want = restate_weighted(ev, mev, P, grid, co, G, start)
        assert want[2].all() and len(np.unique(want[0])) > 5
        for tile in (1, 3, 64, 0, rows - 1, rows, rows + 1):
            for n_own in (-1, 0, 20):
                assert_hook_equals(ev, mev, P, S, grid, co, G, start, tile=tile, n_own=n_own, what=(G, tile, n_own), want=want)


# ---- hand-made chains: (time, type, haplotype, population, newHaplotype, newPopulation) events, MULTITYPE ones carrying their row
# range in (haplotype, population); rows (num, type, haplotype, population, newHaplotype, newPopulation)
def test_every_row_kind_and_rows_that_change_nothing():
    P, S, G = 3, 5, 3
    co = np.array([0, 0, 1, 2, -1])                               # groups 0 and 1 share class 0; 4 is not tracked
    start = np.full((P, G), 100)
    rows = [(2, B, 9, 0, 1, 9), (3, D, 9, 1, 2, 0), (4, SA, 9, 2, 3, 0),                      # step 0
            (5, SC, 0, 1, 1, 0),                                  # step 1: within class 0: nothing
            (6, SC, 0, 1, 2, 0),                                  # class 0 -> 1 in population 1
            (7, SC, 4, 2, 3, 0),                                  # out of the untracked group: +7 only
            (8, SC, 3, 2, 4, 0),                                  # into it: -8 only
            (9, SC, 4, 0, 4, 0),                                  # untracked on both sides
            (10, MI, 0, 0, 2, 2),                                 # keyed by newPopulation and newHaplotype: -10 at (2, class 1)
            (11, MI, 2, 0, 0, 3), (11, MI, 2, 0, 0, -1),          # newPopulation outside [0, P)
            (12, MU, 0, 0, 1, 0),
            (0, D, 0, 0, 0, 0), (-7, D, 0, 0, 0, 0),              # step 2: num = 0 and negative num: nothing, not in `outside` either
            (2, D, 0, 3, 0, 0), (2, D, 0, -1, 0, 0), (2, 6, 0, 0, 0, 0), (2, -1, 0, 0, 0, 0), (2, 7, 0, 0, 0, 0),   # keys / types out of range
            (2, D, 0, 0, 5, 0), (2, SC, 5, 0, 2, 0),              # group outside [0, S): that side changes nothing
            (2, D, 0, 2 ** 32, 0, 0), (2, D, 0, 0, 2 ** 32 + 1, 0), (2, MI, 0, 1, 0, 2 ** 40 + 1),   # a field beyond 32 bits matches nothing
            (2, SC, 2 ** 32 + 2, 0, 2, 0),                        # ... on one side of a SUSCCHANGE: the other side changes
            (13, D | DIRECT, 0, 2, 2, 0)]                         # the direct flag of a flattened row is masked off
    events = [(0.25, D, 0, 0, 0, 0), (1.0, MULTI, 0, 3, 0, 0), (2.0, MULTI, 3, 12, 0, 0), (3.0, MULTI, 12, 26, 0, 0)]
    ev, mev = make(events, rows)
    grid = np.array([0.5, 1.5, 2.5, 3.5])
    values, final, outside = assert_hook_equals(ev, mev, P, S, grid, co, G, start, tile=4)
    want = start.copy(); want[0, 0] += 1
    assert np.array_equal(values[0], want)
    want[0, 0] -= 2; want[1, 1] += 3; want[2, 2] += 4
    assert np.array_equal(values[1], want)
    want[1, 0] -= 6; want[1, 1] += 6; want[2, 2] += 7; want[2, 2] -= 8; want[2, 1] -= 10
    assert np.array_equal(values[2], want)
    want[0, 1] += 2 + 2; want[2, 1] += 13
    assert np.array_equal(values[3], want) and np.array_equal(final, want)
    assert outside.tolist() == [1, 0]
    # one grid point in front of the last step: its rows with positive num lie behind the grid, whether they change a cell or not
    _, _, outside = assert_hook_equals(ev, mev, P, S, np.array([2.5]), co, G, start, tile=5)
    assert outside.tolist() == [1 + (2 + 3 + 4) + (5 + 6 + 7 + 8 + 9 + 10 + 11 + 11 + 12), 2 * 11 + 13]
    # the rows the flattening accepts give the same as prefix rows
    ev3 = [c[:3] for c in ev]
    for n_own in (-1, 0, 1):
        assert_hook_equals(ev3, mev, P, S, grid, co, G, start, tile=2, n_own=n_own, what=n_own)


def test_a_step_on_a_grid_time_is_applied_and_an_empty_chain():
    P, S = 2, 2
    rows = [(3, B, 0, 0, 0, 0), (2, MI, 0, 0, 1, 1), (5, D, 0, 1, 1, 0), (4, SC, 0, 0, 1, 0)]
    events = [(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 2, 0, 0), (2.0, MULTI, 2, 2, 0, 0), (1.5, MULTI, 2, 3, 0, 0), (3.0, MULTI, 3, 4, 0, 0)]
    ev, mev = make(events, rows)
    grid = np.array([1.0, 2.0, 3.0])
    start = np.full((P, S), 10)
    v0 = start.copy(); v0[0, 0] -= 1 + 3; v0[1, 1] -= 2
    v1 = v0.copy(); v1[1, 1] += 5
    v2 = v1.copy(); v2[0, 0] -= 4; v2[0, 1] += 4
    for n_own in (-1, 0, 2, 3, 5):
        values, final, outside = assert_hook_equals(ev, mev, P, S, grid, np.arange(S), S, start, n_own=n_own, what=n_own)
        assert np.array_equal(values, [v0, v1, v2]) and np.array_equal(final, v2) and outside.tolist() == [6, 0]
    values, final, outside = assert_hook_equals([np.zeros(0)] + [np.zeros(0, dtype=np.int64)] * 5, None, P, S, np.array([0.0, 1.0]), np.arange(S), S, start)
    assert np.array_equal(values, [start, start]) and np.array_equal(final, start) and outside.tolist() == [0, 0]


def test_net_changes_and_values_beyond_32_bits_are_exact():
    P, S = 2, 3
    big = 2 ** 31 + 5
    rows = [(big, D, 0, 1, 1, 0), (big, D, 0, 1, 1, 0), (big, D, 0, 1, 1, 0), (7, B, 0, 1, 1, 0),
            (2 * big, B, 0, 1, 1, 0), (big, SC, 1, 1, 2, 0), (3, D, 0, 0, 0, 0)]
    events = [(1.0, MULTI, 0, 4, 0, 0), (2.0, MULTI, 4, 6, 0, 0), (3.0, MULTI, 6, 7, 0, 0)]
    ev, mev = make(events, rows)
    start = np.array([[0, 0, 0], [0, 11, 0]])
    for n_own in (-1, 0, 1):
        for tile in (0, 1, 2):
            values, final, outside = assert_hook_equals(ev, mev, P, S, np.array([1.5, 2.5]), np.arange(S), S, start, tile=tile, n_own=n_own)
            assert 3 * big - 7 > 2 ** 32 and values[0, 1, 1] == 11 + 3 * big - 7          # a net change and a value beyond 2^32
            assert values[1, 1, 1] == 11 - 7 and values[1, 1, 2] == big and final[0, 0] == 3
            assert outside.tolist() == [3 * big + 7, 3]


# ---- refusals
def test_the_hooks_refusals():
    ev, mev = make([(0.5, D, 0, 0, 0, 0), (1.0, MULTI, 0, 1, 0, 0)], [(1, D, 0, 0, 0, 0)])
    ok, co, start = np.array([0.0, 2.0]), np.arange(2), np.zeros((2, 2))
    for grid, text in (([0.0, 1.0, 1.0], "increase strictly"), ([1.0, 0.5], "increase strictly"), ([0.0, float("nan")], "not finite"),
                       ([float("inf")], "not finite"), ([], "T = 0")):
        with pytest.raises(ValueError, match="vgx_test_tau_susceptibles: .*" + text):
            hook(ev, mev, 2, 2, np.array(grid), co, 2, start)
    one = make([(0.5, D, 0, 0, 0, 0)], [])
    values, final, _ = hook(*one, 1, 1, np.array([1.0]), np.array([8191]), 8192, np.zeros((1, 8192)))   # 8 * 8192 = 65536 bytes fit
    assert values[0, 0, 8191] == 1 and values.sum() == 1 and final.sum() == 1
    with pytest.raises(ValueError, match="1 populations x 8193 classes need 65544 bytes"):
        hook(*one, 1, 1, np.array([1.0]), np.array([0]), 8193, np.zeros((1, 8193)))
    with pytest.raises(ValueError, match=r"class_of\[1\] = 2 is outside \[-1, 2\)"):
        hook(ev, mev, 2, 2, ok, np.array([0, 2]), 2, start)
    with pytest.raises(ValueError, match=r"class_of\[0\] = -2 is outside"):
        hook(ev, mev, 2, 2, ok, np.array([-2, 0]), 2, start)
    with pytest.raises(ValueError, match="G = 0"):
        hook(ev, mev, 2, 2, ok, np.array([-1, -1]), 0, np.zeros((2, 0)))
    for n_own in (-1, 0):                                            # as an own step and as part of the prefix
        for bad in ((1.0, MULTI, 0, 2, 0, 0), (1.0, MULTI, -1, 1, 0, 0)):
            ev2, _ = make([(0.5, D, 0, 0, 0, 0), bad], [])
            with pytest.raises(ValueError, match="MULTITYPE row range outside the multievent log"):
                hook(ev2, mev, 2, 2, ok, co, 2, start, n_own=n_own)
    with pytest.raises(ValueError, match="n_own_events"):
        hook(ev, mev, 2, 2, ok, co, 2, start, n_own=3)
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook(ev, mev, 2, 2, ok, co, 2, start, tile=-1)
    neg = make([(1.0, MULTI, 0, 1, 0, 0)], [(-1, D, 0, 0, 0, 0)])
    with pytest.raises(ValueError, match="value out of range"):      # the prefix passes the checks of the flattening
        hook(*neg, 2, 2, ok, co, 2, start, n_own=0)


def test_share_of_an_int64_block():
    from vgsim_amd.ensemble import Susceptibles
    sv = Susceptibles()
    sv.values = np.array([[[[2 ** 33, 3 * 2 ** 33], [0, 0]]]], dtype=np.int64)
    assert sv.share().tolist() == [[[[0.25, 0.75], [0.0, 0.0]]]] and sv.share().dtype == np.float64
