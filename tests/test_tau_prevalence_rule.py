"""The prevalence rule of tau chains (vgsim_amd/csrc/vgx_tau_prevalence.h: weighted rows, signed int64 cells, bounds in row index
space, `outside` as sums of num, the prefix's net block counted once and every chain's started from it, the 64-bit running sum),
compiled for the host and reached through vgx_test_tau_prevalence: the CPU oracle's tau chains, every split of a chain into prefix
and own steps, tile sizes, hand-made chains, against the literal restatement below (never against the code under test), all with
array_equal on integers; and the argument checks of Ensemble.tau_prevalence, which are raised before the library is called.  No GPU.

The hook flattens the PREFIX with the checks of the tau timelines' flattening (a negative num or a field outside 32 bits is
refused there) and takes a replicate's OWN rows as they are, as the device reads them: the hand-made chains put such rows into
the own steps."""
import numpy as np
import pytest

from test_incidence_rule import bare_ensemble
from test_prevalence_rule import deltas, fold
from test_tau_incidence_rule import CHAINS, MEV_COLUMNS, make, oracle_chain

B, D, SA, MU, SC, MI, MULTI = range(7)
DIRECT = 0x100                                               # VGX_TL_ROW_DIRECT


def rows_of_events(events, mev):
    """Every event's rows (num, type, haplotype, population, newHaplotype, newPopulation): one row with num 1 for a direct event,
    the multievent rows of a step."""
    cols = [np.asarray(c, dtype=np.int64) for c in events[1:6]]
    out = []
    for i in range(len(events[0])):
        t = int(cols[0][i])
        if t == MULTI:
            out.append([tuple(int(mev[c][j]) for c in MEV_COLUMNS) for j in range(int(cols[1][i]), int(cols[2][i]))])
        else:
            out.append([(1, t) + tuple(int(c[i]) for c in cols[1:])])
    return out


def restate_weighted_prevalence(events, mev, P, grid, variant_of, V, start, rows=None):
    """The rule as Python loops: the events in order, `point` advanced with grid[point] < t (strictly), every row of an event
    applied num times through variant_of (num changes of one host each are one change of num hosts: the sums are exact Python
    integers).  Returns (values [T, P, V] int64, final [P, V], outside [2])."""
    times = np.asarray(events[0], dtype=np.float64)
    rows = rows_of_events(events, mev) if rows is None else rows
    T, point = len(grid), 0
    state = [[int(v) for v in row] for row in np.asarray(start).reshape(P, V)]
    values = np.zeros((T, P, V), dtype=np.int64)
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
            for p, c, d in deltas(rec, P, variant_of):
                state[p][c] += d * num
    values[point:] = state
    return values, np.array(state, dtype=np.int64), np.array(outside, dtype=np.int64)


def hook(events, mev, P, H, grid, variant_of, V, start, tile=0, n_own=-1):
    from vgsim_amd import _capi
    return _capi.replay_tau_prevalence(events, mev, P, H, grid, variant_of, V, start, tile, n_own)


def assert_hook_equals(events, mev, P, H, grid, variant_of, V, start, tile=0, n_own=-1, what="", want=None, rows=None):
    got = hook(events, mev, P, H, grid, variant_of, V, start, tile, n_own)
    want = restate_weighted_prevalence(events, mev, P, grid, variant_of, V, start, rows) if want is None else want
    assert all(g.dtype == np.int64 for g in got) and got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what
    return got


def three_maps(H, rows):
    """Identity, h % 3, and h % 3 with the second busiest haplotype of the chain (the only one of a model with one) not tracked."""
    seen = np.array([r[2] for ev in rows for r in ev if 0 <= r[2] < H], dtype=np.int64)
    busy = np.bincount(seen, minlength=H).argsort()[::-1]
    partial = np.arange(H) % 3
    partial[busy[min(1, H - 1)]] = -1
    return ((np.arange(H), H), (np.arange(H) % 3, 3), (partial, 3))


# ---- the oracle's chains
@pytest.mark.parametrize("name", CHAINS)
def test_hook_equals_restatement_on_oracle_chains(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    types = ev[1]
    assert (types == MULTI).any() and (types != MULTI).any()
    P, H, tl = m.popNum, m.hapNum, ev[0][-1]
    rows = rows_of_events(ev, mev)
    for k, (vo, V) in enumerate(three_maps(H, rows)):
        start = fold(m.initial_infectious, vo, V)
        for T in (100, 7, 1):
            grid = np.linspace(ev[0][len(types) // 10], 0.9 * tl, T)   # events lie before, between and behind the grid times
            values, final, outside = assert_hook_equals(ev, mev, P, H, grid, vo, V, start, what=(name, k, T), rows=rows)
            assert outside.all() and (T == 1 or (vo < 0).all() or not np.array_equal(values[0], values[-1]))
            assert np.array_equal(final, fold(m.infectious, vo, V))   # with the identity map: the oracle's final infectious state
            assert k == 2 or values.min() >= 0


def _mixed_slice(oracle_mod, n=160):
    m, ev, mev = oracle_chain(oracle_mod, "tau_then_direct")       # direct, tau steps, direct again: a mixed chain
    a = int(np.argmax(ev[1] == MULTI))
    lo = max(0, a - n // 2)
    ev = [c[lo:lo + n] for c in ev]
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any() and len(ev[0]) == n
    return m, ev, mev


def test_every_split_into_prefix_and_own_events_gives_the_whole_chain(oracle_mod):
    """The check on prefix-once for a running sum: wherever the chain is split, the prefix's net block plus the own rows' net block,
    summed up once, is the block of the literal loop over the whole chain."""
    m, ev, mev = _mixed_slice(oracle_mod)
    n, P, H = len(ev[0]), m.popNum, m.hapNum
    vo = np.arange(H) % 3
    start = np.full((P, 3), 10 ** 7)                              # (a slice of a chain: far from zero)
    for T in (9, 1):
        grid = np.linspace(ev[0][n // 5], ev[0][4 * n // 5], T)
        want = restate_weighted_prevalence(ev, mev, P, grid, vo, 3, start)
        assert want[2].all() and (T == 1 or not np.array_equal(want[0][0], want[0][-1]))
        for k in range(n + 1):
            assert_hook_equals(ev, mev, P, H, grid, vo, 3, start, tile=7, n_own=k, what=(T, k), want=want)


def test_tile_sizes_give_the_same_block(oracle_mod):
    m, ev, mev = oracle_chain(oracle_mod, "tau_b")
    n_direct = int(np.argmax(ev[1] == MULTI))
    keep = slice(max(0, n_direct - 40), n_direct + 2)        # (the oracle's multievent log is dense: hundreds of rows per step)
    ev = [c[keep] for c in ev]
    steps = ev[1] == MULTI
    rows = int((~steps).sum() + (ev[3][steps] - ev[2][steps]).sum())
    assert 100 < rows < 2000 and steps.sum() == 2
    P, H = m.popNum, m.hapNum
    grid = np.linspace(ev[0][10], 0.5 * (ev[0][-2] + ev[0][-1]), 8)   # the last step lies behind the grid
    for vo, V in ((np.arange(H), H), (np.arange(H) % 3, 3)):
        start = np.full((P, V), 10 ** 7)
        want = restate_weighted_prevalence(ev, mev, P, grid, vo, V, start)
        assert want[2].all() and len(np.unique(want[0])) > 5
        for tile in (1, 3, 64, 0, rows - 1, rows, rows + 1):
            for n_own in (-1, 0, 20):
                assert_hook_equals(ev, mev, P, H, grid, vo, V, start, tile=tile, n_own=n_own, what=(V, tile, n_own), want=want)


def test_the_restatement_gives_the_trajectories_totals(oracle_mod):
    """What tests/test_hip_tau_prevalence.py relies on when it compares values.sum(-1) with trajectories(): on the oracle's tau
    chains, for a window that starts behind the prefix's last time, the restatement with every haplotype tracked sums to the
    replay the tau trajectories are defined by (test_hip_tau_trajectories.replay: the call's start totals, then per step the
    births and arriving migrations minus the deaths and samplings, a grid point written before the step that takes the time
    past it), at every grid point."""
    for name in ("tau_a", "tau_b", "tau_c", "tau_d"):
        m, ev, mev = oracle_chain(oracle_mod, name)
        P, H = m.popNum, m.hapNum
        n_pre = int(np.argmax(ev[1] == MULTI))
        assert n_pre > 0 and (ev[1][n_pre:] == MULTI).all()
        rows = rows_of_events(ev, mev)
        whole = restate_weighted_prevalence(ev, mev, P, np.array([ev[0].max() + 1.0]), np.arange(H), H, m.initial_infectious, rows)[0][0]
        at_call = restate_weighted_prevalence([c[:n_pre] for c in ev], mev, P, np.array([ev[0].max() + 1.0]), np.arange(H), H,
                                              m.initial_infectious, rows[:n_pre])[0][0].sum(axis=1)   # the totals the tau call starts from
        assert np.array_equal(whole, m.infectious)
        t_pre, t_end = float(ev[0][n_pre - 1]), float(ev[0][-1])
        for T, window in ((33, (t_pre + 0.1 * (t_end - t_pre), t_pre + 0.9 * (t_end - t_pre))), (7, (np.nextafter(t_pre, np.inf), t_end + 1.0)), (1, (0.5 * (t_pre + t_end),) * 2)):
            grid = window[0] + np.arange(T) * ((window[1] - window[0]) / (T - 1) if T > 1 else 0.0)
            assert grid[0] > t_pre
            values = restate_weighted_prevalence(ev, mev, P, grid, np.arange(H), H, m.initial_infectious, rows)[0]
            inf, want, j = at_call.copy(), np.zeros((T, P), dtype=np.int64), 0
            for i in range(n_pre, len(ev[0])):
                while j < T and grid[j] < ev[0][i]:
                    want[j] = inf
                    j += 1
                for num, t, _, pop, _, npop in rows[i]:
                    if t == B or t == MI:
                        inf[npop if t == MI else pop] += num
                    elif t in (D, SA):
                        inf[pop] -= num
            want[j:] = inf
            assert np.array_equal(values.sum(axis=-1), want), (name, T)
            assert np.all(np.diff(grid) > 0) and (T == 1 or not np.array_equal(want[0], want[-1]))


# ---- hand-made chains: (time, type, haplotype, population, newHaplotype, newPopulation) events, MULTITYPE ones carrying their row
# range in (haplotype, population); rows (num, type, haplotype, population, newHaplotype, newPopulation)
def test_a_step_without_rows_on_a_grid_time_and_times_that_go_back():
    P, H = 2, 4
    rows = [(3, B, 1, 0, 0, 0), (2, MI, 1, 0, 0, 1), (5, D, 2, 1, 0, 0), (4, SA, 0, 0, 0, 0)]
    events = [(0.5, B, 0, 0, 0, 0),
              (1.0, MULTI, 0, 2, 0, 0),                              # exactly on grid[0]: applied before point 0
              (2.0, MULTI, 2, 2, 0, 0),                              # no rows, takes the time past grid[0]: cut[0] is the first row after it
              (1.5, MULTI, 2, 3, 0, 0),                              # time goes back: `point` does not
              (3.0, MULTI, 3, 4, 0, 0)]                              # exactly on grid[2]: applied before point 2
    ev, mev = make(events, rows)
    grid = np.array([1.0, 2.0, 3.0])
    start = np.full((P, H), 10)
    v0 = start.copy(); v0[0, 0] += 1; v0[0, 1] += 3; v0[1, 1] += 2
    v1 = v0.copy(); v1[1, 2] -= 5
    v2 = v1.copy(); v2[0, 0] -= 4
    for n_own in (-1, 0, 2, 3, 5):
        values, final, outside = assert_hook_equals(ev, mev, P, H, grid, np.arange(H), H, start, n_own=n_own, what=n_own)
        assert np.array_equal(values, [v0, v1, v2]) and np.array_equal(final, v2) and outside.tolist() == [6, 0]
    # the same chain with the second grid time just below the empty step's time: that step now takes the time past it
    values, _, outside = assert_hook_equals(ev, mev, P, H, np.array([1.0, np.nextafter(2.0, 0.0), 2.5]), np.arange(H), H, start)
    assert np.array_equal(values, [v0, v0, v1]) and outside.tolist() == [6, 4]


def test_grids_before_behind_and_inside_the_chain():
    P, H = 2, 2
    rows = [(k + 1, B, 0, k % 2, 0, 0) for k in range(12)]
    events = [(float(k), B, 1, 1, 0, 0) for k in range(3)] + [(3.0 + k, MULTI, 2 * k, 2 * k + 2, 0, 0) for k in range(6)]
    ev, mev = make(events, rows)
    total = 3 + sum(range(1, 13))
    vo, start = np.arange(H), np.array([[5, 0], [0, 7]])
    end = start + [[sum(range(1, 13, 2)), 0], [sum(range(2, 13, 2)), 3]]
    for n_own in (-1, 0, 4, 9):
        values, final, outside = assert_hook_equals(ev, mev, P, H, np.array([-5.0, -1.0]), vo, H, start, n_own=n_own)      # before the chain
        assert np.array_equal(values, [start, start]) and np.array_equal(final, end) and outside.tolist() == [0, total]
        values, final, outside = assert_hook_equals(ev, mev, P, H, np.array([100.0, 101.0, 102.0]), vo, H, start, n_own=n_own)   # behind it
        assert np.array_equal(values, [end, end, end]) and np.array_equal(final, end) and outside.tolist() == [total, 0]
        values, final, outside = assert_hook_equals(ev, mev, P, H, np.array([1.0, 4.5, 6.0]), vo, H, start, n_own=n_own, tile=3)   # the cuts fall on both sides of the split
        assert np.array_equal(final, end) and outside.tolist() == [2, sum(range(9, 13))]
    values, final, outside = assert_hook_equals([np.zeros(0)] + [np.zeros(0, dtype=np.int64)] * 5, None, P, H, np.array([0.0, 1.0]), vo, H, start)   # an empty chain
    assert np.array_equal(values, [start, start]) and np.array_equal(final, start) and outside.tolist() == [0, 0]


def test_every_row_kind_and_rows_that_change_nothing():
    P, H, V = 3, 5, 3
    vo = np.array([0, 0, 1, 2, -1])                               # haplotypes 0 and 1 share class 0; 4 is not tracked
    start = np.full((P, V), 100)
    rows = [(2, B, 1, 0, 9, 9), (3, D, 2, 1, 0, 0), (4, SA, 3, 2, 0, 0),                      # step 0
            (5, MU, 0, 1, 1, 0),                                  # step 1: within class 0: nothing
            (6, MU, 0, 1, 2, 0),                                  # class 0 -> 1 in population 1
            (7, MU, 4, 2, 3, 0),                                  # out of the untracked haplotype: +7 only
            (8, MU, 3, 2, 4, 0),                                  # into it: -8 only
            (9, MU, 4, 0, 4, 0),                                  # untracked on both sides
            (10, MI, 2, 0, 7, 2),                                 # keyed by newPopulation: +10 at (2, class 1); the source stays
            (11, MI, 2, 0, 0, 3), (11, MI, 2, 0, 0, -1),          # newPopulation outside [0, P)
            (12, SC, 0, 0, 1, 0),
            (0, B, 0, 0, 0, 0), (-7, B, 0, 0, 0, 0),              # step 2: num = 0 and negative num: nothing, not in `outside` either
            (2, B, 0, 3, 0, 0), (2, D, 0, -1, 0, 0), (2, 6, 0, 0, 0, 0), (2, -1, 0, 0, 0, 0), (2, 7, 0, 0, 0, 0),   # keys / types out of range
            (2, B, 5, 0, 0, 0), (2, MU, 5, 0, 2, 0),              # haplotype outside [0, H): that side changes nothing
            (2, B, 0, 2 ** 32, 0, 0), (2, B, 2 ** 32 + 1, 0, 0, 0), (2, MI, 0, 1, 0, 2 ** 40 + 1),   # a field beyond 32 bits matches nothing
            (2, MU, 0, 0, 2 ** 32 + 2, 0),                        # ... on one side of a MUTATION: the other side changes
            (13, B | DIRECT, 2, 2, 0, 0)]                         # the direct flag of a flattened row is masked off
    events = [(0.25, B, 0, 0, 0, 0), (1.0, MULTI, 0, 3, 0, 0), (2.0, MULTI, 3, 12, 0, 0), (3.0, MULTI, 12, 26, 0, 0)]
    ev, mev = make(events, rows)
    grid = np.array([0.5, 1.5, 2.5, 3.5])
    values, final, outside = assert_hook_equals(ev, mev, P, H, grid, vo, V, start, tile=4)
    want = start.copy(); want[0, 0] += 1
    assert np.array_equal(values[0], want)
    want[0, 0] += 2; want[1, 1] -= 3; want[2, 2] -= 4
    assert np.array_equal(values[1], want)
    want[1, 0] -= 6; want[1, 1] += 6; want[2, 2] += 7; want[2, 2] -= 8; want[2, 1] += 10
    assert np.array_equal(values[2], want)
    want[0, 1] += 2; want[0, 0] -= 2; want[2, 1] += 13
    assert np.array_equal(values[3], want) and np.array_equal(final, want)
    assert outside.tolist() == [1, 0]
    # one grid point in front of the last step: its rows with positive num lie behind the grid, whether they change a cell or not
    _, _, outside = assert_hook_equals(ev, mev, P, H, np.array([2.5]), vo, V, start, tile=5)
    assert outside.tolist() == [1 + (2 + 3 + 4) + (5 + 6 + 7 + 8 + 9 + 10 + 11 + 11 + 12), 2 * 11 + 13]
    # the rows the flattening accepts give the same as prefix rows
    ev3 = [c[:3] for c in ev]
    for n_own in (-1, 0, 1):
        assert_hook_equals(ev3, mev, P, H, grid, vo, V, start, tile=2, n_own=n_own, what=n_own)


def test_net_changes_and_values_beyond_32_bits_are_exact():
    P, H = 2, 3
    big = 2 ** 31 + 5
    rows = [(big, B, 1, 1, 0, 0), (big, B, 1, 1, 0, 0), (big, B, 1, 1, 0, 0), (7, D, 1, 1, 0, 0),
            (2 * big, SA, 1, 1, 0, 0), (big, MU, 1, 1, 2, 0), (3, B, 0, 0, 0, 0)]
    events = [(1.0, MULTI, 0, 4, 0, 0), (2.0, MULTI, 4, 6, 0, 0), (3.0, MULTI, 6, 7, 0, 0)]
    ev, mev = make(events, rows)
    start = np.array([[0, 0, 0], [0, 11, 0]])
    for n_own in (-1, 0, 1):
        for tile in (0, 1, 2):
            values, final, outside = assert_hook_equals(ev, mev, P, H, np.array([1.5, 2.5]), np.arange(H), H, start, tile=tile, n_own=n_own)
            assert 3 * big - 7 > 2 ** 32 and values[0, 1, 1] == 11 + 3 * big - 7          # a net change and a value beyond 2^32
            assert values[1, 1, 1] == 11 - 7 and values[1, 1, 2] == big and final[0, 0] == 3
            assert outside.tolist() == [3 * big + 7, 3]


# ---- refusals
def test_the_hooks_refusals():
    ev, mev = make([(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 1, 0, 0)], [(1, B, 0, 0, 0, 0)])
    ok, vo, start = np.array([0.0, 2.0]), np.arange(2), np.zeros((2, 2))
    for grid, text in (([0.0, 1.0, 1.0], "increase strictly"), ([1.0, 0.5], "increase strictly"), ([0.0, float("nan")], "not finite"),
                       ([float("inf")], "not finite"), ([], "T = 0")):
        with pytest.raises(ValueError, match="vgx_test_tau_prevalence: .*" + text):
            hook(ev, mev, 2, 2, np.array(grid), vo, 2, start)
    one = make([(0.5, B, 0, 0, 0, 0)], [])
    values, final, _ = hook(*one, 1, 1, np.array([1.0]), np.array([8191]), 8192, np.zeros((1, 8192)))   # 8 * 8192 = 65536 bytes fit
    assert values[0, 0, 8191] == 1 and values.sum() == 1 and final.sum() == 1
    with pytest.raises(ValueError, match="1 populations x 8193 classes need 65544 bytes"):
        hook(*one, 1, 1, np.array([1.0]), np.array([0]), 8193, np.zeros((1, 8193)))
    with pytest.raises(ValueError, match=r"variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook(ev, mev, 2, 2, ok, np.array([0, 2]), 2, start)
    with pytest.raises(ValueError, match=r"variant_of\[0\] = -2 is outside"):
        hook(ev, mev, 2, 2, ok, np.array([-2, 0]), 2, start)
    with pytest.raises(ValueError, match="V = 0"):
        hook(ev, mev, 2, 2, ok, np.array([-1, -1]), 0, np.zeros((2, 0)))
    for n_own in (-1, 0):                                            # as an own step and as part of the prefix
        for bad in ((1.0, MULTI, 0, 2, 0, 0), (1.0, MULTI, -1, 1, 0, 0)):
            ev2, _ = make([(0.5, B, 0, 0, 0, 0), bad], [])
            with pytest.raises(ValueError, match="MULTITYPE row range outside the multievent log"):
                hook(ev2, mev, 2, 2, ok, vo, 2, start, n_own=n_own)
    with pytest.raises(ValueError, match="n_own_events"):
        hook(ev, mev, 2, 2, ok, vo, 2, start, n_own=3)
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook(ev, mev, 2, 2, ok, vo, 2, start, tile=-1)
    neg = make([(1.0, MULTI, 0, 1, 0, 0)], [(-1, B, 0, 0, 0, 0)])
    with pytest.raises(ValueError, match="value out of range"):      # the prefix passes the checks of the flattening
        hook(*neg, 2, 2, ok, vo, 2, start, n_own=0)


# ---- Ensemble.tau_prevalence: refusals before the library (popNum 3, hapNum 40, 6 replicates)
@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either times or points"),
    (dict(times=[0.0, 1.0], points=4, window=(0, 1)), "either times or points"),
    (dict(points=0, window=(0, 1)), "points must be at least 1"),
    (dict(points=4), "window"),
    (dict(points=4, window=(1.0, 1.0)), "increase strictly"),
    (dict(times=[0.0, 1.0, 1.0]), "grid must increase strictly"),
    (dict(times=[]), "at least one"),
    (dict(times=[0.0, float("nan")]), "finite"),
    (dict(points=4, window=(0.0, float("inf"))), "finite"),
    (dict(times=[0.0], variants=[[0, 1], [40]]), "haplotype index out of range"),
    (dict(times=[0.0], variants=[[0, 1], [2, 1]]), "listed twice"),
    (dict(times=[0.0], variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(times=[0.0], variants=np.full(40, -2)), r"variant_of\[0\] = -2 is outside \[-1, 1\)"),
    (dict(times=[0.0], variants=np.arange(40) * 200), "3 populations x 7801 classes need 187224 bytes"),
    (dict(times=[0.0], variants=np.arange(40) * 70), "3 populations x 2731 classes need 65544 bytes"),   # (fits with 4-byte cells)
    (dict(times=[0.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(times=[0.0], replicates=[1, 1]), "distinct"),
    (dict(times=[0.0], values=False), "values=False needs summary"),
    (dict(times=[0.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(times=[0.0], summary=dict(method='nearest')), "method must be"),
    (dict(times=[0.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=('tau', True)).tau_prevalence(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate_tau"), (('direct', True), "tau chains only"), (('tau', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=r"tau_prevalence\(\).*" + text):
        bare_ensemble(last=last).tau_prevalence(times=[0.0, 1.0])
    with pytest.raises(ValueError, match=r"^prevalence\(\) counts direct chains only"):   # the direct call still refuses tau chains
        bare_ensemble(last=('tau', True)).prevalence(times=[0.0, 1.0])


def test_share_of_an_int64_block():
    from vgsim_amd.ensemble import Prevalence
    pv = Prevalence()
    pv.values = np.array([[[[2 ** 33, 3 * 2 ** 33], [0, 0]]]], dtype=np.int64)
    assert pv.share().tolist() == [[[[0.25, 0.75], [0.0, 0.0]]]] and pv.share().dtype == np.float64
