"""The milestones rule of tau chains (vgsim_amd/csrc/vgx_tau_milestones.h: tiles of whole events, the tile bases of pass A, the
per-event settle of the touched cells, the prefix walked once as a chain of its own, the merge of tiles in order, the end of a
chain), compiled for the host and reached through vgx_test_tau_milestones: the CPU oracle's tau chains, every split of a chain
into prefix and own events, tile sizes and hand-made chains against the literal restatement below (event by event, all rows of
the event applied, then every cell looked at; no tiles; never the code under test), integers with array_equal, times equal with
NaN at the same places; and the argument checks of Ensemble.tau_milestones, which are raised before the library is called.
No GPU."""
import numpy as np
import pytest

from test_incidence_rule import bare_ensemble
from test_milestones_rule import same_times
from test_prevalence_rule import deltas, fold
from test_tau_incidence_rule import CHAINS, make, oracle_chain
from test_tau_prevalence_rule import rows_of_events, three_maps

B, D, SA, MU, SC, MI, MULTI = range(7)
DIRECT = 0x100                                               # VGX_TL_ROW_DIRECT
NEVER = 2 ** 31 - 1
TILES = (1, 2, 3, 7, 64, 4096, 0)
INT64_FIELDS = ("final", "peak")
INT32_FIELDS = ("peak_event", "last_positive_event", "first_event")
TIME_FIELDS = ("peak_time", "extinction_time", "first_time")


def restate(events, mev, P, variant_of, V, start, thresholds=(), t_start=0.0, rows=None):
    """The rule as one Python loop over the EVENTS of a chain on the [P + 1, V] table of cells: all rows of event i are applied,
    then every cell is looked at."""
    times = np.asarray(events[0], dtype=np.float64)
    rows = rows_of_events(events, mev) if rows is None else rows
    n, K = len(times), len(thresholds)
    x = np.zeros((P + 1, V), dtype=np.int64)
    x[:P] = np.asarray(start, dtype=np.int64).reshape(P, V)
    x[P] = x[:P].sum(axis=0)
    peak, peak_event = x.copy(), np.full((P + 1, V), -1, dtype=np.int64)
    first = np.full((K, P + 1, V), NEVER, dtype=np.int64)
    for k, th in enumerate(thresholds):
        first[k][x >= th] = -1
    last = np.where(x > 0, -1, -2)
    for i in range(n):
        for num, *rec in rows[i]:
            if num <= 0:
                continue
            if rec[0] >= 0:
                rec[0] &= ~DIRECT                            # the direct flag of a flattened row
            rec = [v if 0 <= v < 2 ** 31 else -1 for v in rec]   # a field that is not a 32-bit index matches nothing
            for p, c, d in deltas(rec, P, variant_of):
                x[p, c] += d * num
                x[P, c] += d * num
        higher = x > peak
        peak[higher], peak_event[higher] = x[higher], i
        for k, th in enumerate(thresholds):
            first[k][(first[k] == NEVER) & (x >= th)] = i
        last[x > 0] = i

    def time_of(ev):
        ev = np.asarray(ev)
        t = np.full(ev.shape, np.nan)
        t[ev == -1] = t_start
        inside = (ev >= 0) & (ev < n)
        t[inside] = times[ev[inside]]
        return t
    extinct = (last >= -1) & (x == 0)
    return dict(final=x, peak=peak, peak_event=peak_event, last_positive_event=last, first_event=first, peak_time=time_of(peak_event),
                first_time=time_of(first), extinction_time=np.where(extinct, time_of(np.where(extinct, last + 1, NEVER)), np.nan),
                extinct=extinct, reached=first != NEVER, never_present=last == -2)


def assert_same(got, want, what=""):
    for k in INT64_FIELDS + INT32_FIELDS:
        assert got[k].dtype == (np.int64 if k in INT64_FIELDS else np.int32) and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in TIME_FIELDS:
        assert got[k].dtype == np.float64 and same_times(got[k], want[k]), (what, k)


def hook(events, mev, P, H, variant_of, V, start, thresholds=(), tile=0, n_own=-1, t_start=0.0):
    from vgsim_amd import _capi
    return _capi.replay_tau_milestones(events, mev, P, H, variant_of, V, start, thresholds, tile, n_own, t_start)


def check(events, mev, P, H, variant_of, V, start, thresholds=(), t_start=0.0, tiles=TILES, n_owns=None, rows=None):
    """The hook at every tile size and split against the restatement; returns the restatement."""
    want = restate(events, mev, P, variant_of, V, start, thresholds, t_start, rows)
    n = len(events[0])
    for n_own in ((-1, 0, n, n // 2) if n_owns is None else n_owns):
        for tile in tiles:
            assert_same(hook(events, mev, P, H, variant_of, V, start, thresholds, tile, n_own, t_start), want, (tile, n_own))
    return want


def one_cell(events, rows, start, thresholds=(), **kw):
    """A chain on one population and one haplotype."""
    ev, mev = make(events, rows)
    return check(ev, mev, 1, 1, np.array([0]), 1, np.array([[start]]), thresholds, **kw)


def steps(ranges, t0=1.0):
    """MULTITYPE events over consecutive row ranges of the given lengths, at times t0, t0 + 1, ..."""
    out, at = [], 0
    for k, n in enumerate(ranges):
        out.append((t0 + k, MULTI, at, at + n, 0, 0))
        at += n
    return out


# ---- the oracle's chains
@pytest.mark.parametrize("name", CHAINS)
def test_hook_equals_restatement_on_oracle_chains(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any()
    P, H = m.popNum, m.hapNum
    rows = rows_of_events(ev, mev)
    for k, (vo, V) in enumerate(three_maps(H, rows)[::2] + ((np.zeros(H, dtype=np.int64), 1),)):   # identity, three classes with one untracked, one class
        w = check(ev, mev, P, H, vo, V, fold(m.initial_infectious, vo, V), (1, 2, 50, 1000, 10 ** 9), n_owns=(-1,), rows=rows)
        assert np.array_equal(w["final"][:P], fold(m.infectious, vo, V)) and np.array_equal(w["final"][P], w["final"][:P].sum(axis=0))
        assert not w["reached"][4].any() and ((vo < 0).all() or (w["reached"][0].any() and (w["peak_event"] >= 0).any())), (name, k)   # (a model of one haplotype: that one untracked)


def test_every_split_into_prefix_and_own_events_gives_the_whole_chain(oracle_mod):
    m, ev, mev = oracle_chain(oracle_mod, "tau_then_direct")       # direct, tau steps, direct again: a mixed chain
    a = int(np.argmax(ev[1] == MULTI))
    ev = [c[max(0, a - 30):max(0, a - 30) + 60] for c in ev]
    n, P, H = len(ev[0]), m.popNum, m.hapNum
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any() and n == 60
    vo = np.arange(H) % 3
    start = np.full((P, 3), 40)                                    # (a slice of a chain: cells cross zero and come back)
    want = restate(ev, mev, P, vo, 3, start, (30, 41, 45, 100))
    assert want["reached"][1].any() and not want["reached"][1].all() and len(np.unique(want["peak_event"])) > 3
    for k in range(n + 1):
        for tile in (1, 7, 0):
            assert_same(hook(ev, mev, P, H, vo, 3, start, (30, 41, 45, 100), tile, k), want, (k, tile))


# ---- hand-made chains, each at every tile size and with the chain split in several places
def test_a_step_that_adds_and_takes_the_same_amount():
    w = one_cell(steps([2, 1]), [(5, B, 0, 0, 0, 0), (5, D, 0, 0, 0, 0), (1, B, 0, 0, 0, 0)], 2, thresholds=(4, 3))
    assert w["first_event"][:, 0, 0].tolist() == [NEVER, 1]          # 7 inside step 0 is not a value
    assert w["peak"][0, 0] == 3 and w["peak_event"][0, 0] == 1
    w = one_cell(steps([2]), [(5, D, 0, 0, 0, 0), (5, B, 0, 0, 0, 0)], 2, thresholds=(4,))
    assert w["peak"][0, 0] == 2 and w["peak_event"][0, 0] == -1 and w["last_positive_event"][0, 0] == 0


def test_a_cell_at_one_that_loses_and_gains_a_host_in_one_step():
    w = one_cell(steps([2, 0, 1]), [(1, D, 0, 0, 0, 0), (1, B, 0, 0, 0, 0), (1, SA, 0, 0, 0, 0)], 1)
    assert w["last_positive_event"][0, 0] == 1 and w["extinct"][0, 0] and w["extinction_time"][0, 0] == 3.0
    w = one_cell(steps([2, 0]), [(1, D, 0, 0, 0, 0), (1, B, 0, 0, 0, 0)], 1)
    assert w["last_positive_event"][0, 0] == 1 and not w["extinct"][0, 0] and w["final"][0, 0] == 1


def test_extinction_and_return():
    rows = [(2, D, 0, 0, 0, 0), (3, B, 0, 0, 0, 0), (3, D, 0, 0, 0, 0), (1, B, 0, 0, 0, 0), (1, D, 0, 0, 0, 0)]
    w = one_cell(steps([1, 1, 1, 1, 1]), rows, 2)                     # 0 at event 0, back at 1, 0 at 2, back at 3, gone at 4
    assert w["last_positive_event"][0, 0] == 3 and w["extinct"][0, 0] and w["extinction_time"][0, 0] == 5.0
    w = one_cell(steps([1, 1, 1, 1]), rows[:4], 2)
    assert w["last_positive_event"][0, 0] == 3 and not w["extinct"][0, 0]
    w = one_cell(steps([1]), [(5, D, 0, 0, 0, 0)], 2, thresholds=(0, -3, -2))    # below zero is not positive; the start was the last
    assert w["last_positive_event"][0, 0] == -1 and w["final"][0, 0] == -3 and not w["extinct"][0, 0]
    assert w["first_event"][:, 0, 0].tolist() == [-1, -1, -1]


def test_a_peak_tie_between_a_prefix_event_and_an_own_step():
    events = [(0.5, B, 0, 0, 0, 0), (0.75, D, 0, 0, 0, 0)] + steps([1, 1, 1])
    w = one_cell(events, [(1, B, 0, 0, 0, 0), (1, D, 0, 0, 0, 0), (1, B, 0, 0, 0, 0)], 2, n_owns=(-1, 3, 0, 5, 1))
    assert w["peak"][0, 0] == 3 and w["peak_event"][0, 0] == 0 and w["peak_time"][0, 0] == 0.5   # 3 again at events 2 and 4


def test_thresholds_met_at_the_start_the_last_prefix_event_and_the_first_own_step():
    events = [(0.5, B, 0, 0, 0, 0), (0.75, B, 0, 0, 0, 0)] + steps([1, 1])
    w = one_cell(events, [(2, B, 0, 0, 0, 0), (1, B, 0, 0, 0, 0)], 3, thresholds=(3, 5, 6, 7, 8, 9), t_start=0.125, n_owns=(-1, 2, 0, 4))
    assert w["first_event"][:, 0, 0].tolist() == [-1, 1, 2, 2, 3, NEVER]
    assert w["first_time"][:5, 0, 0].tolist() == [0.125, 0.75, 1.0, 1.0, 2.0] and np.isnan(w["first_time"][5, 0, 0])


def test_steps_without_rows_in_the_middle_and_at_the_end():
    w = one_cell(steps([1, 0, 1, 0, 0]), [(1, B, 0, 0, 0, 0), (1, B, 0, 0, 0, 0)], 0, thresholds=(2,))
    assert w["last_positive_event"][0, 0] == 4 and w["final"][0, 0] == 2 and w["first_event"][0, 0, 0] == 2
    assert w["peak_event"][0, 0] == 2 and not w["extinct"][0, 0] and np.isnan(w["extinction_time"][0, 0])
    w = one_cell(steps([1, 0, 0]), [(1, D, 0, 0, 0, 0)], 1)           # emptied at event 0, empty steps behind
    assert w["last_positive_event"][0, 0] == -1 and w["extinct"][0, 0] and w["extinction_time"][0, 0] == 1.0


def test_a_chain_of_zero_events_and_a_prefix_without_own_steps():
    P, H, vo = 2, 3, np.array([0, 1, -1])
    ev, mev = make([], [])
    w = check(ev, mev, P, H, vo, 2, np.array([[0, 2], [1, 0]]), thresholds=(1, 2, 3), t_start=1.5)
    assert w["final"].tolist() == [[0, 2], [1, 0], [1, 2]] and np.array_equal(w["peak"], w["final"]) and (w["peak_event"] == -1).all()
    assert w["last_positive_event"].tolist() == [[-2, -1], [-1, -2], [-1, -1]] and not w["extinct"].any()
    assert w["first_event"][1].tolist() == [[NEVER, -1], [NEVER, NEVER], [NEVER, -1]] and w["first_time"][1, 0, 1] == 1.5
    ev, mev = make([(0.5, B, 0, 0, 0, 0), (0.75, D, 1, 0, 0, 0), (1.0, D, 1, 0, 0, 0)], [])
    w = check(ev, mev, P, H, vo, 2, np.array([[0, 2], [1, 0]]), thresholds=(1,), n_owns=(0, -1))
    assert w["final"][0].tolist() == [1, 0] and w["extinct"][0, 1] and w["extinction_time"][0, 1] == 1.0


def test_long_steps_wide_steps_and_steps_larger_than_the_tile():
    P, H = 20, 20
    rng = np.random.default_rng(5)
    wide = [(int(rng.integers(1, 9)), B, h, p, 0, 0) for p in range(P) for h in range(H)]             # 400 distinct cells in one step
    long_ = [(int(rng.integers(1, 5)), int(rng.choice([B, D, SA])), int(rng.integers(0, 3)), int(rng.integers(0, 2)), 0, 0) for _ in range(700)]
    back = [(9, D, h, p, 0, 0) for p in range(P) for h in range(0, H, 2)]
    ev, mev = make(steps([len(wide), 3, len(long_), len(back), 5]), wide + long_[:3] + long_ + back + long_[:5])
    for vo, V in ((np.arange(H), H), (np.arange(H) % 3, 3)):
        w = check(ev, mev, P, H, vo, V, np.zeros((P, V)), thresholds=(1, 9, 40, 60), tiles=TILES + (256, 257, 699, 700, 701), n_owns=(-1, 0, 2))
        assert (w["peak_event"] == 0).any() and (w["final"] < 0).any() and w["reached"][3].any() and not w["reached"][3].all()


def test_mutations_migrations_and_rows_that_count_nowhere():
    P, H, V = 3, 5, 3
    vo = np.array([0, 0, 1, 2, -1])                               # haplotypes 0 and 1 share class 0; 4 is not tracked
    start = np.array([[20, 1, 0], [0, 30, 1], [1, 0, 0]])
    rows = [(5, MU, 0, 0, 1, 0),                                  # step 0: within class 0: nothing
            (6, MU, 0, 0, 2, 0),                                  # class 0 -> 1 in population 0: row P of both classes, whose totals stay
            (10, MI, 2, 1, 7, 2),                                 # step 1: +10 at (2, class 1) and (P, class 1); the source stays
            (7, MU, 4, 2, 3, 0), (8, MU, 3, 2, 4, 0), (9, MU, 4, 0, 4, 0),   # step 2: untracked on one side, on both
            (11, MI, 2, 0, 0, 3), (11, MI, 2, 0, 0, -1), (12, SC, 0, 0, 1, 0),
            (0, B, 0, 0, 0, 0), (-7, B, 0, 0, 0, 0),              # step 3: num = 0 and negative num
            (2, B, 0, 3, 0, 0), (2, D, 0, -1, 0, 0), (2, 6, 0, 0, 0, 0), (2, -1, 0, 0, 0, 0), (2, 7, 0, 0, 0, 0),
            (2, B, 5, 0, 0, 0), (2, B, 0, 2 ** 32, 0, 0), (2, B, 2 ** 32 + 1, 0, 0, 0), (2, MI, 0, 1, 0, 2 ** 40 + 1),
            (2, MU, 5, 0, 2, 0), (2, MU, 0, 0, 2 ** 32 + 2, 0),   # step 4: one side of a MUTATION outside: the other side changes
            (13, B | DIRECT, 2, 2, 0, 0)]                         # the direct flag of a flattened row is masked off
    ev, mev = make([(0.25, B, 0, 0, 0, 0)] + steps([2, 1, 6, 11, 3]), rows)
    w = check(ev, mev, P, H, vo, V, start, thresholds=(21, 25, 31, 42), n_owns=(-1,))
    assert w["final"].tolist() == [[13, 9, 0], [0, 30, 1], [1, 23, -1], [14, 62, 0]]
    assert w["peak"][3].tolist() == [22, 62, 1] and w["peak_event"][3].tolist() == [0, 5, -1]   # +7 and -8 in one step: no peak of 8
    assert w["peak"][1, 1] == 30 and w["peak_event"][1, 1] == -1                       # the migration's source stays
    assert w["first_event"][:, 3, 1].tolist() == [-1, -1, -1, 2]
    assert w["last_positive_event"][2].tolist() == [5, 5, -2] and w["last_positive_event"][3, 2] == 2 and w["extinct"][3, 2]
    ev3 = [c[:4] for c in ev]                                     # the rows the flattening accepts give the same as prefix rows
    check(ev3, mev, P, H, vo, V, start, thresholds=(21, 25, 31, 42))


def test_values_and_thresholds_beyond_32_bits():
    big = 10 ** 12
    rows = [(big, B, 0, 0, 0, 0), (big, B, 0, 0, 0, 0), (big, B, 0, 0, 0, 0), (7, D, 0, 0, 0, 0), (2 * big, SA, 0, 0, 0, 0), (big - 7, D, 0, 0, 0, 0)]
    w = one_cell(steps([2, 2, 1, 1]), rows, 11, thresholds=(2 ** 32 + 1, 2 * big + 11, 2 * big + 12, 3 * big, -2 ** 62, 2 ** 62))
    assert w["peak"][0, 0] == 3 * big + 4 and w["peak_event"][0, 0] == 1 and w["peak"].dtype == np.int64
    assert w["first_event"][:, 0, 0].tolist() == [0, 0, 1, 1, -1, NEVER]
    assert w["final"][0, 0] == 11 and w["last_positive_event"][0, 0] == 3


def test_times_that_go_back():
    events = [(5.0, B, 0, 0, 0, 0), (6.0, MULTI, 0, 1, 0, 0), (0.5, MULTI, 1, 2, 0, 0), (0.25, MULTI, 2, 3, 0, 0)]   # (a restart: the clock starts again)
    w = one_cell(events, [(2, B, 0, 0, 0, 0), (1, B, 0, 0, 0, 0), (4, D, 0, 0, 0, 0)], 0, thresholds=(4,))
    assert w["peak_time"][0, 0] == 0.5 and w["first_time"][0, 0, 0] == 0.5 and w["extinction_time"][0, 0] == 0.25


def test_random_rows_at_every_tile_size():
    rng = np.random.default_rng(83)
    n_ev, P, H = 120, 4, 12
    lens = rng.choice([0, 1, 2, 5, 40], n_ev)
    total = int(lens.sum())
    rows = list(zip(rng.integers(-1, 6, total).tolist(), rng.integers(-1, 8, total).tolist(), rng.integers(-1, H + 1, total).tolist(),
                    rng.integers(-1, P + 1, total).tolist(), rng.integers(-1, H + 1, total).tolist(), rng.integers(-1, P + 1, total).tolist()))
    n_pre_rows = int(lens[:n_ev - 37].sum())                       # the prefix of the split below passes the checks of the flattening
    rows[:n_pre_rows] = [(max(r[0], 0), max(r[1], 0)) + r[2:] for r in rows[:n_pre_rows]]
    ev, mev = make(steps(lens.tolist()), rows)
    ev[0] = np.sort(rng.uniform(0.0, 10.0, n_ev))
    classes = np.arange(H) % 3 - (np.arange(H) % 5 == 0)
    for vo, V in ((np.arange(H), H), (classes, 3)):
        w = check(ev, mev, P, H, vo, V, rng.integers(0, 6, (P, V)), thresholds=(1, 5, 12, -3, 60), tiles=TILES + (41, total), n_owns=(-1, 37))
        assert w["extinct"].any() and (~w["extinct"]).any() and (w["final"] < 0).any() and len(np.unique(w["peak_event"])) > 5


# ---- the hook's refusals
def test_the_hooks_refusals():
    ev, mev = make([(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 1, 0, 0)], [(1, B, 0, 0, 0, 0)])
    vo, start = np.arange(2), np.zeros((2, 2))
    one = make([(0.5, B, 0, 0, 0, 0)], [])
    got = hook(*one, 1, 1, np.array([584]), 585, np.zeros((1, 585)), thresholds=(1, 2, 3, 4))   # 2 x 585 x 56 + 16 = 65536 bytes fit
    assert got["peak"][0, 584] == 1 and got["peak"].sum() == 2 and got["first_event"][0, 1, 584] == 0
    with pytest.raises(ValueError, match=r"vgx_test_tau_milestones: 1 populations \(and their total\) x 586 classes x 4 thresholds need 65648 bytes of records, "
                                         "above the 65536 bytes of LDS"):
        hook(*one, 1, 1, np.array([0]), 586, np.zeros((1, 586)), thresholds=(1, 2, 3, 4))
    with pytest.raises(ValueError, match="vgx_test_tau_milestones: K = 17 thresholds: at most 16"):
        hook(ev, mev, 2, 2, vo, 2, start, thresholds=range(17))
    assert hook(*one, 1, 1, np.array([0]), 1, np.zeros((1, 1)), thresholds=range(16))["first_event"][:, 0, 0].tolist() == [-1, 0] + [NEVER] * 14
    with pytest.raises(ValueError, match=r"variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook(ev, mev, 2, 2, np.array([0, 2]), 2, start)
    with pytest.raises(ValueError, match=r"variant_of\[0\] = -2 is outside"):
        hook(ev, mev, 2, 2, np.array([-2, 0]), 2, start)
    with pytest.raises(ValueError, match="V = 0"):
        hook(ev, mev, 2, 2, np.array([-1, -1]), 0, np.zeros((2, 0)))
    for n_own in (-1, 0):                                            # as an own step and as part of the prefix
        for bad in ((1.0, MULTI, 0, 2, 0, 0), (1.0, MULTI, -1, 1, 0, 0)):
            ev2, _ = make([(0.5, B, 0, 0, 0, 0), bad], [])
            with pytest.raises(ValueError, match="MULTITYPE row range outside the multievent log"):
                hook(ev2, mev, 2, 2, vo, 2, start, n_own=n_own)
    with pytest.raises(ValueError, match="n_own_events"):
        hook(ev, mev, 2, 2, vo, 2, start, n_own=3)
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook(ev, mev, 2, 2, vo, 2, start, tile=-1)
    neg = make([(1.0, MULTI, 0, 1, 0, 0)], [(-1, B, 0, 0, 0, 0)])
    with pytest.raises(ValueError, match="value out of range"):      # the prefix passes the checks of the flattening
        hook(*neg, 2, 2, vo, 2, start, n_own=0)


# ---- Ensemble.tau_milestones: refusals before the library (popNum 3, hapNum 40, 6 replicates)
@pytest.mark.parametrize("kwargs, text", [
    (dict(variants=[[0, 1], [40]]), "haplotype index out of range"),
    (dict(variants=[[0, 1], [2, 1]]), "listed twice"),
    (dict(variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(variants=np.full(40, -2)), r"variant_of\[0\] = -2 is outside \[-1, 1\)"),
    (dict(variants=np.zeros(40)), "integer"),
    (dict(variants=np.arange(40) * 200), r"3 populations \(and their total\) x 7801 classes x 0 thresholds need 1248176 bytes of records"),
    (dict(variants=np.arange(40) * 10, thresholds=range(7)), r"3 populations \(and their total\) x 391 classes x 7 thresholds need 106368 bytes"),
    (dict(thresholds=range(17)), "K = 17 thresholds: at most 16"),
    (dict(thresholds=[1.5]), "thresholds must be integers"),
    (dict(thresholds=[2 ** 63]), "integers in int64"),
    (dict(thresholds=[-2 ** 63 - 1]), "integers in int64"),
    (dict(thresholds=[[1, 2]]), "sequence of integers"),
    (dict(replicates=[0, 6]), "replicate index out of range"),
    (dict(replicates=[-1]), "replicate index out of range"),
    (dict(replicates=[1, 1]), "distinct"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=('tau', True)).tau_milestones(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate_tau"), (('direct', True), "tau chains only"), (('tau', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=r"tau_milestones\(\).*" + text):
        bare_ensemble(last=last).tau_milestones(thresholds=(10,))


def test_thresholds_of_any_int64_pass_the_check():
    from vgsim_amd import _capi
    th = _capi.tau_milestone_thresholds([2 ** 63 - 1, -2 ** 63, 2 ** 40])
    assert th.dtype == np.int64 and th.tolist() == [2 ** 63 - 1, -2 ** 63, 2 ** 40]
    assert _capi.tau_milestone_thresholds(()).shape == (0,) and _capi.tau_milestone_thresholds(None).dtype == np.int64


def test_an_int64_result_through_the_derived_properties():
    from vgsim_amd.ensemble import Milestones
    ms = Milestones()
    ms.last_positive_event = np.array([[[3]], [[-2]], [[-1]], [[7]]], dtype=np.int32)   # 4 replicates, one cell
    ms.final = np.array([[[0]], [[0]], [[0]], [[2 ** 40]]], dtype=np.int64)
    ms.replicates = np.array([5, 0, 2, 3])
    ms._R, ms._scenario_of, ms._n_scenarios = 6, None, 1
    assert ms.extinct[:, 0, 0].tolist() == [True, False, True, False] and ms.never_present[:, 0, 0].tolist() == [False, True, False, False]
    assert ms.extinction_event[:, 0, 0].tolist() == [4, -1, 0, 8] and ms.extinction_event.dtype == np.int32
    assert ms.extinction_probability()[:, 0, 0].tolist() == [0.5]
    assert ms.extinction_probability(by=np.array([0, 0, 1, 1, 0, 0]))[:, 0, 0].tolist() == [0.5, 0.5]   # groups {5, 0} and {2, 3}
