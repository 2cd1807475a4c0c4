"""The milestones rule of the device pass (vgsim_amd/csrc/vgx_milestones.h: the cells a record changes with the row of all
populations, the tile bases, the ordered walk in rounds of 64 lanes with ballots and population counts, the merge of tiles by
extrema, the end of a chain), compiled for the host and reached through vgx_test_milestones: hand-made chains at every tile size,
the CPU oracle's chains and their final states, against the literal restatement below (never against the code under test), all
with array_equal (times: NaN at the same places, array_equal elsewhere); and the argument checks of Ensemble.milestones, which
are raised before the library is called.  No GPU."""
import numpy as np
import pytest

from test_incidence_rule import ORACLE_CASES, bare_ensemble, chain_of, columns, oracle_model
from test_prevalence_rule import deltas, fold

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
NEVER = 2 ** 31 - 1
TILES = (1, 2, 3, 7, 64, 4096, 0)
INT_FIELDS = ("final", "peak", "peak_event", "last_positive_event", "first_event")
TIME_FIELDS = ("peak_time", "extinction_time", "first_time")


def restate(times, cols, P, variant_of, V, start, thresholds=(), t_start=0.0):
    """Section 1 of the feature's rule as one Python loop over the events of a chain, on the [P + 1, V] table of cells."""
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
        for p, c, d in deltas([col[i] for col in cols], P, variant_of):
            x[p, c] += d
            x[P, c] += d
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
        t[inside] = np.asarray(times, dtype=np.float64)[ev[inside]]
        return t
    extinct = (last >= -1) & (x == 0)
    return dict(final=x, peak=peak, peak_event=peak_event, last_positive_event=last, first_event=first, peak_time=time_of(peak_event),
                first_time=time_of(first), extinction_time=np.where(extinct, time_of(np.where(extinct, last + 1, NEVER)), np.nan),
                extinct=extinct, reached=first != NEVER, never_present=last == -2)


def same_times(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def assert_same(got, want, what=""):
    for k in INT_FIELDS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in TIME_FIELDS:
        assert got[k].dtype == np.float64 and same_times(got[k], want[k]), (what, k)


def hook(times, cols, P, H, variant_of, V, start, thresholds=(), tile=0, t_start=0.0):
    from vgsim_amd import _capi
    return _capi.replay_milestones(times, *cols, P, H, variant_of, V, start, thresholds, tile, t_start)


def check(times, cols, P, H, variant_of, V, start, thresholds=(), t_start=0.0, tiles=TILES):
    """The hook at every tile size against the restatement; returns the restatement."""
    times = np.asarray(times, dtype=np.float64)
    want = restate(times, cols, P, variant_of, V, start, thresholds, t_start)
    for tile in tiles:
        assert_same(hook(times, cols, P, H, variant_of, V, start, thresholds, tile, t_start), want, tile)
    return want


UP, DOWN = (BIRTH, 0, 0, 0, 0), (DEATH, 0, 0, 0, 0)


def one_cell(signs, start, thresholds=(), t_start=0.0):
    recs = [UP if s > 0 else DOWN for s in signs]
    return check(0.5 + np.arange(len(recs)) * 0.25, columns(recs), 1, 1, np.array([0]), 1, np.array([[start]]), thresholds, t_start)


# ---- hand-made chains, each at every tile size
def test_thresholds_at_the_start_at_tile_edges_and_never():
    w = one_cell([1] * 10, 3, thresholds=(3, -5, 0, 4, 1000), t_start=0.125)
    assert w["first_event"][:, 0, 0].tolist() == [-1, -1, -1, 0, NEVER]           # met by the start: event -1
    assert w["first_time"][:3, 0, 0].tolist() == [0.125] * 3 and w["first_time"][3, 0, 0] == 0.5
    assert np.isnan(w["first_time"][4, 0, 0]) and w["reached"][:, 0, 0].tolist() == [True] * 4 + [False]
    # with tiles of 2, 3, 7 and 64 events: thresholds met at the last event of a tile (1, 2, 6, 63) and at the first of the next
    w = one_cell([1] * 130, 0, thresholds=(2, 3, 4, 7, 8, 64, 65, 129, 130, 131))
    assert w["first_event"][:, 0, 0].tolist() == [1, 2, 3, 6, 7, 63, 64, 128, 129, NEVER]
    assert w["peak"][0, 0] == 130 and w["peak_event"][0, 0] == 129
    # K = 0
    w = one_cell([1, -1, 1], 1)
    assert w["first_event"].shape == (0, 2, 1) and w["peak"].tolist() == [[2], [2]]


def test_peaks():
    w = one_cell([1, 1, -1, 1, -1, -1, 1, 1, -1], 5, thresholds=(7,))               # 7 at events 1, 3 and 7: the first wins
    assert w["peak"][0, 0] == 7 and w["peak_event"][0, 0] == 1 and w["peak_time"][0, 0] == 0.75
    w = one_cell([-1, 1, -1, -1, 1], 4, t_start=0.25)                                # the start is the peak (attained again at 1)
    assert w["peak"][0, 0] == 4 and w["peak_event"][0, 0] == -1 and w["peak_time"][0, 0] == 0.25
    w = one_cell([1] * 70 + [-1] * 3 + [1] * 3 + [-1] * 60, 0)                       # attained twice, in different rounds of a tile
    assert w["peak"][0, 0] == 70 and w["peak_event"][0, 0] == 69


def test_extinction_and_return():
    w = one_cell([-1, -1, 1, 1, -1], 2)                                              # to zero at 1, back at 2
    assert w["last_positive_event"][0, 0] == 4 and not w["extinct"][0, 0] and np.isnan(w["extinction_time"][0, 0])
    w = one_cell([-1, -1, 1, -1], 2)                                                 # dies for good at event 3
    assert w["last_positive_event"][0, 0] == 2 and w["extinct"][0, 0] and w["final"][0, 0] == 0
    assert w["extinction_time"][0, 0] == 0.5 + 3 * 0.25
    w = one_cell([-1], 1)                                                            # the start is the last positive value
    assert w["last_positive_event"][0, 0] == -1 and w["extinct"][0, 0] and w["extinction_time"][0, 0] == 0.5
    w = one_cell([1] * 63 + [-1] * 63 + [1, -1], 0)                                  # zero at the last lane of a round, back in the next
    assert w["last_positive_event"][0, 0] == 126 and w["extinct"][0, 0]
    # never positive: -2, whatever the records do to other cells; below zero is not positive
    P, H, vo = 2, 2, np.array([0, 1])
    w = check([0.1, 0.2, 0.3], columns([(BIRTH, 0, 0, 0, 0), (DEATH, 1, 1, 0, 0), (DEATH, 0, 0, 0, 0)]), P, H, vo, 2, np.zeros((2, 2)), (0, -1))
    assert w["last_positive_event"].tolist() == [[1, -2], [-2, -2], [1, -2]] and w["never_present"][1].all()
    assert w["final"].tolist() == [[0, 0], [0, -1], [0, -1]] and w["peak"][1, 1] == 0 and w["peak_event"][1, 1] == -1
    assert w["first_event"][:, 1, 1].tolist() == [-1, -1] and not w["extinct"][1, 1]


def test_mutations_migrations_and_records_that_count_nowhere():
    P, H, V = 3, 5, 3
    vo = np.array([0, 0, 1, 2, -1])                                                  # haplotypes 0, 1 share class 0; 4 is not tracked
    start = np.array([[2, 1, 0], [0, 3, 1], [1, 0, 0]])
    recs = [(MUTATION, 0, 0, 1, 0),                                                  # within class 0: nothing
            (MUTATION, 0, 0, 2, 0),                                                  # class 0 -> 1 in population 0: row P of both classes
            (MIGRATION, 2, 1, 0, 2),                                                 # +1 at (2, class 1) and (P, class 1); source untouched
            (MUTATION, 4, 1, 3, 0), (MUTATION, 3, 1, 4, 0), (MUTATION, 4, 0, 4, 0),  # untracked haplotype on one side, on both
            (BIRTH, 4, 0, 0, 0), (BIRTH, 5, 0, 0, 0), (BIRTH, -1, 0, 0, 0), (DEATH, 0, 3, 0, 0), (DEATH, 0, -1, 0, 0),
            (MIGRATION, 2, 0, 0, 3), (MIGRATION, 2, 0, 0, -1), (SUSCCHANGE, 0, 0, 1, 0), (6, 0, 0, 0, 0), (-1, 0, 0, 0, 0),
            (MUTATION, 5, 0, 2, 0),                                                  # out of a haplotype outside [0, H): +1 only
            (MUTATION, 0, 3, 2, 0), (SAMPLING, 2, 1, 0, 0)]
    w = check(np.arange(len(recs)) * 0.5, columns(recs), P, H, vo, V, start, thresholds=(1, 2, 5))
    assert w["final"].tolist() == [[1, 3, 0], [0, 2, 1], [1, 1, 0], [2, 6, 1]]
    assert w["peak"][3].tolist() == [3, 7, 2] and w["peak_event"][3].tolist() == [-1, 16, 3]
    assert w["peak"][1, 1] == 3 and w["peak_event"][1, 1] == -1                      # the migration's source stays
    assert w["first_event"][2, 3].tolist() == [NEVER, 1, NEVER]                      # all populations reach 5 of class 1 at the mutation
    assert w["first_event"][1, 2].tolist() == [NEVER, NEVER, NEVER] and w["first_event"][0, 2].tolist() == [-1, 2, NEVER]
    assert np.array_equal(w["final"][3], w["final"][:3].sum(axis=0))


def test_130_alternating_events_on_one_cell():
    """Two full rounds plus two events: the in-round prefix arithmetic is wrong if any lane is off by one."""
    w = one_cell([1, -1] * 65, 0, thresholds=(1, 2))
    assert w["peak"][0, 0] == 1 and w["peak_event"][0, 0] == 0 and w["last_positive_event"][0, 0] == 128
    assert w["first_event"][:, 0, 0].tolist() == [0, NEVER] and w["extinct"][0, 0] and w["extinction_time"][0, 0] == 0.5 + 129 * 0.25
    w = one_cell([-1, 1] * 65, 1, thresholds=(1, 2))
    assert w["peak_event"][0, 0] == -1 and w["last_positive_event"][0, 0] == 129 and not w["extinct"][0, 0]
    w = one_cell([1, 1, -1] * 43 + [1], 0, thresholds=(43, 44, 45))
    assert w["final"][0, 0] == 44 and w["first_event"][:, 0, 0].tolist() == [124, 127, NEVER]


def test_more_than_64_distinct_cells_in_one_round():
    """64 events of one round that touch 64 different (population, class) cells and, with the row of all populations, 80 cells."""
    P, H = 8, 16
    recs = [(BIRTH, i % H, (i // H + i) % P, 0, 0) for i in range(64)] + [(DEATH, i % H, (i // H + i) % P, 0, 0) for i in range(0, 64, 3)]
    assert len({(r[1], r[2]) for r in recs[:64]}) == 64
    w = check(np.arange(len(recs)) * 0.125, columns(recs), P, H, np.arange(H), H, np.zeros((P, H)), thresholds=(1, 2, 4, 5))
    assert w["peak"][P].tolist() == [4] * H and w["first_event"][2, P].tolist() == list(range(48, 64)) and w["extinct"].sum() == 22


def test_a_chain_of_zero_events():
    P, H, vo = 2, 3, np.array([0, 1, -1])
    w = check([], columns([]), P, H, vo, 2, np.array([[0, 2], [1, 0]]), thresholds=(1, 2, 3), t_start=1.5)
    assert w["final"].tolist() == [[0, 2], [1, 0], [1, 2]] and np.array_equal(w["peak"], w["final"]) and (w["peak_event"] == -1).all()
    assert w["last_positive_event"].tolist() == [[-2, -1], [-1, -2], [-1, -1]] and not w["extinct"].any()
    assert w["first_event"][1].tolist() == [[NEVER, -1], [NEVER, NEVER], [NEVER, -1]] and w["first_time"][1, 0, 1] == 1.5


def test_random_records_at_every_tile_size():
    rng = np.random.default_rng(79)
    n, P, H = 700, 4, 12
    recs = np.stack([rng.integers(-1, 8, n), rng.integers(-1, H + 1, n), rng.integers(-1, P + 1, n), rng.integers(-1, H + 1, n),
                     rng.integers(-1, P + 1, n)], axis=1)
    t = np.sort(rng.uniform(0.0, 10.0, n))
    classes = np.arange(H) % 3 - (np.arange(H) % 5 == 0)
    for vo, V in ((np.arange(H), H), (classes, 3)):
        start = rng.integers(0, 3, (P, V))
        w = check(t, columns(recs), P, H, vo, V, start, thresholds=(1, 2, 4, -3, 9), tiles=TILES + (257, n - 1, n, n + 1))
        assert w["extinct"].any() and (~w["extinct"]).any() and (w["final"] < 0).any() and len(np.unique(w["peak_event"])) > 5


# ---- the oracle's chains
@pytest.fixture(scope="module")
def oracle_chains(oracle_mod):
    return {name: oracle_model(oracle_mod, name) for name in ORACLE_CASES}


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_chains(oracle_chains, name):
    m = oracle_chains[name]
    t, cols = chain_of(m)
    P, H = m.popNum, m.hapNum
    assert len(t) > 100
    busy = np.bincount(cols[1][(cols[1] >= 0) & (cols[1] < H)], minlength=H).argsort()[::-1]
    three = np.arange(H) % 3
    three[busy[1]] = -1
    thresholds = (1, 2, 5, 50, 10 ** 6)
    for vo, V in ((np.arange(H), H), (three, 3)):
        w = check(t, cols, P, H, vo, V, fold(m.initial_infectious, vo, V), thresholds)
        assert np.array_equal(w["final"][:P], fold(m.infectious, vo, V))
        assert np.array_equal(w["final"][P], w["final"][:P].sum(axis=0))
        assert (w["peak"][P] <= w["peak"][:P].sum(axis=0)).all()
        assert w["reached"][0].any() and not w["reached"][4].any() and (w["peak_event"] >= 0).any()


# ---- the hook's refusals
def test_the_hook_refuses_what_the_device_pass_refuses():
    one, vo = columns([UP]), np.array([0])
    got = hook([0.5], one, 1, 1, np.array([1023]), 1024, np.zeros((1, 1024)), thresholds=(1, 2, 3, 4))   # 2 x 1024 x 32 = 65536 bytes fit
    assert got["peak"][0, 1023] == 1 and got["peak"].sum() == 2 and got["first_event"][0, 1, 1023] == 0
    with pytest.raises(ValueError, match=r"vgx_test_milestones: 1 populations \(and their total\) x 1024 classes x 5 thresholds need 73728 bytes of records, "
                                         "above the 65536 bytes of LDS"):
        hook([0.5], one, 1, 1, np.array([0]), 1024, np.zeros((1, 1024)), thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="3 populations .* x 2731 classes x 0 thresholds need 174784 bytes"):
        hook([0.5], one, 3, 1, np.array([0]), 2731, np.zeros((3, 2731)))
    with pytest.raises(ValueError, match="vgx_test_milestones: K = 17 thresholds: at most 16"):
        hook([0.5], one, 1, 1, vo, 1, np.zeros((1, 1)), thresholds=range(17))
    assert hook([0.5], one, 1, 1, vo, 1, np.zeros((1, 1)), thresholds=range(16))["first_event"][:, 0, 0].tolist() == [-1, 0] + [NEVER] * 14
    with pytest.raises(ValueError, match=r"variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook([0.5], one, 1, 2, np.array([0, 2]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match=r"variant_of\[0\] = -2 is outside"):
        hook([0.5], one, 1, 2, np.array([-2, 0]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match="V = 0"):
        hook([0.5], one, 1, 1, np.array([-1]), 0, np.zeros((1, 0)))
    with pytest.raises(ValueError, match="start value outside"):
        hook([0.5], one, 1, 1, vo, 1, np.array([[-1]]))
    with pytest.raises(ValueError, match="start value outside"):                     # the sum over the populations too
        hook([0.5], one, 2, 1, vo, 1, np.array([[2 ** 30], [2 ** 30]]))
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook([0.5], one, 1, 1, vo, 1, np.zeros((1, 1)), tile=-1)


# ---- Ensemble.milestones: refusals before the library (popNum 3, hapNum 40, 6 replicates)
@pytest.mark.parametrize("kwargs, text", [
    (dict(variants=[[0, 1], [40]]), "haplotype index out of range"),
    (dict(variants=[[0, 1], [2, 1]]), "listed twice"),
    (dict(variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(variants=np.full(40, -2)), r"variant_of\[0\] = -2 is outside \[-1, 1\)"),
    (dict(variants=np.zeros(40)), "integer"),
    (dict(variants=np.arange(40) * 200), r"3 populations \(and their total\) x 7801 classes x 0 thresholds need 499264 bytes of records"),
    (dict(variants=np.arange(40) * 10, thresholds=range(7)), r"3 populations \(and their total\) x 391 classes x 7 thresholds need 68816 bytes"),
    (dict(thresholds=range(17)), "K = 17 thresholds: at most 16"),
    (dict(thresholds=[1.5]), "thresholds must be integers"),
    (dict(thresholds=[2 ** 31]), "integers in int32"),
    (dict(thresholds=[-2 ** 31 - 1]), "integers in int32"),
    (dict(thresholds=[[1, 2]]), "sequence of integers"),
    (dict(replicates=[0, 6]), "replicate index out of range"),
    (dict(replicates=[-1]), "replicate index out of range"),
    (dict(replicates=[1, 1]), "distinct"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(scenarios=2).milestones(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate"), (('tau', True), "direct chains only"), (('direct', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=r"milestones\(\).*" + text):
        bare_ensemble(last=last).milestones(thresholds=(10,))


def test_derived_properties_and_extinction_probability():
    from vgsim_amd.ensemble import Milestones
    ms = Milestones()
    ms.last_positive_event = np.array([[[3]], [[-2]], [[-1]], [[7]]], dtype=np.int32)   # 4 replicates, one cell
    ms.final = np.array([[[0]], [[0]], [[0]], [[2]]], dtype=np.int32)
    ms.replicates = np.array([5, 0, 2, 3])
    ms._R, ms._scenario_of, ms._n_scenarios = 6, np.arange(6) % 2, 2
    assert ms.extinct[:, 0, 0].tolist() == [True, False, True, False] and ms.never_present[:, 0, 0].tolist() == [False, True, False, False]
    assert ms.extinction_event[:, 0, 0].tolist() == [4, -1, 0, 8] and ms.extinction_event.dtype == np.int32
    assert ms.extinction_probability()[:, 0, 0].tolist() == [0.5, 0.5]               # scenario 0: replicates 0, 2; scenario 1: 5, 3
    assert ms.extinction_probability(by=np.zeros(6, dtype=np.int64))[:, 0, 0].tolist() == [0.5]
    assert np.isnan(ms.extinction_probability(by=np.array([0, 1, 0, 0, 1, 0]))[1, 0, 0])
    assert Milestones.NEVER == NEVER
