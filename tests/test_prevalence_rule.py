"""The prevalence rule of the device pass (vgsim_amd/csrc/vgx_prevalence.h: the signed cells a record changes, the cut /
interval rule, the walk of a tile, the running sum), compiled for the host and reached through vgx_test_prevalence: hand-made
chains, every record kind, every tile size, the CPU oracle's chains and their final states, against the literal restatement
below (never against the code under test), all with array_equal on integers; and the argument checks of Ensemble.prevalence,
which are raised before the library is called.  No GPU."""
import numpy as np
import pytest

from test_incidence_rule import ORACLE_CASES, bare_ensemble, chain_of, columns, oracle_model

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)


def cuts(times, grid):
    """cut[j] = first event index i with grid[j] < t_i (n if none), by the literal loop: `point` never goes back."""
    T, out, point = len(grid), [], 0
    for i, t in enumerate(times):
        while point < T and grid[point] < t:
            out.append(i)
            point += 1
    return out + [len(times)] * (T - len(out))


def deltas(rec, P, variant_of):
    """The (population, class, +1 / -1) changes of one record (type, haplotype, population, newHaplotype, newPopulation)."""
    t, hap, pop, nhap, npop = (int(v) for v in rec)

    def cls(h):
        return int(variant_of[h]) if 0 <= h < len(variant_of) else -1
    if t == BIRTH:
        got = [(pop, cls(hap), 1)]
    elif t in (DEATH, SAMPLING):
        got = [(pop, cls(hap), -1)]
    elif t == MUTATION:
        got = [] if cls(hap) == cls(nhap) else [(pop, cls(hap), -1), (pop, cls(nhap), 1)]
    elif t == MIGRATION:
        got = [(npop, cls(hap), 1)]
    else:
        got = []
    return [(p, c, d) for p, c, d in got if 0 <= p < P and c >= 0]


def restate(times, cols, P, grid, variant_of, V, start):
    """Section 1 of the feature's rule as a Python loop: (values [T, P, V] int64, final [P, V], outside [2])."""
    T, n = len(grid), len(times)
    cut = cuts(times, grid)
    bound = [0] + cut + [n]
    state = np.array(start, dtype=np.int64).reshape(P, V).copy()
    values = np.zeros((T, P, V), dtype=np.int64)
    for j in range(T + 1):
        for i in range(bound[j], bound[j + 1]):
            for p, c, d in deltas([col[i] for col in cols], P, variant_of):
                state[p, c] += d
        if j < T:
            values[j] = state
    return values, state, np.array([cut[0], n - cut[T - 1]], dtype=np.int64)


def fold(infectious, variant_of, V):
    """A state [P, H] folded through variant_of: [P, V]."""
    inf = np.asarray(infectious, dtype=np.int64)
    out = np.zeros((inf.shape[0], V), dtype=np.int64)
    for h, c in enumerate(variant_of):
        if c >= 0:
            out[:, c] += inf[:, h]
    return out


def hook(times, cols, P, H, grid, variant_of, V, start, tile=0):
    from vgsim_amd import _capi
    return _capi.replay_prevalence(times, *cols, P, H, grid, variant_of, V, start, tile)


def assert_hook_equals(times, cols, P, H, grid, variant_of, V, start, tile=0, what=""):
    got = hook(times, cols, P, H, grid, variant_of, V, start, tile)
    want = restate(times, cols, P, grid, variant_of, V, start)
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape and got[1].dtype == np.int32
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what
    return got


# ---- hand-made chains
def test_an_event_at_a_grid_time_is_applied_before_the_point():
    P, H = 2, 2
    vo, start = np.arange(H), np.array([[1, 0], [0, 0]])
    recs = columns([(BIRTH, 0, 0, 0, 0), (BIRTH, 1, 1, 0, 0), (DEATH, 0, 0, 0, 0), (BIRTH, 1, 0, 0, 0)])
    values, final, outside = assert_hook_equals([0.5, 1.0, 1.0, 1.5], recs, P, H, np.array([0.0, 1.0, 2.0]), vo, H, start)
    assert values.tolist() == [[[1, 0], [0, 0]],        # at 0.0: nothing has happened
                               [[1, 0], [0, 1]],        # at 1.0: the three events up to and AT t = 1.0
                               [[1, 1], [0, 1]]]
    assert final.tolist() == [[1, 1], [0, 1]] and outside.tolist() == [0, 0]


def test_empty_chain_one_point_the_window_and_times_that_go_back():
    P, H = 2, 2
    vo, start = np.arange(H), np.array([[3, 0], [0, 2]])
    values, final, outside = assert_hook_equals([], columns([]), P, H, np.array([0.0, 1.0]), vo, H, start)
    assert np.array_equal(values, [start, start]) and np.array_equal(final, start) and outside.tolist() == [0, 0]
    recs = columns([(BIRTH, 0, 0, 0, 0), (BIRTH, 0, 1, 0, 0), (DEATH, 1, 1, 0, 0), (BIRTH, 1, 1, 0, 0)])
    # T = 1
    values, final, outside = assert_hook_equals([0.0, 0.5, 0.999, 1.0], recs, P, H, np.array([0.5]), vo, H, start)
    assert values.tolist() == [[[4, 0], [1, 2]]] and final.tolist() == [[4, 0], [1, 2]] and outside.tolist() == [2, 2]
    # all events before grid[0]: every point sees the final state; all after grid[T - 1]: every point sees the start
    values, final, outside = assert_hook_equals([0.1, 0.2, 0.3, 0.4], recs, P, H, np.array([1.0, 2.0]), vo, H, start)
    assert np.array_equal(values, [final, final]) and outside.tolist() == [4, 0]
    values, final, outside = assert_hook_equals([3.1, 3.2, 3.3, 3.4], recs, P, H, np.array([1.0, 2.0]), vo, H, start)
    assert np.array_equal(values, [start, start]) and not np.array_equal(final, start) and outside.tolist() == [0, 4]
    # `point` never goes back: the event at t = 0.2 after one at t = 1.5 stays in the interval the loop had reached
    values, _, _ = assert_hook_equals([0.1, 1.5, 0.2, 2.5], recs, P, H, np.array([0.0, 1.0, 2.0, 3.0]), vo, H, start)
    assert values[:, :, :].sum(axis=(1, 2)).tolist() == [5, 6, 6, 7]
    # decreasing times
    assert_hook_equals([4.0, 3.0, 2.0, 1.0], recs, P, H, np.array([0.5, 1.5, 2.5, 3.5]), vo, H, start)
    for grid in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], [0.0, float("inf")], []):
        with pytest.raises(ValueError, match="grid|T = 0"):
            hook([0.1], columns([(BIRTH, 0, 0, 0, 0)]), P, H, np.array(grid), vo, H, start)


def test_every_record_kind():
    P, H, V = 3, 5, 3
    vo = np.array([0, 0, 1, 2, -1])                               # haplotypes 0 and 1 share class 0; 4 is not tracked
    start = np.full((P, V), 10)
    recs = [(BIRTH, 1, 0, 9, 9), (DEATH, 2, 1, 0, 0), (SAMPLING, 3, 2, 0, 0),
            (MUTATION, 0, 1, 1, 0),                               # within class 0: writes nothing
            (MUTATION, 0, 1, 2, 0),                               # class 0 -> 1 in population 1
            (MUTATION, 4, 2, 3, 0),                               # out of the untracked haplotype: +1 only
            (MUTATION, 3, 2, 4, 0),                               # into it: -1 only
            (MUTATION, 4, 0, 4, 0),                               # untracked on both sides
            (MIGRATION, 2, 0, 7, 2),                              # keyed by newPopulation: +1 at (2, class 1); the source stays
            (MIGRATION, 2, 7, 0, 1),                              # `population` is not a key: still +1 at (1, class 1)
            (MIGRATION, 2, 0, 0, 3), (MIGRATION, 2, 0, 0, -1),    # newPopulation outside [0, P)
            (SUSCCHANGE, 0, 0, 1, 0),
            (BIRTH, 4, 0, 0, 0), (BIRTH, 5, 0, 0, 0), (BIRTH, -1, 0, 0, 0), (DEATH, 0, 3, 0, 0), (DEATH, 0, -1, 0, 0),
            (MUTATION, 5, 0, 2, 0),                               # haplotype outside [0, H): that side counts nowhere
            (MUTATION, 0, 3, 2, 0),                               # population outside [0, P)
            (6, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (7, 1, 1, 1, 1)]
    times = np.arange(len(recs)) * 0.25
    grid = np.array([0.6, 2.0, 10.0])
    values, final, outside = assert_hook_equals(times, columns(recs), P, H, grid, vo, V, start)
    want = np.full((P, V), 10)
    want[0, 0] += 1; want[1, 1] -= 1; want[2, 2] -= 1             # the first three, t <= 0.5
    assert np.array_equal(values[0], want)
    want[1, 0] -= 1; want[1, 1] += 1                              # ... up to t = 2.0: the mutations and the first migration
    want[2, 2] += 1; want[2, 2] -= 1
    want[2, 1] += 1
    assert np.array_equal(values[1], want)
    want[1, 1] += 1                                               # the second migration
    want[0, 1] += 1                                               # MUTATION out of haplotype 5 into class 1
    assert np.array_equal(values[2], want) and np.array_equal(final, want)
    assert outside.tolist() == [3, 0]


def _long_chain(n=700, P=5, H=40):
    rng = np.random.default_rng(78)
    t = np.sort(np.where(rng.random(n) < 0.2, rng.uniform(0.0, 2.0, n), rng.uniform(3.0, 10.5, n)))   # nothing in [2, 3)
    t[0] = -0.5                                                  # one event before the grid, some after 10
    recs = np.stack([rng.integers(-1, 8, n), rng.integers(-1, H + 1, n), rng.integers(-1, P + 1, n), rng.integers(-1, H + 1, n),
                     rng.integers(-1, P + 1, n)], axis=1)
    return t, columns(recs), P, H


def test_every_tile_size_gives_the_same_block():
    t, cols, P, H = _long_chain()
    n = len(t)
    grid = np.arange(0.0, 11.0)
    cut = cuts(t, grid)
    assert cut[2] == cut[3]                                      # an interval of zero events
    assert sum(1 for c in cut if 257 <= c < 514) >= 3            # the tile [257, 514) spans four intervals at least
    classes = np.arange(H) % 4 - (np.arange(H) % 7 == 0)         # 4 classes, some haplotypes untracked
    for vo, V in ((np.arange(H), H), (classes, 4)):
        start = np.full((P, V), 1000)                            # (random records: far from zero)
        want = restate(t, cols, P, grid, vo, V, start)
        assert want[2][0] == 1 and want[2][1] > 0 and len(np.unique(want[0])) > 10
        for tile in (1, 7, 64, 257, n - 1, n, n + 1, 0):
            got = hook(t, cols, P, H, grid, vo, V, start, tile)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (V, tile)


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
    grid = np.linspace(0.05 * t[-1], 0.9 * t[-1], 9)
    # every haplotype its own class: the final block is the model's final state, and no population holds more than its size
    ident = np.arange(H)
    values, final, outside = hook(t, cols, P, H, grid, ident, H, m.initial_infectious, tile=257)
    assert np.array_equal(final, m.infectious)
    assert values.min() >= 0 and (values.sum(axis=2) <= np.asarray(m.sizes)[None, :]).all()
    assert outside.sum() < len(t) and not np.array_equal(values[0], values[-1])
    # three classes and one untracked haplotype, chosen among those the chain touches
    busy = np.bincount(cols[1][(cols[1] >= 0) & (cols[1] < H)], minlength=H).argsort()[::-1]
    vo = np.arange(H) % 3
    vo[busy[1]] = -1
    start = fold(m.initial_infectious, vo, 3)
    got = assert_hook_equals(t, cols, P, H, grid, vo, 3, start, tile=64, what=name)
    assert np.array_equal(got[1], fold(m.infectious, vo, 3))
    assert np.array_equal(got[0], fold_values(values, vo, 3))


def fold_values(values, variant_of, V):
    out = np.zeros(values.shape[:2] + (V,), dtype=np.int64)
    for h, c in enumerate(variant_of):
        if c >= 0:
            out[:, :, c] += values[:, :, h]
    return out


# ---- the hook's refusals
def test_the_hook_refuses_what_the_device_pass_refuses():
    one = columns([(BIRTH, 0, 0, 0, 0)])
    values, final, _ = hook([0.5], one, 1, 1, np.array([1.0]), np.array([16383]), 16384, np.zeros((1, 16384)))   # 65536 bytes fit
    assert values[0, 0, 16383] == 1 and values.sum() == 1 and final.sum() == 1
    with pytest.raises(ValueError, match="1 populations x 16385 classes need 65540 bytes"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 16385, np.zeros((1, 16385)))
    with pytest.raises(ValueError, match=r"variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook([0.5], one, 1, 2, np.array([1.0]), np.array([0, 2]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match=r"variant_of\[0\] = -2 is outside"):
        hook([0.5], one, 1, 2, np.array([1.0]), np.array([-2, 0]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match="V = 0"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([-1]), 0, np.zeros((1, 0)))
    with pytest.raises(ValueError, match="start value outside"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 1, np.array([[-1]]))
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 1, np.zeros((1, 1)), tile=-1)


# ---- Ensemble.prevalence: refusals before the library (popNum 3, hapNum 40, 6 replicates)
@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either times or points"),
    (dict(times=[0.0, 1.0], points=4, window=(0, 1)), "either times or points"),
    (dict(points=0, window=(0, 1)), "points must be at least 1"),
    (dict(points=4), "window"),
    (dict(points=4, window=(1.0, 1.0)), "increase strictly"),
    (dict(times=[0.0, 1.0, 1.0]), "grid must increase strictly"),
    (dict(times=[0.0, 2.0, 1.0]), "grid must increase strictly"),
    (dict(times=[]), "at least one"),
    (dict(times=[0.0, float("nan")]), "finite"),
    (dict(times=[float("inf")]), "finite"),
    (dict(points=4, window=(0.0, float("inf"))), "finite"),
    (dict(times=[0.0], variants=[[0, 1], [40]]), "haplotype index out of range"),
    (dict(times=[0.0], variants=[[0, 1], [-1]]), "haplotype index out of range"),
    (dict(times=[0.0], variants=[[0, 1], [2, 1]]), "listed twice"),
    (dict(times=[0.0], variants=[[0, 1, 1]]), "listed twice"),
    (dict(times=[0.0], variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(times=[0.0], variants=np.full(40, -2)), r"variant_of\[0\] = -2 is outside \[-1, 1\)"),
    (dict(times=[0.0], variants=np.zeros(40)), "integer"),
    (dict(times=[0.0], variants=np.arange(40) * 200), "3 populations x 7801 classes need 93612 bytes"),
    (dict(times=[0.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(times=[0.0], replicates=[-1]), "replicate index out of range"),
    (dict(times=[0.0], replicates=[1, 1]), "distinct"),
    (dict(times=[0.0], values=False), "values=False needs summary"),
    (dict(times=[0.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(times=[0.0], summary=dict(method='nearest')), "method must be"),
    (dict(times=[0.0], summary=dict(by='scenario')), "by must be 'auto'"),
    (dict(times=[0.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(scenarios=2).prevalence(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate"), (('tau', True), "direct chains only"), (('direct', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=r"prevalence\(\).*" + text):
        bare_ensemble(last=last).prevalence(times=[0.0, 1.0])


def test_points_and_window_form_the_trajectories_grid():
    from vgsim_amd.ensemble import _prevalence_grid
    t0, t1, points = 0.1, 0.7, 8
    g = _prevalence_grid(None, points, (t0, t1))
    dt = (t1 - t0) / (points - 1)
    assert g.dtype == np.float64 and g.tolist() == [t0 + j * dt for j in range(points)]
    assert _prevalence_grid(None, 1, (2.5, 9.0)).tolist() == [2.5]
    assert np.array_equal(_prevalence_grid([0, 1, 5], None, None), [0.0, 1.0, 5.0])


def test_variants_in_their_three_forms():
    from vgsim_amd import _capi
    vo, V = _capi.variant_map(None, 5)
    assert vo.dtype == np.int32 and vo.tolist() == [0, 1, 2, 3, 4] and V == 5
    vo, V = _capi.variant_map([-1, 2, 0, 0, -1], 5)
    assert vo.dtype == np.int32 and vo.tolist() == [-1, 2, 0, 0, -1] and V == 3
    vo, V = _capi.variant_map([[3, 1], [], [0]], 5)
    assert vo.tolist() == [2, 0, -1, 0, -1] and V == 3
    assert _capi.variant_map(np.full(5, -1), 5)[1] == 1


def test_share():
    from vgsim_amd.ensemble import Prevalence
    pv = Prevalence()
    pv.values = np.array([[[[1, 3], [0, 0]]]], dtype=np.int32)
    assert pv.share().tolist() == [[[[0.25, 0.75], [0.0, 0.0]]]] and pv.share().dtype == np.float64
