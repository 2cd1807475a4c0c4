"""The susceptible rule of the device pass (vgsim_amd/csrc/vgx_susceptible.h: the signed cells a record changes; cuts, tile walk
and running sum are vgx_prevalence.h's), compiled for the host and reached through vgx_test_susceptibles: hand-made chains, every
record kind, every tile size, the CPU oracle's chains with their final states and the conservation with replay_prevalence, against
the literal restatement below (never against the code under test), all with array_equal on integers; and the argument checks of
Ensemble.susceptibles, which are raised before the library is called.  No GPU."""
import os
import re

import numpy as np
import pytest

from test_incidence_rule import ORACLE_CASES, bare_ensemble, chain_of, columns, oracle_model
from test_prevalence_rule import cuts

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def deltas(rec, P, class_of):
    """The (population, class, +1 / -1) changes of one record (type, haplotype, population, newHaplotype, newPopulation)."""
    t, hap, pop, nhap, npop = (int(v) for v in rec)

    def cls(g):
        return int(class_of[g]) if 0 <= g < len(class_of) else -1
    if t == BIRTH:
        got = [(pop, cls(nhap), -1)]
    elif t in (DEATH, SAMPLING):
        got = [(pop, cls(nhap), 1)]
    elif t == SUSCCHANGE:
        got = [] if cls(hap) == cls(nhap) else [(pop, cls(nhap), 1), (pop, cls(hap), -1)]
    elif t == MIGRATION:
        got = [(npop, cls(nhap), -1)]
    else:
        got = []
    return [(p, c, d) for p, c, d in got if 0 <= p < P and c >= 0]


def restate(times, cols, P, grid, class_of, G, start):
    """Section 1 of the feature's rule as a Python loop: (values [T, P, G] int64, final [P, G], outside [2])."""
    T, n = len(grid), len(times)
    cut = cuts(times, grid)
    bound = [0] + cut + [n]
    state = np.array(start, dtype=np.int64).reshape(P, G).copy()
    values = np.zeros((T, P, G), dtype=np.int64)
    for j in range(T + 1):
        for i in range(bound[j], bound[j + 1]):
            for p, c, d in deltas([col[i] for col in cols], P, class_of):
                state[p, c] += d
        if j < T:
            values[j] = state
    return values, state, np.array([cut[0], n - cut[T - 1]], dtype=np.int64)


def fold(susceptible, class_of, G):
    """A state [P, S] folded through class_of: [P, G]."""
    sus = np.asarray(susceptible, dtype=np.int64)
    out = np.zeros((sus.shape[0], G), dtype=np.int64)
    for g, c in enumerate(class_of):
        if c >= 0:
            out[:, c] += sus[:, g]
    return out


def hook(times, cols, P, S, grid, class_of, G, start, tile=0):
    from vgsim_amd import _capi
    return _capi.replay_susceptibles(times, *cols, P, S, grid, class_of, G, start, tile)


def assert_hook_equals(times, cols, P, S, grid, class_of, G, start, tile=0, what=""):
    got = hook(times, cols, P, S, grid, class_of, G, start, tile)
    want = restate(times, cols, P, grid, class_of, G, start)
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape and got[1].dtype == np.int32
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what
    return got


# ---- hand-made chains
def test_an_event_at_a_grid_time_is_applied_before_the_point():
    P, S = 2, 2
    co, start = np.arange(S), np.array([[5, 0], [4, 0]])
    recs = columns([(BIRTH, 0, 0, 0, 0), (DEATH, 0, 1, 1, 0), (BIRTH, 0, 0, 0, 0), (SUSCCHANGE, 1, 1, 0, 0)])
    values, final, outside = assert_hook_equals([0.5, 1.0, 1.0, 1.5], recs, P, S, np.array([0.0, 1.0, 2.0]), co, S, start)
    assert values.tolist() == [[[5, 0], [4, 0]],        # at 0.0: nothing has happened
                               [[3, 0], [4, 1]],        # at 1.0: the three events up to and AT t = 1.0
                               [[3, 0], [5, 0]]]
    assert final.tolist() == [[3, 0], [5, 0]] and outside.tolist() == [0, 0]


def test_empty_chain_one_point_the_window_and_times_that_go_back():
    P, S = 2, 2
    co, start = np.arange(S), np.array([[30, 0], [0, 20]])
    values, final, outside = assert_hook_equals([], columns([]), P, S, np.array([0.0, 1.0]), co, S, start)
    assert np.array_equal(values, [start, start]) and np.array_equal(final, start) and outside.tolist() == [0, 0]
    recs = columns([(BIRTH, 0, 0, 0, 0), (BIRTH, 0, 1, 1, 0), (DEATH, 1, 1, 0, 0), (BIRTH, 1, 1, 1, 0)])
    # T = 1
    values, final, outside = assert_hook_equals([0.0, 0.5, 0.999, 1.0], recs, P, S, np.array([0.5]), co, S, start)
    assert values.tolist() == [[[29, 0], [0, 19]]] and final.tolist() == [[29, 0], [1, 18]] and outside.tolist() == [2, 2]
    # all events before grid[0]: every point sees the final state; all after grid[T - 1]: every point sees the start
    values, final, outside = assert_hook_equals([0.1, 0.2, 0.3, 0.4], recs, P, S, np.array([1.0, 2.0]), co, S, start)
    assert np.array_equal(values, [final, final]) and outside.tolist() == [4, 0]
    values, final, outside = assert_hook_equals([3.1, 3.2, 3.3, 3.4], recs, P, S, np.array([1.0, 2.0]), co, S, start)
    assert np.array_equal(values, [start, start]) and not np.array_equal(final, start) and outside.tolist() == [0, 4]
    # `point` never goes back: the event at t = 0.2 after one at t = 1.5 stays in the interval the loop had reached
    values, _, _ = assert_hook_equals([0.1, 1.5, 0.2, 2.5], recs, P, S, np.array([0.0, 1.0, 2.0, 3.0]), co, S, start)
    assert values.sum(axis=(1, 2)).tolist() == [50, 49, 49, 48]
    # decreasing times
    assert_hook_equals([4.0, 3.0, 2.0, 1.0], recs, P, S, np.array([0.5, 1.5, 2.5, 3.5]), co, S, start)
    for grid in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], [0.0, float("inf")], []):
        with pytest.raises(ValueError, match="grid|T = 0"):
            hook([0.1], columns([(BIRTH, 0, 0, 0, 0)]), P, S, np.array(grid), co, S, start)


def test_every_record_kind():
    P, S, G = 3, 5, 3
    co = np.array([0, 0, 1, 2, -1])                               # groups 0 and 1 share class 0; 4 is not tracked
    start = np.full((P, G), 10)
    recs = [(BIRTH, 9, 0, 1, 9), (DEATH, 9, 1, 2, 0), (SAMPLING, 9, 2, 3, 0),   # the group is newHaplotype; `haplotype` is no key
            (SUSCCHANGE, 0, 1, 1, 0),                             # within class 0: writes nothing
            (SUSCCHANGE, 0, 1, 2, 0),                             # class 0 -> 1 in population 1
            (SUSCCHANGE, 4, 2, 3, 0),                             # out of the untracked group: +1 only
            (SUSCCHANGE, 3, 2, 4, 0),                             # into it: -1 only
            (SUSCCHANGE, 4, 0, 4, 0),                             # untracked on both sides
            (MIGRATION, 7, 0, 2, 2),                              # keyed by newPopulation: -1 at (2, class 1)
            (MIGRATION, 0, 7, 2, 1),                              # `population` is not a key: still -1 at (1, class 1)
            (MIGRATION, 0, 0, 2, 3), (MIGRATION, 0, 0, 2, -1),    # newPopulation outside [0, P)
            (MUTATION, 0, 0, 1, 0), (MUTATION, 2, 1, 3, 0),       # nothing
            (BIRTH, 0, 0, 4, 0), (BIRTH, 0, 0, 5, 0), (BIRTH, 0, 0, -1, 0), (DEATH, 0, 3, 0, 0), (DEATH, 0, -1, 0, 0),
            (SUSCCHANGE, 5, 0, 2, 0),                             # source group outside [0, S): that side counts nowhere
            (SUSCCHANGE, 0, 3, 2, 0),                             # population outside [0, P)
            (6, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (7, 1, 1, 1, 1)]
    times = np.arange(len(recs)) * 0.25
    grid = np.array([0.6, 2.0, 10.0])
    values, final, outside = assert_hook_equals(times, columns(recs), P, S, grid, co, G, start)
    want = np.full((P, G), 10)
    want[0, 0] -= 1; want[1, 1] += 1; want[2, 2] += 1             # the first three, t <= 0.5
    assert np.array_equal(values[0], want)
    want[1, 0] -= 1; want[1, 1] += 1                              # ... up to t = 2.0: the immunity changes and the first migration
    want[2, 2] += 1; want[2, 2] -= 1
    want[2, 1] -= 1
    assert np.array_equal(values[1], want)
    want[1, 1] -= 1                                               # the second migration
    want[0, 1] += 1                                               # SUSCCHANGE out of group 5 into class 1
    assert np.array_equal(values[2], want) and np.array_equal(final, want)
    assert outside.tolist() == [3, 0]


def _long_chain(n=700, P=5, S=12):
    rng = np.random.default_rng(78)
    t = np.sort(np.where(rng.random(n) < 0.2, rng.uniform(0.0, 2.0, n), rng.uniform(3.0, 10.5, n)))   # nothing in [2, 3)
    t[0] = -0.5                                                  # one event before the grid, some after 10
    recs = np.stack([rng.integers(-1, 8, n), rng.integers(-1, S + 1, n), rng.integers(-1, P + 1, n), rng.integers(-1, S + 1, n),
                     rng.integers(-1, P + 1, n)], axis=1)
    return t, columns(recs), P, S


def test_every_tile_size_gives_the_same_block():
    t, cols, P, S = _long_chain()
    n = len(t)
    grid = np.arange(0.0, 11.0)
    cut = cuts(t, grid)
    assert cut[2] == cut[3]                                      # an interval of zero events
    assert sum(1 for c in cut if 257 <= c < 514) >= 3            # the tile [257, 514) spans four intervals at least
    classes = np.arange(S) % 4 - (np.arange(S) % 7 == 0)         # 4 classes, some groups untracked
    for co, G in ((np.arange(S), S), (classes, 4)):
        start = np.full((P, G), 1000)                            # (random records: far from zero)
        want = restate(t, cols, P, grid, co, G, start)
        assert want[2][0] == 1 and want[2][1] > 0 and len(np.unique(want[0])) > 10
        for tile in (1, 7, 64, 257, n - 1, n, n + 1, 0):
            got = hook(t, cols, P, S, grid, co, G, start, tile)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (G, tile)


# ---- the oracle's chains
@pytest.fixture(scope="module")
def oracle_chains(oracle_mod):
    return {name: oracle_model(oracle_mod, name) for name in ORACLE_CASES}


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_chains(oracle_chains, name):
    from vgsim_amd import _capi
    m = oracle_chains[name]
    t, cols = chain_of(m)
    P, H, S = m.popNum, m.hapNum, m.susNum
    assert len(t) > 100
    assert (cols[0] == SUSCCHANGE).sum() >= 10 and (cols[0] == MIGRATION).sum() >= 20
    grid = np.linspace(0.05 * t[-1], 0.9 * t[-1], 9)
    # every group its own class: the final block is the model's final state, and nothing goes below zero
    ident = np.arange(S)
    values, final, outside = assert_hook_equals(t, cols, P, S, grid, ident, S, m.initial_susceptible, tile=257, what=name)
    assert np.array_equal(final, m.susceptible)
    assert values.min() >= 0
    assert outside.sum() < len(t) and not np.array_equal(values[0], values[-1])
    # with the infectious half of the same chain on the same grid: nobody is lost or made
    inf, inf_final, inf_outside = _capi.replay_prevalence(t, *cols, P, H, grid, np.arange(H), H, m.initial_infectious, 257)
    sizes = np.asarray(m.sizes, dtype=np.int64)
    assert np.array_equal(outside, inf_outside)
    assert np.array_equal(values.sum(axis=2, dtype=np.int64) + inf.sum(axis=2, dtype=np.int64), np.broadcast_to(sizes, (len(grid), P)))
    assert np.array_equal(final.sum(axis=1, dtype=np.int64) + inf_final.sum(axis=1, dtype=np.int64), sizes)
    # two classes and one untracked group
    if S >= 2:
        co = np.arange(S) % 2
        co[S - 1] = -1
        got = assert_hook_equals(t, cols, P, S, grid, co, 2, fold(m.initial_susceptible, co, 2), tile=64, what=name)
        assert np.array_equal(got[1], fold(m.susceptible, co, 2))


# ---- the hook's refusals
def test_the_hook_refuses_what_the_device_pass_refuses():
    one = columns([(DEATH, 0, 0, 0, 0)])
    values, final, _ = hook([0.5], one, 1, 1, np.array([1.0]), np.array([16383]), 16384, np.zeros((1, 16384)))   # 65536 bytes fit
    assert values[0, 0, 16383] == 1 and values.sum() == 1 and final.sum() == 1
    with pytest.raises(ValueError, match="vgx_test_susceptibles: 1 populations x 16385 classes need 65540 bytes"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 16385, np.zeros((1, 16385)))
    with pytest.raises(ValueError, match=r"class_of\[1\] = 2 is outside \[-1, 2\)"):
        hook([0.5], one, 1, 2, np.array([1.0]), np.array([0, 2]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match=r"class_of\[0\] = -2 is outside"):
        hook([0.5], one, 1, 2, np.array([1.0]), np.array([-2, 0]), 2, np.zeros((1, 2)))
    with pytest.raises(ValueError, match="G = 0"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([-1]), 0, np.zeros((1, 0)))
    with pytest.raises(ValueError, match="start value outside"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 1, np.array([[-1]]))
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook([0.5], one, 1, 1, np.array([1.0]), np.array([0]), 1, np.zeros((1, 1)), tile=-1)
    with pytest.raises(ValueError, match="log value outside 32 bits"):
        hook([0.5], columns([(DEATH, 0, 0, 1 << 40, 0)]), 1, 1, np.array([1.0]), np.array([0]), 1, np.zeros((1, 1)))


# ---- Ensemble.susceptibles / tau_susceptibles: refusals before the library (popNum 3, susNum 5, 6 replicates)
def bare(last=('direct', True), scenarios=None):
    ens = bare_ensemble(last=last, scenarios=scenarios)

    class Shape:
        popNum, hapNum, susNum = 3, 40, 5
    ens.model = Shape()
    return ens


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
    (dict(times=[0.0], groups=[[0, 1], [5]]), "susceptibility group index out of range"),
    (dict(times=[0.0], groups=[[0, 1], [-1]]), "susceptibility group index out of range"),
    (dict(times=[0.0], groups=[[0, 1], [2, 1]]), "listed twice"),
    (dict(times=[0.0], groups=[[0, 1, 1]]), "listed twice"),
    (dict(times=[0.0], groups=np.zeros(4, dtype=np.int64)), "one class per susceptibility group"),
    (dict(times=[0.0], groups=np.full(5, -2)), r"class_of\[0\] = -2 is outside \[-1, 1\)"),
    (dict(times=[0.0], groups=np.zeros(5)), "integer"),
    (dict(times=[0.0], groups=np.arange(5) * 2000), "3 populations x 8001 classes need 96012 bytes"),
    (dict(times=[0.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(times=[0.0], replicates=[1, 1]), "distinct"),
    (dict(times=[0.0], values=False), "values=False needs summary"),
    (dict(times=[0.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(times=[0.0], summary=dict(by='scenario')), "by must be 'auto'"),
    (dict(times=[0.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare(scenarios=2).susceptibles(**kwargs)
    with pytest.raises(ValueError, match=text.replace("96012", "192024")):
        bare(last=('tau', True)).tau_susceptibles(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate"), (('tau', True), "direct chains only"), (('direct', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=r"^susceptibles\(\).*" + text):
        bare(last=last).susceptibles(times=[0.0, 1.0])


@pytest.mark.parametrize("last, text", [(None, "simulate_tau"), (('direct', True), "tau chains only"), (('tau', False), "record_events")])
def test_the_wrong_last_call_is_refused_for_tau(last, text):
    with pytest.raises(ValueError, match=r"^tau_susceptibles\(\).*" + text):
        bare(last=last).tau_susceptibles(times=[0.0, 1.0])


def test_groups_in_their_three_forms():
    from vgsim_amd import _capi
    co, G = _capi.group_map(None, 5)
    assert co.dtype == np.int32 and co.tolist() == [0, 1, 2, 3, 4] and G == 5
    co, G = _capi.group_map([-1, 2, 0, 0, -1], 5)
    assert co.dtype == np.int32 and co.tolist() == [-1, 2, 0, 0, -1] and G == 3
    co, G = _capi.group_map([[3, 1], [], [0]], 5)
    assert co.tolist() == [2, 0, -1, 0, -1] and G == 3
    assert _capi.group_map(np.full(5, -1), 5)[1] == 1


def test_share():
    from vgsim_amd.ensemble import Susceptibles
    sv = Susceptibles()
    sv.values = np.array([[[[1, 3], [0, 0]]]], dtype=np.int32)
    assert sv.share().tolist() == [[[[0.25, 0.75], [0.0, 0.0]]]] and sv.share().dtype == np.float64


def test_struct_layouts_match_the_header():
    """Field order of the ctypes mirrors of the new structures == field order in include/vgx.h."""
    from vgsim_amd import _capi
    src = open(os.path.join(ROOT, "include", "vgx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for cname, ctype, like in (("vgx_susceptibles_io", _capi.VgxSusceptiblesIO, _capi.VgxPrevalenceIO),
                               ("vgx_tau_susceptibles_io", _capi.VgxTauSusceptiblesIO, _capi.VgxTauPrevalenceIO),
                               ("vgx_tau_susceptibles_chain", _capi.VgxTauSusceptiblesChain, _capi.VgxTauPrevalenceChain)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = re.sub(r"^(const\s+)?(double|int64_t|int32_t|vgx_traj_summary_io)\s*", "", decl.strip())
            names += [re.sub(r"[\s\*]|\[.*\]", "", part) for part in decl.split(",") if decl]
        assert names == [f[0] for f in ctype._fields_], cname
        # the layout of the prevalence structure it mirrors, field by field
        assert [f[1] for f in ctype._fields_] == [f[1] for f in like._fields_], cname
        rename = {"G": "V", "class_of": "variant_of", "susNum": "hapNum"}
        assert [rename.get(f[0], f[0]) for f in ctype._fields_] == [f[0] for f in like._fields_], cname
