"""The incidence rule of the device pass (vgsim_amd/csrc/vgx_incidence.h: which cells a record counts in, the cut / bin rule,
the walk of a tile), compiled for the host and reached through vgx_test_incidence: hand-made chains, the haplotype filter,
every tile size, the CPU oracle's chains and the conservation of the infectious totals, against the literal restatement below
(never against the code under test), all with array_equal on integers; and the argument checks of Ensemble.incidence, which
are raised before the library is called.  No GPU."""
import numpy as np
import pytest

import helpers
import models

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
CHANNELS = 7


def cuts(times, edges):
    """cut[k] = first event index i with edges[k] <= t_i (n if none), by the literal loop: `point` never goes back."""
    T, out, point = len(edges) - 1, [], 0
    for i, t in enumerate(times):
        while point <= T and edges[point] <= t:
            out.append(i)
            point += 1
    return out + [len(times)] * (T + 1 - len(out))


def cells(rec, P, allowed):
    """The (population, channel) cells one record (type, haplotype, population, newHaplotype, newPopulation) counts in."""
    t, hap, pop, nhap, npop = (int(v) for v in rec)
    if t not in (BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION):
        return []
    if allowed is not None:
        if t == SUSCCHANGE:
            return []
        if (nhap if t == MUTATION else hap) not in allowed:
            return []
    got = [(npop, 5), (pop, 6)] if t == MIGRATION else [(pop, t)]
    return [(p, k) for p, k in got if 0 <= p < P]


def restate(times, cols, P, edges, haplotypes=None):
    """Section 1 of the feature's rule as a Python loop: (counts [T, P, 7] int64, outside [2])."""
    T, n = len(edges) - 1, len(times)
    cut = cuts(times, edges)
    allowed = None if haplotypes is None else {int(h) for h in haplotypes}
    counts = np.zeros((T, P, CHANNELS), dtype=np.int64)
    for b in range(T):
        for i in range(cut[b], cut[b + 1]):
            for p, k in cells([c[i] for c in cols], P, allowed):
                counts[b, p, k] += 1
    return counts, np.array([cut[0], n - cut[T]], dtype=np.int64)


def restate_sorted(times, cols, P, edges, haplotypes=None):
    """The same for a chain whose times do not decrease (asserted): searchsorted and np.add.at."""
    times = np.asarray(times, dtype=np.float64)
    assert np.all(np.diff(times) >= 0)
    T = len(edges) - 1
    typ, hap, pop, nhap, npop = (np.asarray(c, dtype=np.int64) for c in cols)
    b = np.searchsorted(edges, times, side='right') - 1
    inside = (b >= 0) & (b < T)
    ok = inside & (typ >= 0) & (typ <= 5)
    if haplotypes is not None:
        judged = np.where(typ == MUTATION, nhap, hap)
        ok &= (typ != SUSCCHANGE) & np.isin(judged, np.asarray(list(haplotypes), dtype=np.int64))
    counts = np.zeros((T, P, CHANNELS), dtype=np.int64)
    plain = ok & (typ != MIGRATION) & (pop >= 0) & (pop < P)
    np.add.at(counts, (b[plain], pop[plain], typ[plain]), 1)
    arr = ok & (typ == MIGRATION) & (npop >= 0) & (npop < P)
    np.add.at(counts, (b[arr], npop[arr], np.full(arr.sum(), 5)), 1)
    dep = ok & (typ == MIGRATION) & (pop >= 0) & (pop < P)
    np.add.at(counts, (b[dep], pop[dep], np.full(dep.sum(), 6)), 1)
    return counts, np.array([(b < 0).sum(), (b >= T).sum()], dtype=np.int64)


def hook(times, cols, P, hapNum, edges, haplotypes=None, tile=0):
    from vgsim_amd import _capi
    mask = None if haplotypes is None else _capi.haplotype_mask(list(haplotypes), hapNum)
    return _capi.replay_incidence(times, *cols, P, hapNum, edges, mask, tile)


def assert_hook_equals(times, cols, P, hapNum, edges, haplotypes=None, tile=0, what=""):
    got, out = hook(times, cols, P, hapNum, edges, haplotypes, tile)
    want, wout = restate(times, cols, P, edges, haplotypes)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), what
    assert np.array_equal(out, wout), what
    return got, out


def chain_of(m):
    ev, n = m.events, m.events.ptr
    return ev.times[:n].copy(), [getattr(ev, c)[:n].copy() for c in ("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")]


def columns(records):
    a = np.asarray(records, dtype=np.int64).reshape(-1, 5)
    return [np.ascontiguousarray(a[:, j]) for j in range(5)]


# ---- hand-made chains
def test_one_record_of_every_type_and_the_edges():
    P, H = 3, 4
    edges = np.array([1.0, 2.0, 2.5, 4.0])                      # non-uniform, T = 3
    recs = [(BIRTH, 1, 0, 0, 0), (DEATH, 1, 1, 0, 0), (SAMPLING, 2, 2, 0, 0), (MUTATION, 0, 1, 3, 0), (SUSCCHANGE, 0, 2, 1, 0),
            (MIGRATION, 2, 0, 0, 2),                              # arrival in 2, departure from 0
            (MIGRATION, 2, 1, 0, 3), (MIGRATION, 2, -1, 0, 1),    # one key outside [0, P) each: the other still counts
            (BIRTH, 0, 3, 0, 0), (DEATH, 0, -1, 0, 0), (6, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (7, 1, 1, 1, 1),   # count nowhere
            (BIRTH, 3, 2, 0, 0), (SAMPLING, 0, 0, 0, 0)]
    times = [0.5, 1.0, 1.5, 2.0, 2.0, 2.25, 2.5, 2.5, 2.75, 3.0, 3.0, 3.5, 3.5, 3.999, 4.0]   # before edges[0]; on edges 0, 1, 2; at edges[T]
    got, out = assert_hook_equals(times, columns(recs), P, H, edges)
    assert out.tolist() == [1, 1]
    want = np.zeros((3, P, CHANNELS), dtype=np.int64)
    want[0, 1, 1] = want[0, 2, 2] = 1                             # t = 1.0 lies in bin 0 (edges[0] <= t)
    want[1, 1, 3] = want[1, 2, 4] = want[1, 2, 5] = want[1, 0, 6] = 1   # t = 2.0 lies in bin 1
    want[2, 1, 6] = want[2, 1, 5] = want[2, 2, 0] = 1
    assert np.array_equal(got, want)


def test_empty_chain_one_bin_and_times_that_go_back():
    P, H = 2, 2
    none = columns([])
    got, out = assert_hook_equals([], none, P, H, np.array([0.0, 1.0]))
    assert got.shape == (1, P, CHANNELS) and not got.any() and out.tolist() == [0, 0]
    recs = columns([(BIRTH, 0, 0, 0, 0), (BIRTH, 0, 1, 0, 0), (DEATH, 1, 0, 0, 0), (BIRTH, 1, 1, 0, 0)])
    got, out = assert_hook_equals([0.0, 0.5, 0.999, 1.0], recs, P, H, np.array([0.0, 1.0]))   # T = 1
    assert got[0, :, 0].tolist() == [1, 1] and got[0, 0, 1] == 1 and out.tolist() == [0, 1]
    # `point` never goes back: the event at t = 0.2 after one at t = 1.5 stays in the bin the loop had reached
    got, out = assert_hook_equals([0.1, 1.5, 0.2, 2.5], recs, P, H, np.array([0.0, 1.0, 2.0, 3.0]))
    assert got[:, :, :2].sum(axis=(1, 2)).tolist() == [1, 2, 1]
    for edges in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], [0.0, float("inf")], [0.0]):
        with pytest.raises(ValueError, match="edges|T = 0"):
            hook([0.1], columns([(BIRTH, 0, 0, 0, 0)]), P, H, np.array(edges))


def test_filter_judges_the_right_haplotype():
    P, H = 2, 37                                                  # hapNum no multiple of 32: bit 36 is bit 4 of word 1
    recs = [(BIRTH, 36, 0, 0, 0), (BIRTH, 35, 0, 0, 0), (DEATH, 36, 1, 0, 0), (SAMPLING, 36, 1, 5, 0), (SAMPLING, 5, 1, 36, 0),
            (MUTATION, 36, 0, 5, 0),                              # out of 36 into 5: not counted under {36}
            (MUTATION, 5, 0, 36, 0),                              # the variant 36 arises: counted
            (SUSCCHANGE, 36, 0, 36, 0),                           # carries no haplotype: drops out under a filter
            (MIGRATION, 36, 0, 5, 1), (MIGRATION, 5, 0, 36, 1), (BIRTH, 37, 0, 0, 0), (BIRTH, -1, 0, 0, 0)]
    times = np.arange(len(recs)) * 0.1
    edges = np.array([0.0, 10.0])
    from vgsim_amd import _capi
    assert _capi.haplotype_mask([36], H).tolist() == [0, 16]
    got, _ = assert_hook_equals(times, columns(recs), P, H, edges, haplotypes=[36])
    want = np.zeros((1, P, CHANNELS), dtype=np.int64)
    want[0, 0, 0] = want[0, 1, 1] = want[0, 1, 2] = want[0, 0, 3] = want[0, 1, 5] = want[0, 0, 6] = 1
    assert np.array_equal(got, want)
    everything, _ = assert_hook_equals(times, columns(recs), P, H, edges)
    assert everything[0, 0, 4] == 1 and everything[0, 0, 0] == 4 and everything[0, 0, 3] == 2
    both, _ = assert_hook_equals(times, columns(recs), P, H, edges, haplotypes=[5, 36])
    assert both[0, 0, 3] == 2 and both[0, 0, 4] == 0
    nothing, _ = assert_hook_equals(times, columns(recs), P, H, edges, haplotypes=[])
    assert not nothing.any()


def _long_chain(n=700, P=5, H=40):
    rng = np.random.default_rng(77)
    t = np.sort(np.where(rng.random(n) < 0.2, rng.uniform(0.0, 2.0, n), rng.uniform(3.0, 10.5, n)))   # nothing in [2, 3)
    t[0] = -0.5                                                  # one event before the window, some after 10
    recs = np.stack([rng.integers(-1, 8, n), rng.integers(-1, H + 1, n), rng.integers(-1, P + 1, n), rng.integers(-1, H + 1, n),
                     rng.integers(-1, P + 1, n)], axis=1)
    return t, columns(recs), P, H


def test_every_tile_size_gives_the_same_counts():
    t, cols, P, H = _long_chain()
    n = len(t)
    edges = np.arange(0.0, 11.0)
    cut = cuts(t, edges)
    assert cut[2] == cut[3]                                      # a bin of zero events
    assert sum(1 for c in cut if 255 <= c < 510) >= 3            # the tile [255, 510) spans three bins at least
    want, wout = restate(t, cols, P, edges)
    assert np.array_equal(want, restate_sorted(t, cols, P, edges)[0]) and np.array_equal(wout, restate_sorted(t, cols, P, edges)[1])
    assert wout[0] == 1 and wout[1] > 0 and all(want[..., k].sum() > 0 for k in range(CHANNELS))
    for tile in (1, 2, 255, 256, 257, n, n + 1, 0):
        for hp in (None, range(0, H, 3)):
            assert_hook_equals(t, cols, P, H, edges, haplotypes=hp, tile=tile, what=("tile", tile))


# ---- the oracle's chains
ORACLE_CASES = ("g9_short", "stress_h64", "p70")


def oracle_model(oracle_mod, name, seed=None, n_max=3000, epidemic_time=-1):
    from vgsim_amd import Simulator
    ctor, phases = models.CASES[name]
    with helpers.quiet():
        sim = Simulator(**(ctor if seed is None else dict(ctor, seed=int(seed))))
        phases[0][0](sim)
    ph = phases[0][1]
    m = sim.simulation
    assert oracle_mod.run_direct(m, min(ph["iterations"], n_max), 10 ** 9, epidemic_time, ph.get("attempts", 200)) == 0
    return m


@pytest.fixture(scope="module")
def oracle_chains(oracle_mod):
    return {name: oracle_model(oracle_mod, name) for name in ORACLE_CASES}


def test_oracle_chains_equal_the_restatement(oracle_chains):
    seen = set()
    for name, m in oracle_chains.items():
        t, cols = chain_of(m)
        assert len(t) > 100
        seen |= set(np.unique(cols[0]).tolist())
        for T in (100, 7):
            edges = np.linspace(0.05 * t[-1], 0.9 * t[-1], T + 1)
            got, out = assert_hook_equals(t, cols, m.popNum, m.hapNum, edges, what=(name, T))
            fast = restate_sorted(t, cols, m.popNum, edges)
            assert np.array_equal(got, fast[0]) and np.array_equal(out, fast[1])
        # a window over the whole chain: every channel sums to the number of records of its type
        edges = np.array([0.0, 0.3 * t[-1], np.nextafter(t[-1], np.inf)])
        got, out = assert_hook_equals(t, cols, m.popNum, m.hapNum, edges, tile=257, what=name)
        assert out.tolist() == [0, 0]
        for k in range(5):
            assert got[..., k].sum() == (cols[0] == k).sum(), (name, k)
        assert got[..., 5].sum() == got[..., 6].sum() == (cols[0] == MIGRATION).sum()
        inner, out = hook(t, cols, m.popNum, m.hapNum, np.linspace(0.2 * t[-1], 0.6 * t[-1], 8))
        assert inner[..., :5].sum() + inner[..., 5].sum() + out.sum() == len(t)
        occupied = sorted({int(h) for h in np.argwhere(m.infectious > 0)[:, 1]})
        assert_hook_equals(t, cols, m.popNum, m.hapNum, np.linspace(0.0, t[-1], 11), haplotypes=occupied, what=(name, "filter"))
    assert seen == {BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION}   # every record type occurs in these cases


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_new_infections_minus_removals_give_the_final_totals(oracle_chains, name):
    """Births and arrivals add one infectious host to their population, deaths and samplings remove one; a mutation moves a host
    between haplotypes of one population and a departure leaves the source where it is: the totals do not see them."""
    m = oracle_chains[name]
    t, cols = chain_of(m)
    got, out = hook(t, cols, m.popNum, m.hapNum, np.array([0.0, 0.5 * t[-1], np.nextafter(t[-1], np.inf)]))
    assert out.tolist() == [0, 0] and (cols[0] == MUTATION).sum() > 0
    net = got.sum(axis=0).astype(np.int64)
    start = np.asarray(m.initial_infectious, dtype=np.int64).sum(axis=1)
    assert np.array_equal(start + net[:, 0] + net[:, 5] - net[:, 1] - net[:, 2], np.asarray(m.totalInfectious, dtype=np.int64))


def test_the_lds_budget_is_a_refusal_that_names_the_number():
    cols = columns([(BIRTH, 0, 2339, 0, 0)])
    got, _ = hook([0.5], cols, 2340, 1, np.array([0.0, 1.0]))   # 2340 * 28 = 65520 bytes fit
    assert got[0, 2339, 0] == 1 and got.sum() == 1
    with pytest.raises(ValueError, match="2341 populations need 65548 bytes"):
        hook([0.5], cols, 2341, 1, np.array([0.0, 1.0]))


# ---- Ensemble.incidence: refusals before the library
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


class _Shape:
    popNum, hapNum = 3, 40


def bare_ensemble(R=6, last=('direct', True), scenarios=None):
    from vgsim_amd import ensemble
    e = ensemble.Ensemble.__new__(ensemble.Ensemble)
    e.R, e.engine, e.model = R, _NoLibrary(), _Shape()
    e.scenarios = [object()] * scenarios if scenarios else None
    e.scenario_of = np.arange(R, dtype=np.int32) % scenarios if scenarios else None
    e._last_call = last
    return e


@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either edges or bins"),
    (dict(edges=[0.0, 1.0], bins=4, window=(0, 1)), "either edges or bins"),
    (dict(bins=0, window=(0, 1)), "bins must be at least 1"),
    (dict(bins=4), "window"),
    (dict(bins=4, window=(1.0, 1.0)), "increase strictly"),
    (dict(edges=[0.0, 1.0, 1.0]), "increase strictly"),
    (dict(edges=[0.0, 2.0, 1.0]), "increase strictly"),
    (dict(edges=[0.0]), "at least two"),
    (dict(edges=[0.0, float("nan")]), "finite"),
    (dict(edges=[0.0, float("inf")]), "finite"),
    (dict(bins=4, window=(0.0, float("inf"))), "finite"),
    (dict(edges=[0.0, 1.0], haplotypes=[40]), "haplotype index out of range"),
    (dict(edges=[0.0, 1.0], haplotypes=[-1]), "haplotype index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[-1]), "replicate index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[1, 1]), "distinct"),
    (dict(edges=[0.0, 1.0], counts=False), "counts=False needs summary"),
    (dict(edges=[0.0, 1.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(edges=[0.0, 1.0], summary=dict(method='nearest')), "method must be"),
    (dict(edges=[0.0, 1.0], summary=dict(by='scenario')), "by must be 'auto'"),
    (dict(edges=[0.0, 1.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(scenarios=2).incidence(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate"), (('tau', True), "direct chains only"), (('direct', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=last).incidence(edges=[0.0, 1.0])


def test_bins_and_window_form_the_edges():
    from vgsim_amd.ensemble import _incidence_edges
    e = _incidence_edges(None, 52, (0.0, 364.0))
    assert e.dtype == np.float64 and len(e) == 53 and e[0] == 0.0 and e[52] == 364.0 and e[1] == 7.0
    t0, t1, bins = 0.1, 0.7, 7
    e = _incidence_edges(None, bins, (t0, t1))
    assert e.tolist() == [t0 + (k * (t1 - t0)) / bins for k in range(bins)] + [t1]
    assert np.array_equal(_incidence_edges([0, 1, 5], None, None), [0.0, 1.0, 5.0])
