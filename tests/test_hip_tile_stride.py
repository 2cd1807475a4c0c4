"""The tiled log replays past the cap of their launch grids.  Every replay gives a chain one workgroup row per tile, at most 65535
rows; beyond that a workgroup walks several tiles in a stride loop (`for (t0 = blockIdx.y * tile; t0 < n; t0 += gridDim.y * tile)`).
At the default tiles that loop starts at some 10^8 events per chain; at a tile of 1 (every tile size but the pack kernel's has an
environment switch) it starts at 65536 events, records or rows, which the chains below hold: a workgroup then takes tile y in
the head of the chain and tile y + 65535 in its tail, and every grid has borders in both, so that the two tiles lie in different
intervals and the workgroup must flush and clear between them.

Expected values never come from the code under test: they are the literal restatements of the rules the sibling GPU tests use
(test_*_rule.py through the want_block / want_rows helpers of test_hip_*.py) on replicate_events() and replicate_state(), and the
host replay of the lineage walk (test_hip_lineages._host_row).  Every comparison is array_equal on integers (milestone times: NaN
at the same places, array_equal elsewhere), and every result must also equal the same call at the default tile, the path the
rest of the suite pins.  Every test asserts its own precondition first: chain, record or row count above 65535, no restart, and a
border inside the head and inside the tail of every chain.

Not reached here: the pack kernel of vgx_timelines.hip (its tile is a compile-time 4096: 2.7 * 10^8 events).  Of the tau replays
both chains stride: the prefix (the model's history before the call, walked once by the same launcher and kernel) and every
replicate's own rows; but for tau_milestones(), whose tiles never split a step: there the prefix alone strides.

The last test is apart from the stride: lineages() on what every direct kernel leaves behind (it reads the final occupancy lists
and converts the 4-byte counts of the FAST and long-list kernels itself)."""
import types

import numpy as np
import pytest

import helpers
import models
import test_hip_flows as hip_flows
import test_hip_incidence as hip_incidence
import test_hip_milestones as hip_milestones
import test_hip_prevalence as hip_prevalence
import test_hip_susceptibles as hip_susceptibles
import test_hip_tau_flows as tau_flows
import test_hip_tau_incidence as tau_incidence
import test_hip_tau_milestones as tau_milestones
import test_hip_tau_prevalence as tau_prevalence
import test_hip_tau_susceptibles as tau_susceptibles
from test_flows_rule import variant_maps
from test_hip_ensemble_genealogy import _ensemble
from test_hip_ensemble_tau_timelines import SEEDS
from test_hip_incidence import event_chain
from test_hip_lineages import _grid, _host_row, _three, assert_rows_equal_host
from test_hip_param_sets import ATTEMPTS, base_sim
from test_hip_prevalence import H, IDENT, P, THREE
from test_hip_susceptibles import ONE, S
from test_milestones_rule import INT_FIELDS, NEVER, TIME_FIELDS
from test_tau_susceptibles_rule import maps_of

pytestmark = pytest.mark.gpu

CAP = 65535                                   # workgroup rows of a launch: a chain of more tiles strides
MARGIN = 300
N = CAP + MARGIN
DIRECT_SEEDS = (1002, 1004)                   # seeds whose first attempt survives (every test asserts that nothing restarted)
THRESHOLDS = (3, 100)                         # 3 is first reached within the first 300 events, 100 by some cell only in the second half
IDENT_S = np.arange(S, dtype=np.int64)
TILE_SWITCHES = ("VGX_INCIDENCE_TILE_EVENTS", "VGX_FLOWS_TILE_EVENTS", "VGX_PREVALENCE_TILE_EVENTS", "VGX_MILESTONES_TILE_EVENTS",
                 "VGX_LINEAGES_TILE_RECORDS", "VGX_TAU_MILESTONES_TILE_ROWS", "VGX_FLOWS_FORM", "VGX_MILESTONES_WAVES", "VGX_TAU_MILESTONES_WAVES")


@pytest.fixture(autouse=True)
def default_tiles(monkeypatch):
    for name in TILE_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def long_sim():
    """The family of test_hip_param_sets.py (3 populations with migration, 16 haplotypes with mutation, 2 susceptibility groups
    with immunity loss, lockdowns) with 20000 hosts per population: an epidemic of some hundreds of infectious hosts per population
    that neither dies out nor saturates within 65835 events."""
    sim = base_sim()
    sim.set_population_size(20000)
    return sim


def tiles_of(n, tile=1):
    return -(-int(n) // tile)


def common_grid(all_times):
    """One grid for all chains: of every chain a point exactly at an event time and one between two events inside its first 300
    events, two points in its middle, and two inside its last 300 events."""
    points = set()
    for t in all_times:
        n = len(t)
        points |= {float(t[150]), 0.5 * float(t[220] + t[221]), float(t[n // 3]), 0.5 * float(t[n // 2] + t[n // 2 + 1]),
                   0.5 * float(t[n - 150] + t[n - 149]), float(t[n - 60])}
    grid = np.array(sorted(points))
    assert (np.diff(grid) > 0).all()
    return grid


def assert_cuts_in_head_and_tail(cut, n):
    """`cut`: the positions (in tiles of one) at which a chain of n tiles changes its interval.  One lies strictly inside the head
    (the tiles y that have a partner y + 65535: with n = 65535 + 300 the first 300) and one strictly inside the tail (the partners:
    the last n - 65535), so that a workgroup's two tiles lie in different intervals and the tail itself is cut."""
    cut = np.asarray(cut)
    assert tiles_of(n) > CAP
    assert ((cut > 0) & (cut < n - CAP)).any() and ((cut > CAP) & (cut < n)).any(), (n, cut)


def assert_borders_in_head_and_tail(times, grid):
    """Borders of `grid` inside the head and the tail of a chain of one-row events, by either cut rule (grid < t, grid <= t); and
    one grid point exactly at an event time."""
    times = np.asarray(times, dtype=np.float64)
    for side in ("left", "right"):
        assert_cuts_in_head_and_tail(np.searchsorted(times, grid, side=side), len(times))
    assert np.isin(grid, times).any()


# ---- 1. direct consumers
@pytest.fixture(scope="module")
def direct():
    """The long direct ensemble, run once; shared and never changed."""
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(long_sim(), 2, seeds=np.array(DIRECT_SEEDS, dtype=np.int64))
    assert (ens.model.popNum, ens.model.hapNum, ens.model.susNum) == (P, H, S)
    with helpers.quiet():
        res = ens.simulate(N, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
    chains = [event_chain(ens, r) for r in range(2)]
    d = types.SimpleNamespace(ens=ens, res=res, chains=chains, grid=common_grid([t for t, _ in chains]))
    yield d
    ens.close()


def assert_reached(d):
    """What every test of part 1 rests on: no restart, chains of N events, more tiles of one event than a launch has rows, and
    borders in the head and the tail of both chains; all kinds of records occur."""
    assert not d.res.restarts.any() and [int(n) for n in d.res.events] == [N, N]
    for t, cols in d.chains:
        assert len(t) == N and tiles_of(len(t)) > CAP
        assert_borders_in_head_and_tail(t, d.grid)
        assert (np.bincount(cols[0], minlength=6)[:6] > 100).all()      # births, deaths, samplings, mutations, immunity changes, migrations


def test_direct_incidence(direct, monkeypatch):
    assert_reached(direct)
    ens, edges = direct.ens, direct.grid
    counts, outside = hip_incidence.want_block(ens, range(2), edges)
    assert counts[:, 0].any() and counts[:, -1].any() and outside.any(axis=0).all()
    whole = ens.incidence(edges=edges)
    monkeypatch.setenv("VGX_INCIDENCE_TILE_EVENTS", "1")
    one = ens.incidence(edges=edges)
    hip_incidence.assert_equals(one, counts, outside, "tile 1")
    hip_incidence.assert_equals(whole, counts, outside, "default tile")


def test_direct_flows_in_both_forms(direct, monkeypatch):
    assert_reached(direct)
    ens, edges = direct.ens, direct.grid
    vo, V = variant_maps(H)["own"]
    counts, outside = hip_flows.want_block(ens, range(2), edges, vo, V)
    assert counts[:, 0].any() and counts[:, -1].any() and counts.sum() > np.einsum('rbppc->', counts) > 0     # births and arrivals
    whole = ens.flows(edges=edges)
    assert whole.form == "dense"
    hip_flows.assert_equals(whole, counts, outside, "default tile")
    monkeypatch.setenv("VGX_FLOWS_TILE_EVENTS", "1")
    for form in ("dense", "split"):
        monkeypatch.setenv("VGX_FLOWS_FORM", form)
        fl = ens.flows(edges=edges)
        assert fl.form == form
        hip_flows.assert_equals(fl, counts, outside, ("tile 1", form))
    assert hip_flows.no_mismatches(ens)


@pytest.mark.parametrize("key", ["identity", "three"])
def test_direct_prevalence(direct, monkeypatch, key):
    assert_reached(direct)
    ens, grid = direct.ens, direct.grid
    variant_of, V, variants = {"identity": (IDENT, H, None), "three": (THREE, 3, THREE)}[key]
    want = hip_prevalence.want_rows(ens, range(2), grid, variant_of, V)
    assert len(np.unique(want[0])) > 10 and want[2].any(axis=0).all()
    whole = ens.prevalence(times=grid, variants=variants)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "1")
    one = ens.prevalence(times=grid, variants=variants)
    hip_prevalence.assert_equals(one, want, "tile 1")
    hip_prevalence.assert_equals(whole, want, "default tile")


@pytest.mark.parametrize("key", ["identity", "one"])
def test_direct_susceptibles(direct, monkeypatch, key):
    """(The maps of susceptibles() are over the susceptibility groups: the identity, and group 1 not tracked.)"""
    assert_reached(direct)
    ens, grid = direct.ens, direct.grid
    class_of, G, groups = {"identity": (IDENT_S, S, None), "one": (ONE, 1, ONE)}[key]
    want = hip_susceptibles.want_rows(ens, range(2), grid, class_of, G)
    assert len(np.unique(want[0])) > 10 and want[2].any(axis=0).all()
    whole = ens.susceptibles(times=grid, groups=groups)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "1")
    one = ens.susceptibles(times=grid, groups=groups)
    hip_susceptibles.assert_equals(one, want, "tile 1")
    hip_susceptibles.assert_equals(whole, want, "default tile")


def milestone_rows(ms):
    return {k: getattr(ms, k) for k in INT_FIELDS + TIME_FIELDS + ("extinct", "reached", "never_present")}


MILESTONE_MAPS = {"identity": (IDENT, H, None), "three": (THREE, 3, THREE)}


@pytest.fixture(scope="module")
def direct_milestone_rows(direct):
    """The restatement of the milestones per map, formed once for the two workgroup shapes; shared and never changed."""
    return {key: hip_milestones.want_rows(direct.ens, range(2), vo, V, THRESHOLDS) for key, (vo, V, _) in MILESTONE_MAPS.items()}


@pytest.mark.parametrize("waves", [None, "4"])
@pytest.mark.parametrize("key", ["identity", "three"])
def test_direct_milestones(direct, direct_milestone_rows, monkeypatch, key, waves):
    assert_reached(direct)
    ens = direct.ens
    variant_of, V, variants = MILESTONE_MAPS[key]
    want = direct_milestone_rows[key]
    first = want["first_event"]
    for r in range(2):
        assert ((first[r, 0] >= 0) & (first[r, 0] < MARGIN)).any(), "no cell reaches %d within the first %d events" % (THRESHOLDS[0], MARGIN)
        assert ((first[r, 1] >= N // 2) & (first[r, 1] != NEVER)).any(), "no cell reaches %d only in the second half" % THRESHOLDS[1]
        assert (want["last_positive_event"][r] >= CAP).any() and len(np.unique(want["peak_event"][r])) > 5
    whole = ens.milestones(variants=variants, thresholds=THRESHOLDS)
    if waves is not None:
        monkeypatch.setenv("VGX_MILESTONES_WAVES", waves)
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "1")
    one = ens.milestones(variants=variants, thresholds=THRESHOLDS)
    hip_milestones.assert_equals(one, want, ("tile 1", waves))
    hip_milestones.assert_equals(whole, want, "default tile")
    hip_milestones.assert_equals(one, milestone_rows(whole), "tile 1 against the default tile")


@pytest.mark.parametrize("n", [CAP, CAP + 1])
def test_prevalence_at_the_caps_border(monkeypatch, n):
    """Chains of exactly 65535 events (as many tiles of one event as a launch has rows: no stride) and of 65536 (one workgroup
    with a second tile)."""
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(long_sim(), 2, seeds=np.array(DIRECT_SEEDS, dtype=np.int64))
    try:
        with helpers.quiet():
            res = ens.simulate(n, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
        assert not res.restarts.any() and [int(k) for k in res.events] == [n, n] and (tiles_of(n) > CAP) == (n == CAP + 1)
        times = [event_chain(ens, r)[0] for r in range(2)]
        grid = np.array(sorted({float(t[k]) for t in times for k in (0, 1, n // 2, n - 2, n - 1)} | {0.5 * float(t[0]) for t in times}))
        for t in times:                                                   # a border at the first and at the last event of every chain
            cut = np.searchsorted(t, grid, side="right")
            assert (cut == 1).any() and (cut == n - 1).any() and (np.searchsorted(t, grid, side="left") == n - 1).any()
        want = hip_prevalence.want_rows(ens, range(2), grid, THREE, 3)
        whole = ens.prevalence(times=grid, variants=THREE)
        monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "1")
        one = ens.prevalence(times=grid, variants=THREE)
        hip_prevalence.assert_equals(one, want, "tile 1")
        hip_prevalence.assert_equals(whole, want, "default tile")
    finally:
        ens.close()


# ---- 2. lineages
LINEAGE_EVENTS, LINEAGE_SEEDS, WALK_SEED = 130000, (1001, 1002), 4711


def lineage_sim():
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=2, populations_number=3, number_of_susceptible_groups=2, seed=1)
    sim.set_transmission_rate(2.5); sim.set_recovery_rate(0.2); sim.set_sampling_rate(1.0)
    sim.set_population_size(100000); sim.set_migration_probability(0.1); sim.set_mutation_rate(0.5)
    sim.set_susceptibility_type(1); sim.set_susceptibility(0.3, susceptibility_type=1)
    sim.set_immunity_transition(0.05, source=1, target=0)
    return sim


def assert_lineage_borders(times, types, grid, host):
    """The lineage log lies in descending event order with at most one record per event, and every sampling is a record (a leaf).
    Its head, the first records - 65535 records, are the tiles y with a partner y + 65535; the partners are its tail, the last
    records - 65535.  `host`: the host replay under the identity map (status 0: it did not raise).
    Head: behind some border lie fewer events than the head has records, one of them a sampling: the log changes its interval
    strictly inside the head.  Tail: up to some border lie fewer events than the tail has records, and at that border the host
    counts two lineages or more, which coalesce in a birth before it: the log changes its interval strictly inside the tail."""
    n, head = len(times), int(host["records"]) - CAP
    assert head > 256 and tiles_of(host["records"]) > CAP
    upto = np.searchsorted(times, grid, side="right")                 # events up to and at every grid time
    samplings_behind = np.array([(types[k:] == 2).sum() for k in upto])
    assert ((samplings_behind >= 1) & (n - upto < head)).any(), (head, n - upto, samplings_behind)
    alive = host["values"].reshape(len(grid), -1).sum(axis=1)
    assert ((alive >= 2) & (upto < head)).any(), (head, upto, alive)
    assert host["values"][0].any() and len(np.unique(host["values"])) > 10


def test_lineages_past_the_cap(monkeypatch):
    """Lineage tiles count records (2 sCounter - 1 plus the mutations and migrations the walk takes), not events.  The model: 3
    populations of 100000 hosts, 16 haplotypes, transmission 2.5, recovery 0.2, sampling 1.0, mutation 0.5 per site, migration
    0.1, 130000 events.  On the CPU (the oracle's chains through _capi.replay_lineages, walk seed 4711) seed 1001 gave sCounter
    29011 and 77589 records, seed 1002 sCounter 28780 and 77280 records, both walks with status 0 and neither run restarted."""
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(lineage_sim(), 2, seeds=np.array(LINEAGE_SEEDS, dtype=np.int64))
    try:
        with helpers.quiet():
            res = ens.simulate(LINEAGE_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
        assert not res.restarts.any() and [int(n) for n in res.events] == [LINEAGE_EVENTS] * 2
        chains = [event_chain(ens, r) for r in range(2)]
        grid = common_grid([t for t, _ in chains])
        H_ = ens.model.hapNum
        ident = np.arange(H_, dtype=np.int32)
        for r, (t, cols) in enumerate(chains):                        # (replicate 0 must be healthy: its replay does not raise)
            try:
                host = _host_row(ens, r, WALK_SEED, grid, ident, H_)
            except ValueError:
                assert r > 0
                continue
            assert host["records"] > CAP + 256
            assert_lineage_borders(t, cols[0], grid, host)
        for vo, V, variants in ((ident, H_, None), (_three(H_), 3, _three(H_))):
            monkeypatch.delenv("VGX_LINEAGES_TILE_RECORDS", raising=False)
            whole = ens.lineages(times=grid, variants=variants, seed=WALK_SEED)
            assert whole.status[0] == 0 and whole.records[0] > CAP + 256 and tiles_of(whole.records[0]) > CAP, (whole.status, whole.records)
            monkeypatch.setenv("VGX_LINEAGES_TILE_RECORDS", "1")
            one = ens.lineages(times=grid, variants=variants, seed=WALK_SEED)
            assert assert_rows_equal_host(ens, one, WALK_SEED, grid, vo, V) >= 1
            for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
                assert np.array_equal(getattr(one, k), getattr(whole, k)), (V, k)
    finally:
        ens.close()


# ---- 3. tau consumers: the prefix chain and the replicates' own rows
BIG = 10 ** 12


TAU_STEPS = 700                               # some 250 rows per step at the end: more than 65535 + 300 own rows per replicate


def own_points(t_own):
    """Grid points among a replicate's own steps: between its first steps (one exactly at a step's time), in the middle, and
    before each of its last steps."""
    k = len(t_own)
    return {0.5 * float(t_own[2] + t_own[3]), float(t_own[6]), 0.5 * float(t_own[k // 2] + t_own[k // 2 + 1]), float(t_own[k - 40]),
            0.5 * float(t_own[k - 3] + t_own[k - 2]), 0.5 * float(t_own[k - 2] + t_own[k - 1])}


@pytest.fixture(scope="module")
def tau():
    """tau_b of tests/models.py after a direct warm-up of N events on the Simulator, then TAU_STEPS tau steps on 2 replicates: the
    prefix is a chain of N one-row events, counted once per call through the launcher and kernel of the replicates' own rows,
    and every replicate's own steps hold more rows than a launch has workgroup rows as well."""
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, "tau_b")
        phases[0][0](sim)
        sim.simulate(iterations=N)
    ens = Ensemble(sim, 2, seeds=SEEDS[:2])
    ens.simulate_tau(TAU_STEPS, sample_size=BIG, record_events=True)
    m = ens.model
    n_pre = int(m.events.ptr)
    t_pre = np.array(m.events.times[:n_pre], dtype=np.float64)
    chains = tau_prevalence.chains_of(ens)
    points = set(common_grid([t_pre]).tolist())
    for _, _, events, _ in chains.values():
        points |= own_points(np.asarray(events[0][n_pre:], dtype=np.float64))
    d = types.SimpleNamespace(ens=ens, n_pre=n_pre, t_pre=t_pre, grid=np.array(sorted(points)), chains=chains)
    yield d
    ens.close()


def assert_prefix_reached(d):
    """The prefix: N one-row events with borders in its head and tail.  The own rows of every replicate: more than 65535 + 300,
    with borders (which fall between steps) in the head and the tail of the rows."""
    assert d.n_pre == N and tiles_of(d.n_pre) > CAP and (np.diff(d.grid) > 0).all()
    assert_borders_in_head_and_tail(d.t_pre, d.grid)
    assert (np.asarray(d.ens.model.events.types[:d.n_pre]) != 6).all()                     # direct events: one row each
    for host, _, events, rows in d.chains.values():
        assert not host.restarted and host.own_steps == TAU_STEPS and len(events[0]) == N + TAU_STEPS    # every chain starts with the prefix
        t_own = np.asarray(events[0][N:], dtype=np.float64)
        first_row = np.concatenate([[0], np.cumsum([len(r) for r in rows[N:]])])           # of every own step, and the end
        assert first_row[-1] > CAP + MARGIN
        for side in ("left", "right"):
            assert_cuts_in_head_and_tail(first_row[np.searchsorted(t_own, d.grid, side=side)], first_row[-1])
        assert np.isin(d.grid, t_own).any()


def test_tau_incidence(tau, monkeypatch):
    assert_prefix_reached(tau)
    ens, edges = tau.ens, tau.grid
    counts, outside = tau_incidence.want_block(ens, tau_incidence.chains_of(ens), range(2), edges)
    assert counts[:, 0].any() and counts[:, -1].any() and outside.any(axis=0).all()
    whole = ens.tau_incidence(edges=edges)
    monkeypatch.setenv("VGX_INCIDENCE_TILE_EVENTS", "1")
    one = ens.tau_incidence(edges=edges)
    assert one.passes == 2                                                                   # the prefix, then the replicates
    tau_incidence.assert_equals(one, counts, outside, "tile 1")
    tau_incidence.assert_equals(whole, counts, outside, "default tile")


def test_tau_flows_in_both_forms(tau, monkeypatch):
    assert_prefix_reached(tau)
    ens, edges = tau.ens, tau.grid
    vo, V = variant_maps(ens.model.hapNum)["three"]
    counts, outside = tau_flows.want_block(ens, tau_flows.chains_of(ens), range(2), edges, vo, V)
    assert counts[:, 0].any() and counts[:, -1].any() and tau_flows.across(counts) > 0
    whole = ens.tau_flows(edges=edges, variants=vo)
    tau_flows.assert_equals(whole, counts, outside, "default tile")
    monkeypatch.setenv("VGX_FLOWS_TILE_EVENTS", "1")
    for form in ("dense", "split"):
        monkeypatch.setenv("VGX_FLOWS_FORM", form)
        fl = ens.tau_flows(edges=edges, variants=vo)
        assert fl.form == form and fl.passes == 2
        tau_flows.assert_equals(fl, counts, outside, ("tile 1", form))


@pytest.mark.parametrize("key", ["identity", "three"])
def test_tau_prevalence(tau, monkeypatch, key):
    assert_prefix_reached(tau)
    ens, grid = tau.ens, tau.grid
    H_ = ens.model.hapNum
    variants, V = (None, H_) if key == "identity" else tau_prevalence.three_classes(ens, tau.chains)
    vo = np.arange(H_) if variants is None else variants
    want = tau_prevalence.want_block(ens, tau.chains, range(2), grid, vo, V)
    assert len(np.unique(want[0])) > 10 and want[2].any(axis=0).all()
    whole = ens.tau_prevalence(times=grid, variants=variants)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "1")
    one = ens.tau_prevalence(times=grid, variants=variants)
    assert one.passes == 2
    tau_prevalence.assert_equals(one, *want, what="tile 1")
    tau_prevalence.assert_equals(whole, *want, what="default tile")


@pytest.mark.parametrize("k", [0, 1], ids=["identity", "partial"])
def test_tau_susceptibles(tau, monkeypatch, k):
    assert_prefix_reached(tau)
    ens, grid = tau.ens, tau.grid
    co, G = maps_of(ens.model.susNum)[k]
    want = tau_susceptibles.want_block(ens, tau.chains, range(2), grid, co, G)
    assert len(np.unique(want[0])) > 10 and want[2].any(axis=0).all()
    whole = ens.tau_susceptibles(times=grid, groups=None if k == 0 else co)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "1")
    one = ens.tau_susceptibles(times=grid, groups=None if k == 0 else co)
    assert one.passes == 2
    tau_susceptibles.assert_equals(one, *want, what="tile 1")
    tau_susceptibles.assert_equals(whole, *want, what="default tile")


@pytest.fixture(scope="module")
def tau_milestone_rows(tau):
    """The restatement of the tau milestones, formed once for the two workgroup shapes; shared and never changed."""
    variants, V = tau_prevalence.three_classes(tau.ens, tau.chains)
    return variants, V, tau_milestones.want_rows(tau.ens, tau.chains, range(2), variants, V)


@pytest.mark.parametrize("waves", [None, "4"])
def test_tau_milestones(tau, tau_milestone_rows, monkeypatch, waves):
    assert_prefix_reached(tau)
    ens = tau.ens
    variants, V, want = tau_milestone_rows
    for w in want:                                                     # a threshold first met in the head, a peak behind the cap
        first = w["first_event"]
        assert ((first >= 0) & (first < MARGIN)).any() and (w["peak_event"] >= CAP).any()
    whole = ens.tau_milestones(variants=variants, thresholds=tau_milestones.THRESHOLDS)
    if waves is not None:
        monkeypatch.setenv("VGX_TAU_MILESTONES_WAVES", waves)
    monkeypatch.setenv("VGX_TAU_MILESTONES_TILE_ROWS", "1")
    one = ens.tau_milestones(variants=variants, thresholds=tau_milestones.THRESHOLDS)
    assert one.passes == 2
    tau_milestones.assert_rows(one, want, ("tile 1", waves))
    tau_milestones.assert_rows(whole, want, "default tile")


# ---- 4. lineages on every direct kernel's final state
LONG_LIST_SEEDS = (301, 303, 304, 305)        # runs in which the sampled population's epidemic takes off


def long_list_start():
    """A start whose sampled lineages can coalesce although an occupancy list holds more than a 64-entry tile (the long-list form
    of the row kernel from its first event): population 0 holds 70 haplotypes of one host each (and the index case) that hardly
    transmit and are never sampled, population 3 one host; no migration.  Every sampled case descends from that host, and with
    4^8 haplotypes and mutation its population's list grows to some 200 entries within the call."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=8, populations_number=4, number_of_susceptible_groups=1, seed=2020)
    sim.set_transmission_rate(2.5); sim.set_recovery_rate(0.5); sim.set_sampling_rate(0.5)
    sim.set_mutation_rate(0.2); sim.set_population_size(10 ** 6); sim.set_contact_density(0.01, population=0)
    for pn in range(3):
        sim.set_sampling_multiplier(0.0, population=pn)
    m = sim.simulation
    haps = np.random.default_rng(11).choice(np.arange(1, m.hapNum), size=70, replace=False)
    m.infectious[0, haps] = 1
    m.susceptible[0, 0] -= 70
    m.infectious[3, 0] = 1
    m.susceptible[3, 0] -= 1
    m.set_mutation_rate(0.2, None, None)
    assert np.count_nonzero(m.infectious[0]) > 64
    return sim


def assert_lineages_read_the_final_state(ens, what, variants=None):
    """lineages() first, before any call that brings the 8-byte counts of the lists up to date by itself (replicate_state,
    genealogies); then row by row against the host replay, and the walk's status and generator against genealogies()."""
    H_ = ens.model.hapNum
    vo, V = (np.arange(H_, dtype=np.int32), H_) if variants is None else (variants, int(variants.max()) + 1)
    grid = _grid(ens)
    ln = ens.lineages(times=grid, variants=variants, seed=None)
    healthy = assert_rows_equal_host(ens, ln, None, grid, vo, V)
    batch = ens.genealogies(seed=None)
    assert np.array_equal(ln.status, batch.status) and np.array_equal(ln.status_arg, batch.status_arg), what
    assert np.array_equal(ln.rng_raw, batch.rng_raw), what
    return healthy


def test_lineages_read_every_direct_kernels_final_state():
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    ran = set()
    runs = [(k, dict(kernel=k)) for k in ("wave", "lane", "quad", "quadg", "solo", "lone")] + [("fast", dict(kernel="quad", mode="fast"))]
    for what, kw in runs:
        try:
            ens = _ensemble("g5_short", 4, n_max=2000, **kw)
        except _capi.VgxError as e:   # a kernel that does not take the model refuses the call (bad argument); anything else is a failure
            assert e.code == 1, (what, str(e))
            continue
        try:
            ran.add("fast" if what == "fast" else ens.engine.last_kernel)
            assert what != "fast" or ens.engine.last_kernel == "quad"
            assert assert_lineages_read_the_final_state(ens, what) > 0, what
        finally:
            ens.close()
    assert {"wave", "quad", "quadg", "solo", "fast"} <= ran, ran
    # a list of more than a tile from the start: the row kernel's long-list form, which keeps the 4-byte counts only
    ens = Ensemble(long_list_start(), 4, seeds=np.array(LONG_LIST_SEEDS, dtype=np.int64))
    try:
        with helpers.quiet():
            ens.simulate(2000, sample_size=10 ** 9, record_events=True, kernel="quad")
        assert ens.engine.last_kernel == "quad"
        healthy = assert_lineages_read_the_final_state(ens, "long lists", _three(ens.model.hapNum))    # (4^8 haplotypes: three classes, one untracked)
        assert healthy > 0
        # (only now: replicate_state brings the 8-byte counts up to date by itself)
        assert max(np.count_nonzero(ens.replicate_state(r).infectious[3]) for r in range(4)) > 128      # the sampled population's final list
    finally:
        ens.close()
