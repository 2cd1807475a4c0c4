"""The incidence rule of tau chains (vgsim_amd/csrc/vgx_tau_incidence.h: weighted rows, cuts in row index space, `outside` as sums
of num, int64 counts, the prefix counted once and added), compiled for the host and reached through vgx_test_tau_incidence: the
CPU oracle's tau chains, every split of a chain into prefix and own steps, every tile size, hand-made chains and the conservation
of the infectious totals, against the literal restatement below (never against the code under test), all with array_equal on
integers; and the argument checks of Ensemble.tau_incidence, which are raised before the library is called.  No GPU.

The hook flattens the PREFIX with the checks of the tau timelines' flattening (a negative num or a field outside 32 bits is
refused there) and takes a replicate's OWN rows as they are, as the device reads them: the hand-made chains put such rows into
the own steps."""
import numpy as np
import pytest

import helpers
from test_incidence_rule import CHANNELS, bare_ensemble, cells

B, D, SA, MU, SC, MI, MULTI = range(7)
MEV_COLUMNS = ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")
CHAINS = ("tau_a", "tau_b", "tau_c", "tau_d", "tau_then_direct")


def restate_weighted(events, mev, P, edges, haplotypes=None):
    """The rule as Python loops.  events: times and the five columns; mev: dict of the multievent columns.  The chain is flattened
    to (time, num, five fields) records, the cuts are formed by the loop over EVENTS, every record counts num times in cells()."""
    times = np.asarray(events[0], dtype=np.float64)
    cols = [np.asarray(c, dtype=np.int64) for c in events[1:6]]
    recs, first = [], []
    for i in range(len(times)):
        first.append(len(recs))
        t = int(cols[0][i])
        if t == MULTI:
            for j in range(int(cols[1][i]), int(cols[2][i])):
                recs.append((times[i], int(mev["num"][j])) + tuple(int(mev[c][j]) for c in MEV_COLUMNS[1:]))
        else:
            recs.append((times[i], 1, t) + tuple(int(c[i]) for c in cols[1:]))
    T, cut, point = len(edges) - 1, [], 0
    for i, t in enumerate(times):
        while point <= T and edges[point] <= t:
            cut.append(first[i])                       # an event without rows: the first row after it
            point += 1
    cut += [len(recs)] * (T + 1 - len(cut))
    allowed = None if haplotypes is None else {int(h) for h in haplotypes}
    counts = np.zeros((T, P, CHANNELS), dtype=np.int64)
    for b in range(T):
        for j in range(cut[b], cut[b + 1]):
            num, rec = recs[j][1], list(recs[j][2:])
            if num <= 0:
                continue
            if rec[0] >= 0:
                rec[0] &= ~0x100                       # the direct flag of a flattened row: incidence knows no such difference
            rec = [v if 0 <= v < 2 ** 31 else -1 for v in rec]   # a field that is not a 32-bit index matches nothing
            for p, k in cells(rec, P, allowed):
                counts[b, p, k] += num
    pos = [max(r[1], 0) for r in recs]
    return counts, np.array([sum(pos[:cut[0]]), sum(pos[cut[T]:])], dtype=np.int64)


def hook(events, mev, P, H, edges, haplotypes=None, tile=0, n_own=-1):
    from vgsim_amd import _capi
    mask = None if haplotypes is None else _capi.haplotype_mask(list(haplotypes), H)
    return _capi.replay_tau_incidence(events, mev, P, H, edges, mask, tile, n_own)


def assert_hook_equals(events, mev, P, H, edges, haplotypes=None, tile=0, n_own=-1, what="", want=None):
    got, out = hook(events, mev, P, H, edges, haplotypes, tile, n_own)
    want, wout = restate_weighted(events, mev, P, edges, haplotypes) if want is None else want
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), what
    assert np.array_equal(out, wout), what
    return got, out


def events_of(m):
    ev, n = m.events, m.events.ptr
    return [ev.times[:n].copy()] + [getattr(ev, c)[:n].copy() for c in ("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")]


_CACHE = {}


def oracle_chain(oracle_mod, name):
    if name not in _CACHE:
        m = helpers.run_case_oracle(oracle_mod, name, record_multievents=True).simulation
        _CACHE[name] = (m, events_of(m), oracle_mod.get_state(m).mev)
    return _CACHE[name]


@pytest.mark.parametrize("name", CHAINS)
def test_hook_equals_restatement_on_oracle_chains(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    types = ev[1]
    assert (types == MULTI).any() and (types != MULTI).any()
    if name == "tau_then_direct":
        assert types[-1] != MULTI                                   # trailing MULTITYPE count 0: all prefix
    tl = ev[0][-1]
    occupied = sorted({int(h) for h in np.argwhere(m.infectious > 0)[:, 1]})
    for T in (100, 7, 1):
        edges = np.linspace(ev[0][len(types) // 10], 0.9 * tl, T + 1)   # events lie before, inside and behind the window
        got, out = assert_hook_equals(ev, mev, m.popNum, m.hapNum, edges, what=(name, T))
        assert got.any() and out.all()
        assert_hook_equals(ev, mev, m.popNum, m.hapNum, edges, haplotypes=occupied, what=(name, T, "filter"))


def test_every_split_into_prefix_and_own_events_gives_the_whole_chain(oracle_mod):
    """The check on prefix-once: wherever the chain is split, the prefix block plus the own rows' block is the block of the literal
    loop over the whole chain."""
    m, ev, mev = oracle_chain(oracle_mod, "tau_then_direct")       # direct, tau steps, direct again: a mixed chain
    n = 160
    a = int(np.argmax(ev[1] == MULTI))
    lo = max(0, a - n // 2)
    ev = [c[lo:lo + n] for c in ev]
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any() and len(ev[0]) == n
    for T in (9, 1):
        edges = np.linspace(ev[0][n // 5], ev[0][4 * n // 5], T + 1)
        want = restate_weighted(ev, mev, m.popNum, edges)
        assert want[0].any() and want[1].all()
        for k in range(n + 1):
            assert_hook_equals(ev, mev, m.popNum, m.hapNum, edges, tile=7, n_own=k, what=(T, k), want=want)


def test_every_tile_size_gives_the_same_counts(oracle_mod):
    m, ev, mev = oracle_chain(oracle_mod, "tau_b")
    n_direct = int(np.argmax(ev[1] == MULTI))
    keep = slice(max(0, n_direct - 40), n_direct + 2)        # (the oracle's multievent log is dense: hundreds of rows per step)
    ev = [c[keep] for c in ev]
    own = int((ev[1] == MULTI).sum())
    steps = ev[1] == MULTI
    rows = int((~steps).sum() + (ev[3][steps] - ev[2][steps]).sum())
    assert 100 < rows < 2000 and own == 2
    edges = np.linspace(ev[0][10], 0.5 * (ev[0][-2] + ev[0][-1]), 8)   # the last step lies behind the window
    want = restate_weighted(ev, mev, m.popNum, edges)
    assert want[0].any() and want[1].all()
    for tile in range(1, rows + 2):
        assert_hook_equals(ev, mev, m.popNum, m.hapNum, edges, tile=tile, what=tile, want=want)


# ---- hand-made chains: (time, type, haplotype, population, newHaplotype, newPopulation) events, MULTITYPE ones carrying their row
# range in (haplotype, population); rows (num, type, haplotype, population, newHaplotype, newPopulation)
def make(events, rows):
    ev = [np.array([e[0] for e in events], dtype=np.float64)] + [np.array([e[j] for e in events], dtype=np.int64) for j in range(1, 6)]
    mev = {c: np.array([r[j] for r in rows], dtype=np.int64) for j, c in enumerate(MEV_COLUMNS)}
    return ev, mev


def test_a_step_without_rows_on_an_edge_and_times_that_go_back():
    P, H = 2, 4
    rows = [(3, B, 1, 0, 0, 0), (2, MI, 1, 0, 0, 1), (5, D, 2, 1, 0, 0), (4, SA, 0, 0, 0, 0)]
    events = [(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 2, 0, 0),
              (2.0, MULTI, 2, 2, 0, 0),                              # no rows, exactly on edges[1]: its cut is the first row after it
              (1.5, MULTI, 2, 3, 0, 0),                              # time goes back: `point` does not, the rows stay in bin 1
              (3.0, MULTI, 3, 4, 0, 0)]
    ev, mev = make(events, rows)
    edges = np.array([1.0, 2.0, 3.0])
    want = np.zeros((2, P, CHANNELS), dtype=np.int64)
    want[0, 0, 0], want[0, 1, 5], want[0, 0, 6] = 3, 2, 2
    want[1, 1, 1] = 5
    for n_own in (-1, 0, 2, 5):
        got, out = assert_hook_equals(ev, mev, P, H, edges, n_own=n_own, what=n_own)
        assert np.array_equal(got, want) and out.tolist() == [1, 4]


def test_rows_that_count_nowhere_and_counts_beyond_32_bits():
    P, H = 3, 4
    big = 2 ** 31 + 5
    rows = [(0, B, 0, 0, 0, 0), (-7, B, 0, 0, 0, 0),                 # num = 0 and negative num: nothing, not in `outside` either
            (2, B, 0, 3, 0, 0), (2, D, 0, -1, 0, 0), (2, 6, 0, 0, 0, 0), (2, -1, 0, 0, 0, 0), (2, 7, 0, 0, 0, 0),   # keys / types out of range
            (2, MI, 0, 5, 0, 1), (2, MI, 0, 2, 0, -3),              # one key of a MIGRATION out of range: the other counts
            (2, B, 0, 2 ** 32 + 1, 0, 0), (2, MI, 0, 1, 0, 2 ** 40),  # a field beyond 32 bits matches nothing
            (2, B | 0x100, 1, 2, 0, 0),                               # the direct flag of a flattened row is masked off
            (big, SA, 1, 1, 0, 0), (big, SA, 2, 1, 0, 0), (big, SA, 3, 1, 0, 0)]
    events = [(0.25, B, 1, 1, 0, 0), (1.0, MULTI, 0, 2, 0, 0), (1.5, MULTI, 2, 12, 0, 0), (1.75, MULTI, 12, 15, 0, 0), (9.0, MULTI, 0, 2, 0, 0)]
    ev, mev = make(events, rows)
    edges = np.array([0.5, 1.6, 2.0])
    got, out = assert_hook_equals(ev, mev, P, H, edges, tile=4)
    want = np.zeros((2, P, CHANNELS), dtype=np.int64)
    want[0, 1, 5] = want[0, 2, 6] = want[0, 1, 6] = want[0, 2, 0] = 2
    want[1, 1, 2] = 3 * big
    assert 3 * big > 2 ** 32 and np.array_equal(got, want) and out.tolist() == [1, 0]
    got, _ = assert_hook_equals(ev, mev, P, H, edges, haplotypes=[2, 3], tile=1)
    assert got[1, 1, 2] == 2 * big and got.sum() == 2 * big


def test_windows_before_behind_and_inside_the_chain():
    P, H = 2, 2
    rows = [(k + 1, B, 0, k % 2, 0, 0) for k in range(12)]
    events = [(float(k), B, 1, 1, 0, 0) for k in range(3)] + [(3.0 + k, MULTI, 2 * k, 2 * k + 2, 0, 0) for k in range(6)]
    ev, mev = make(events, rows)
    total = 3 + sum(range(1, 13))
    for n_own in (-1, 0, 4, 9):
        got, out = assert_hook_equals(ev, mev, P, H, np.array([-5.0, -1.0]), n_own=n_own)              # before the chain
        assert not got.any() and out.tolist() == [0, total]
        got, out = assert_hook_equals(ev, mev, P, H, np.array([100.0, 101.0, 102.0]), n_own=n_own)     # behind it
        assert not got.any() and out.tolist() == [total, 0]
        got, out = assert_hook_equals(ev, mev, P, H, np.array([1.0, 4.5, 6.0]), n_own=n_own, tile=3)   # inside: the cuts fall on both sides of the split
        assert got.sum() + out.sum() == total and out.tolist() == [1, sum(range(7, 13))]
    got, out = assert_hook_equals([np.zeros(0)] + [np.zeros(0, dtype=np.int64)] * 5, None, P, H, np.array([0.0, 1.0]))   # an empty chain
    assert not got.any() and out.tolist() == [0, 0]


@pytest.mark.parametrize("name", CHAINS)
def test_new_infections_minus_removals_give_the_final_totals(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    got, out = hook(ev, mev, m.popNum, m.hapNum, np.array([0.0, 0.5 * ev[0][-1], np.nextafter(ev[0].max(), np.inf)]), tile=257)
    assert out.tolist() == [0, 0]
    net = got.sum(axis=0)
    start = np.asarray(m.initial_infectious, dtype=np.int64).sum(axis=1)
    assert np.array_equal(start + net[:, 0] + net[:, 5] - net[:, 1] - net[:, 2], np.asarray(m.totalInfectious, dtype=np.int64))


# ---- refusals
def test_the_hooks_refusals():
    ev, mev = make([(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 1, 0, 0)], [(1, B, 0, 0, 0, 0)])
    ok = np.array([0.0, 2.0])
    for edges, text in (([0.0, 1.0, 1.0], "increase strictly"), ([1.0, 0.5], "increase strictly"), ([0.0, float("nan")], "not finite"),
                        ([0.0], "at least 1")):
        with pytest.raises(ValueError, match="vgx_test_tau_incidence: .*" + text):
            hook(ev, mev, 2, 2, np.array(edges))
    one = make([(0.5, B, 0, 1169, 0, 0)], [])
    got, _ = hook(*one, 1170, 1, ok)                                 # 1170 * 56 = 65520 bytes fit
    assert got[0, 1169, 0] == 1 and got.sum() == 1
    with pytest.raises(ValueError, match="1171 populations need 65576 bytes"):
        hook(*one, 1171, 1, ok)
    for n_own in (-1, 0):                                            # as an own step and as part of the prefix
        for bad in ((1.0, MULTI, 0, 2, 0, 0), (1.0, MULTI, -1, 1, 0, 0)):
            ev2, _ = make([(0.5, B, 0, 0, 0, 0), bad], [])
            with pytest.raises(ValueError, match="MULTITYPE row range outside the multievent log"):
                hook(ev2, mev, 2, 2, ok, n_own=n_own)
    with pytest.raises(ValueError, match="n_own_events"):
        hook(ev, mev, 2, 2, ok, n_own=3)
    neg = make([(1.0, MULTI, 0, 1, 0, 0)], [(-1, B, 0, 0, 0, 0)])
    with pytest.raises(ValueError, match="value out of range"):      # the prefix passes the checks of the flattening
        hook(*neg, 2, 2, ok, n_own=0)


@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either edges or bins"),
    (dict(edges=[0.0, 1.0], bins=4, window=(0, 1)), "either edges or bins"),
    (dict(bins=0, window=(0, 1)), "bins must be at least 1"),
    (dict(bins=4), "window"),
    (dict(edges=[0.0, 1.0, 1.0]), "increase strictly"),
    (dict(edges=[0.0]), "at least two"),
    (dict(edges=[0.0, float("nan")]), "finite"),
    (dict(edges=[0.0, 1.0], haplotypes=[40]), "haplotype index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[1, 1]), "distinct"),
    (dict(edges=[0.0, 1.0], counts=False), "counts=False needs summary"),
    (dict(edges=[0.0, 1.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(edges=[0.0, 1.0], summary=dict(method='nearest')), "method must be"),
    (dict(edges=[0.0, 1.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=('tau', True)).tau_incidence(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate_tau"), (('direct', True), "tau chains only"), (('tau', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=last).tau_incidence(edges=[0.0, 1.0])
    with pytest.raises(ValueError, match="incidence\\(\\) counts direct chains only"):   # the direct call still refuses tau chains
        bare_ensemble(last=('tau', True)).incidence(edges=[0.0, 1.0])
