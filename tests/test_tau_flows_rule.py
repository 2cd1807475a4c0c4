"""The flows rule of tau chains (vgsim_amd/csrc/vgx_tau_flows.h: weighted rows in the one cell of vgx_flows.h, cuts in row index
space, `outside` as sums of num, int64 cells, the two forms with 8-byte cells, the prefix counted once and added), compiled for
the host and reached through vgx_test_tau_flows: the CPU oracle's tau chains, every split of a chain into prefix and own steps,
every tile size, both forms, hand-made chains, against the literal restatement below and, for the margins, against the
independent vgx_test_tau_incidence (never against the code under test), all with array_equal on integers; the form choice and
the refusals; and the argument checks of Ensemble.tau_flows, which are raised before the library is called.  No GPU.

As in test_tau_incidence_rule.py the hook flattens the PREFIX with the checks of the flattening and takes a replicate's OWN rows
as they are: the hand-made chains put rows the flattening would refuse into the own steps."""
import numpy as np
import pytest

from test_flows_rule import offdiagonal_pairs, variant_maps
from test_incidence_rule import bare_ensemble
from test_tau_incidence_rule import MEV_COLUMNS, make, oracle_chain

B, D, SA, MU, SC, MI, MULTI = range(7)
LDS = 65536
FORMS = {"dense": 1, "split": 2}


def flat_records(events, mev):
    """The chain flattened to (num, type, haplotype, population, newHaplotype, newPopulation) records, and every event's first record."""
    cols = [np.asarray(c, dtype=np.int64) for c in events[1:6]]
    recs, first = [], []
    for i in range(len(cols[0])):
        first.append(len(recs))
        t = int(cols[0][i])
        if t == MULTI:
            for j in range(int(cols[1][i]), int(cols[2][i])):
                recs.append(tuple(int(mev[c][j]) for c in MEV_COLUMNS))
        else:
            recs.append((1, t) + tuple(int(c[i]) for c in cols[1:]))
    return recs, first


def restate_weighted_flows(events, mev, P, edges, variant_of, V, within=True, flat=None):
    """The rule as Python loops: the chain flattened to records, the cuts formed by the loop over EVENTS, every record adding num
    at its one cell.  Returns (counts [T, P, P, V] int64 in src, dst, class order, outside [2] int64).  `flat`: flat_records of the
    same chain, to flatten a long chain once."""
    times = np.asarray(events[0], dtype=np.float64)
    recs, first = flat_records(events, mev) if flat is None else flat
    T, cut, point, H = len(edges) - 1, [], 0, len(variant_of)
    for i, t in enumerate(times):
        while point <= T and edges[point] <= t:
            cut.append(first[i])                       # an event without rows: the first row after it
            point += 1
    cut += [len(recs)] * (T + 1 - len(cut))
    counts = np.zeros((T, P, P, V), dtype=np.int64)
    for b in range(T):
        for j in range(cut[b], cut[b + 1]):
            num, t, hap, pop, _, npop = recs[j]
            if num <= 0:
                continue
            if t >= 0:
                t &= ~0x100                            # the direct flag of a flattened row
            if t == B:
                if not within:
                    continue
                src, dst = pop, pop
            elif t == MI:
                src, dst = pop, npop
            else:
                continue
            if not (0 <= src < P and 0 <= dst < P and 0 <= hap < H):   # (an index of 2^31 or more lies outside every such range)
                continue
            c = int(variant_of[hap])
            if c < 0:
                continue
            counts[b, src, dst, c] += num
    pos = [max(r[0], 0) for r in recs]
    return counts, np.array([sum(pos[:cut[0]]), sum(pos[cut[T]:])], dtype=np.int64)


def hook(events, mev, P, H, edges, variant_of, V, within=True, tile=0, form=0, n_own=-1):
    from vgsim_amd import _capi
    return _capi.replay_tau_flows(events, mev, P, H, edges, variant_of, V, within, tile, form, n_own)


def forms_that_fit(P, V):
    return [f for f, cells in (("dense", P * P * V), ("split", P * V)) if 8 * cells <= LDS]


def assert_hook_equals(events, mev, P, H, edges, vo, V, within=True, tile=0, form=0, n_own=-1, what="", want=None):
    got, out, ran = hook(events, mev, P, H, edges, vo, V, within, tile, form, n_own)
    want, wout = restate_weighted_flows(events, mev, P, edges, vo, V, within) if want is None else want
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), what
    assert np.array_equal(out, wout), what
    assert ran == (form if form in FORMS else forms_that_fit(P, V)[0]), what
    return got, out


def migrations_of(flat):
    """(rows, summed num, rows with equal keys) of the MIGRATION records with num > 0"""
    mig = [r for r in flat[0] if r[0] > 0 and r[1] >= 0 and (r[1] & ~0x100) == MI]
    return len(mig), sum(r[0] for r in mig), sum(1 for r in mig if r[3] == r[5])


# ---- the oracle's chains
@pytest.mark.parametrize("name", ("tau_a", "tau_b", "tau_c", "tau_d", "tau_then_direct"))
def test_hook_equals_restatement_on_oracle_chains(oracle_mod, name):
    m, ev, mev = oracle_chain(oracle_mod, name)
    P, H, types = m.popNum, m.hapNum, ev[1]
    assert (types == MULTI).any() and (types != MULTI).any()
    flat = flat_records(ev, mev)
    n_mig, num_mig, equal = migrations_of(flat)
    assert equal == 0
    if name == "tau_a":
        assert P == 1 and n_mig == 0                                # one population: the diagonal alone
    else:
        assert P > 1 and n_mig > 0 and num_mig >= n_mig
    tl = ev[0][-1]
    for T in (100, 7, 1):
        edges = np.linspace(ev[0][len(types) // 10], 0.9 * tl, T + 1)   # events lie before, inside and behind the window
        for key, (vo, V) in variant_maps(H).items():
            forms = forms_that_fit(P, V)
            assert "split" in forms, (name, key)
            for within in (True, False):
                want = restate_weighted_flows(ev, mev, P, edges, vo, V, within, flat=flat)
                diag = np.einsum('bppc->', want[0])
                assert (diag > 0) == within and want[1].all(), (name, T, key, within)
                if name != "tau_a":
                    assert want[0].sum() - diag > 0 and offdiagonal_pairs(want[0]) > 0, (name, T, key)
                else:
                    assert want[0].sum() == diag
                for form in forms:
                    assert_hook_equals(ev, mev, P, H, edges, vo, V, within, 0, form, what=(name, T, key, within, form), want=want)
                if T == 7:
                    assert_hook_equals(ev, mev, P, H, edges, vo, V, within, 257, 0, what=(name, key, within, "auto"), want=want)


def mixed_slice(oracle_mod, n=160):
    """about n events of tau_then_direct around its first step: direct, tau steps, direct again"""
    m, ev, mev = oracle_chain(oracle_mod, "tau_then_direct")
    a = int(np.argmax(ev[1] == MULTI))
    lo = max(0, a - n // 2)
    ev = [c[lo:lo + n] for c in ev]
    assert (ev[1] == MULTI).any() and (ev[1] != MULTI).any() and len(ev[0]) == n
    return m, ev, mev


def test_every_split_into_prefix_and_own_events_gives_the_whole_chain(oracle_mod):
    """The check on prefix-once: wherever the chain is split, the prefix block plus the own rows' block is the block of the literal
    loop over the whole chain."""
    m, ev, mev = mixed_slice(oracle_mod)
    n, P, H = len(ev[0]), m.popNum, m.hapNum
    vo, V = variant_maps(H)["three"]
    for T in (9, 1):
        edges = np.linspace(ev[0][n // 5], ev[0][4 * n // 5], T + 1)
        want = restate_weighted_flows(ev, mev, P, edges, vo, V)
        assert want[0].any() and want[1].all()
        for form in forms_that_fit(P, V):
            for k in range(n + 1):
                assert_hook_equals(ev, mev, P, H, edges, vo, V, True, 7, form, n_own=k, what=(T, form, k), want=want)


def test_every_tile_size_gives_the_same_block_in_both_forms(oracle_mod):
    m, ev, mev = oracle_chain(oracle_mod, "tau_b")
    n_direct = int(np.argmax(ev[1] == MULTI))
    # (the oracle's multievent log is dense: hundreds of rows per step.)  40 direct events, the first step with a migration among
    # its rows and the step after it
    moving = next(i for i in range(n_direct, len(ev[0]))
                  if ev[1][i] == MULTI and any(mev["types"][j] == MI and mev["num"][j] > 0 for j in range(ev[2][i], ev[3][i])))
    keep = list(range(max(0, n_direct - 40), n_direct)) + [moving, moving + 1]
    ev = [c[keep] for c in ev]
    steps = ev[1] == MULTI
    rows = int((~steps).sum() + (ev[3][steps] - ev[2][steps]).sum())
    assert 100 < rows < 2000 and int(steps.sum()) == 2
    P, H = m.popNum, m.hapNum
    vo, V = variant_maps(H)["three"]
    assert forms_that_fit(P, V) == ["dense", "split"]
    edges = np.linspace(ev[0][10], 0.5 * (ev[0][-2] + ev[0][-1]), 8)   # the last step lies behind the window
    want = restate_weighted_flows(ev, mev, P, edges, vo, V)
    assert want[0].any() and want[1].all() and offdiagonal_pairs(want[0]) > 0
    for form in ("dense", "split"):
        for tile in range(1, rows + 2):
            assert_hook_equals(ev, mev, P, H, edges, vo, V, True, tile, form, what=(form, tile), want=want)


@pytest.mark.parametrize("name", ("tau_b", "tau_c", "tau_d", "tau_then_direct"))
def test_margins_are_the_channels_of_the_tau_incidence_hook(oracle_mod, name):
    """vgx_test_tau_incidence is older code with its own rule and its own tests: with hap_mask = the members of class c, the sum
    over src is births + arrivals, the off-diagonal sum over dst the departures, the diagonal the births (no MIGRATION of these
    chains has equal keys)."""
    from vgsim_amd import _capi
    m, ev, mev = oracle_chain(oracle_mod, name)
    P, H = m.popNum, m.hapNum
    assert migrations_of(flat_records(ev, mev))[2] == 0
    edges = np.linspace(ev[0][len(ev[0]) // 10], 0.9 * ev[0][-1], 13)
    maps = variant_maps(H)
    seen = 0
    for key in ("one", "three") + (("own",) if H <= 16 else ()):
        vo, V = maps[key]
        for form in forms_that_fit(P, V):
            got, out, _ = hook(ev, mev, P, H, edges, vo, V, True, 257, form)
            diag = np.einsum('bppc->bpc', got)
            for c in range(V):
                members = np.flatnonzero(vo == c)
                inc, iout = _capi.replay_tau_incidence(ev, mev, P, H, edges, _capi.haplotype_mask(members, H))
                assert inc.dtype == np.int64 and np.array_equal(out, iout)
                assert np.array_equal(got[..., c].sum(axis=1), inc[..., 0] + inc[..., 5]), (name, key, c)    # over src: new infections in dst
                assert np.array_equal(got[..., c].sum(axis=2) - diag[..., c], inc[..., 6]), (name, key, c)   # over dst, off the diagonal
                assert np.array_equal(diag[..., c], inc[..., 0]), (name, key, c)
                seen += int(inc[..., 5].sum())
    assert seen > 0


# ---- hand-made chains: events (time, type, haplotype, population, newHaplotype, newPopulation), MULTITYPE ones carrying their row
# range in (haplotype, population); rows (num, type, haplotype, population, newHaplotype, newPopulation)
P3, H4, V2 = 3, 4, 2
VO = np.array([0, 1, -1, 1], dtype=np.int32)                         # haplotype 2 is not tracked


def test_rows_that_count_nowhere_equal_keys_the_direct_flag_and_sums_beyond_32_bits():
    big = 2 ** 31 - 1
    rows = [(3, MI, 0, 2, 0, 2),                                     # 0: equal keys land on the diagonal: (2, 2, class 0) += 3
            (0, B, 0, 0, 0, 0), (-7, B, 0, 0, 0, 0), (-2, MI, 0, 0, 0, 1),   # 1..3: num = 0 and negative num: nothing, not in `outside` either
            (2, B, 0, 3, 0, 0), (2, B, 0, -1, 0, 0), (2, MI, 0, -1, 0, 1), (2, MI, 0, 1, 0, 3), (2, MI, 0, 1, 0, -1), (2, MI, 0, 3, 0, 0),   # 4..9: keys P and -1
            (2, B, 4, 0, 0, 0), (2, MI, -1, 0, 0, 1), (2, B, 2, 0, 0, 0),   # 10..12: haplotype H, -1, and one that is not tracked
            (2, B, 0, 2 ** 31, 0, 0), (2, MI, 0, 1, 0, 2 ** 40), (2, B, 2 ** 32 + 1, 0, 0, 0), (2, 2 ** 32, 0, 0, 0, 0),   # 13..16: fields beyond 31 bits
            (2, D, 0, 0, 0, 1), (2, SA, 0, 0, 0, 1), (2, MU, 0, 0, 1, 1), (2, SC, 0, 0, 1, 1), (2, 6, 0, 0, 0, 1), (2, -1, 0, 0, 0, 1), (2, 7, 0, 0, 0, 1),   # 17..23: other types
            (2, B | 0x100, 1, 2, 0, 0), (5, MI | 0x100, 3, 0, 0, 1),   # 24, 25: the direct flag is masked off: (2, 2, class 1) += 2, (0, 1, class 1) += 5
            (4, MI, 1, 2, 2, 0),                                     # 26: (2, 0, class 1) += 4: newHaplotype is not looked at
            (big, MI, 1, 1, 0, 0), (big, MI, 3, 1, 0, 0), (big, MI, 1, 1, 0, 0)]   # 27..29: one cell, three times 2^31 - 1
    events = [(0.25, B, 1, 1, 0, 0),                                 # before the window
              (1.0, MULTI, 0, 4, 0, 0), (1.5, MULTI, 4, 24, 0, 0),
              (2.0, MULTI, 24, 24, 0, 0),                            # no rows, exactly on edges[1]: its cut is the first row after it
              (1.75, MULTI, 24, 27, 0, 0),                           # time goes back: `point` does not, the rows stay in bin 1
              (2.5, MULTI, 27, 30, 0, 0),
              (9.0, MULTI, 0, 1, 0, 0)]                              # behind the window
    ev, mev = make(events, rows)
    edges = np.array([0.5, 2.0, 3.0])
    want = np.zeros((2, P3, P3, V2), dtype=np.int64)
    want[0, 2, 2, 0] = 3
    want[1, 2, 2, 1], want[1, 0, 1, 1], want[1, 2, 0, 1] = 2, 5, 4
    want[1, 1, 0, 1] = 3 * big
    assert 3 * big > 2 ** 32
    across = want.copy()
    across[1, 2, 2, 1] = 0                                           # within = 0: the birth goes, the migration with equal keys stays
    for within, block in ((True, want), (False, across)):
        lit, lout = restate_weighted_flows(ev, mev, P3, edges, VO, V2, within)
        assert np.array_equal(lit, block) and lout.tolist() == [1, 3]
        for form in ("dense", "split", 0):
            for tile in (1, 2, 3, 5, 31, 0):
                for n_own in (-1, 7):                                # the steps, or every event (the flattening of a prefix would refuse these rows)
                    got, out = assert_hook_equals(ev, mev, P3, H4, edges, VO, V2, within, tile, form, n_own, what=(within, form, tile, n_own))
                    assert np.array_equal(got, block) and out.tolist() == [1, 3]


def test_a_migration_with_equal_keys_shifts_the_margin_identity():
    from vgsim_amd import _capi
    rows = [(5, B, 0, 1, 0, 0), (3, MI, 0, 1, 0, 1), (2, MI, 0, 1, 0, 2), (4, MI, 0, 0, 0, 1)]
    ev, mev = make([(1.0, MULTI, 0, 4, 0, 0)], rows)
    edges = np.array([0.0, 2.0])
    vo = np.zeros(H4, dtype=np.int32)
    for form in ("dense", "split"):
        for n_own in (-1, 0):
            got, _ = assert_hook_equals(ev, mev, P3, H4, edges, vo, 1, True, 0, form, n_own)
            inc, _ = _capi.replay_tau_incidence(ev, mev, P3, H4, edges)
            g, diag = got[0, :, :, 0], np.diagonal(got[0, :, :, 0])
            same = np.array([0, 3, 0])                               # the equal-key migration: an arrival and a departure of population 1
            assert diag.tolist() == [0, 8, 0]
            assert np.array_equal(diag, inc[0, :, 0] + same)
            assert np.array_equal(g.sum(axis=0), inc[0, :, 0] + inc[0, :, 5])        # unchanged: an arrival is a new infection in dst
            assert np.array_equal(g.sum(axis=1) - diag, inc[0, :, 6] - same)


def test_a_step_without_rows_still_advances_the_cuts_and_an_empty_chain_counts_nothing():
    rows = [(3, B, 1, 0, 0, 0), (2, MI, 1, 0, 0, 1), (5, MI, 3, 1, 0, 2), (4, B, 0, 2, 0, 0)]
    events = [(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 2, 0, 0),
              (2.0, MULTI, 2, 2, 0, 0),                              # no rows, on edges[1]
              (1.5, MULTI, 2, 3, 0, 0),                              # bin 1, although its time lies in bin 0
              (3.0, MULTI, 3, 4, 0, 0)]
    ev, mev = make(events, rows)
    edges = np.array([1.0, 2.0, 3.0])
    want = np.zeros((2, P3, P3, V2), dtype=np.int64)
    want[0, 0, 0, 1], want[0, 0, 1, 1], want[1, 1, 2, 1] = 3, 2, 5
    for form in ("dense", "split"):
        for n_own in (-1, 0, 2, 3, 5):
            got, out = assert_hook_equals(ev, mev, P3, H4, edges, VO, V2, True, 2, form, n_own, what=(form, n_own))
            assert np.array_equal(got, want) and out.tolist() == [1, 4]
    none = [np.zeros(0)] + [np.zeros(0, dtype=np.int64)] * 5
    for form in ("dense", "split", 0):
        got, out = assert_hook_equals(none, None, P3, H4, edges, VO, V2, form=form)
        assert got.shape == (2, P3, P3, V2) and not got.any() and out.tolist() == [0, 0]


# ---- the form choice
def random_chain(P, H, seed, n_direct=60, n_steps=12, rows_per_step=40):
    rng = np.random.default_rng(seed)
    events, rows = [], []
    t = 0.0
    for _ in range(n_direct):
        t += rng.exponential(0.1)
        typ = int(rng.choice([B, D, MI, MU]))
        events.append((t, typ, int(rng.integers(H)), int(rng.integers(P)), int(rng.integers(H)), int(rng.integers(P))))
    for _ in range(n_steps):
        t += 0.5
        k = int(rng.integers(0, rows_per_step))
        events.append((t, MULTI, len(rows), len(rows) + k, 0, 0))
        for _ in range(k):
            rows.append((int(rng.integers(0, 50)), int(rng.choice([B, D, MI, MI])), int(rng.integers(H)), int(rng.integers(P)),
                         int(rng.integers(H)), int(rng.integers(P))))
    return make(events, rows), t


def test_dense_runs_where_it_fits_and_split_behind_it():
    H = 3
    vo = np.zeros(H, dtype=np.int32)
    for P, auto in ((90, "dense"), (91, "split")):
        assert (8 * P * P <= LDS) == (auto == "dense")
        (ev, mev), t_end = random_chain(P, H, seed=P)
        edges = np.linspace(1.0, 0.9 * t_end, 6)
        want = restate_weighted_flows(ev, mev, P, edges, vo, 1)
        assert offdiagonal_pairs(want[0]) > 50 and want[1].all()
        for n_own in (-1, 0):
            got, out, ran = hook(ev, mev, P, H, edges, vo, 1, n_own=n_own)
            assert ran == auto and np.array_equal(got, want[0]) and np.array_equal(out, want[1])
            assert_hook_equals(ev, mev, P, H, edges, vo, 1, True, 64, "split", n_own, want=want)
    with pytest.raises(ValueError, match="vgx_test_tau_flows: 91 populations x 1 classes need 66248 bytes of 8-byte cells in the dense form, above the 65536 bytes"):
        hook(ev, mev, 91, H, edges, vo, 1, form="dense")
    assert_hook_equals(*random_chain(90, H, seed=90)[0], 90, H, edges, vo, 1, True, 64, "dense")


def test_cells_above_the_lds_budget_are_refused_in_every_form():
    edges = np.array([0.0, 1.0])
    last, _ = make([(0.5, B, 8191, 0, 0, 0)], [])
    got, _, ran = hook(last, None, 1, 8192, edges, np.arange(8192, dtype=np.int32), 8192)     # 8 * 8192 = 65536 bytes fit (dense and split alike)
    assert ran == "dense" and got[0, 0, 0, 8191] == 1 and got.sum() == 1
    for P, V, need in ((1, 8193, 65544), (2, 4097, 65552), (130, 64, 66560)):
        vo = np.arange(V, dtype=np.int32)
        for form in (0, "split"):
            with pytest.raises(ValueError, match="vgx_test_tau_flows: %d populations x %d classes need %d bytes of 8-byte cells in the split form, above the 65536 bytes" % (P, V, need)):
                hook(last, None, P, V, edges, vo, V, form=form)
        with pytest.raises(ValueError, match="vgx_test_tau_flows: .* bytes of 8-byte cells in the dense form"):
            hook(last, None, P, V, edges, vo, V, form="dense")


# ---- refusals of the hook
def test_the_hooks_refusals():
    ev, mev = make([(0.5, B, 0, 0, 0, 0), (1.0, MULTI, 0, 1, 0, 0)], [(1, B, 0, 0, 0, 0)])
    ok, vo = np.array([0.0, 2.0]), np.zeros(2, dtype=np.int32)
    for edges, text in (([0.0, 1.0, 1.0], "increase strictly"), ([1.0, 0.5], "increase strictly"), ([0.0, float("nan")], "not finite"),
                        ([0.0, float("inf")], "not finite"), ([0.0], "T = 0 bins: at least 1")):
        with pytest.raises(ValueError, match="vgx_test_tau_flows: .*" + text):
            hook(ev, mev, 2, 2, np.array(edges), vo, 1)
    with pytest.raises(ValueError, match="vgx_test_tau_flows: V = 0 classes: at least 1"):
        hook(ev, mev, 2, 2, ok, vo, 0)
    with pytest.raises(ValueError, match=r"vgx_test_tau_flows: variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook(ev, mev, 2, 2, ok, np.array([0, 2], dtype=np.int32), 2)
    with pytest.raises(ValueError, match=r"vgx_test_tau_flows: variant_of\[0\] = -2 is outside \[-1, 2\)"):
        hook(ev, mev, 2, 2, ok, np.array([-2, 0], dtype=np.int32), 2)
    for form in (3, -1):
        with pytest.raises(ValueError, match="vgx_test_tau_flows: form = %d is none of" % form):
            hook(ev, mev, 2, 2, ok, vo, 1, form=form)
    with pytest.raises(ValueError, match="form must be"):
        hook(ev, mev, 2, 2, ok, vo, 1, form="sparse")
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook(ev, mev, 2, 2, ok, vo, 1, tile=-1)
    for n_own in (-1, 0):                                            # as an own step and as part of the prefix
        for bad in ((1.0, MULTI, 0, 2, 0, 0), (1.0, MULTI, -1, 1, 0, 0)):
            ev2, _ = make([(0.5, B, 0, 0, 0, 0), bad], [])
            with pytest.raises(ValueError, match="MULTITYPE row range outside the multievent log"):
                hook(ev2, mev, 2, 2, ok, vo, 1, n_own=n_own)
    with pytest.raises(ValueError, match="n_own_events"):
        hook(ev, mev, 2, 2, ok, vo, 1, n_own=3)
    neg = make([(1.0, MULTI, 0, 1, 0, 0)], [(-1, B, 0, 0, 0, 0)])
    with pytest.raises(ValueError, match="value out of range"):      # the prefix passes the checks of the flattening
        hook(*neg, 2, 2, ok, vo, 1, n_own=0)
    got, out, _ = hook(*neg, 2, 2, ok, vo, 1, n_own=1)               # as an own row it counts nothing
    assert not got.any() and out.tolist() == [0, 0]


# ---- Ensemble.tau_flows: refusals before the library
@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either edges or bins"),
    (dict(edges=[0.0, 1.0], bins=4, window=(0, 1)), "either edges or bins"),
    (dict(bins=4), "window"),
    (dict(edges=[0.0, 1.0, 1.0]), "increase strictly"),
    (dict(edges=[0.0, float("nan")]), "finite"),
    (dict(edges=[0.0, 1.0], variants=[[40]]), "haplotype index out of range"),
    (dict(edges=[0.0, 1.0], variants=[[1], [1]]), "listed twice"),
    (dict(edges=[0.0, 1.0], variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(edges=[0.0, 1.0], variants=np.arange(40) * 1000), "3 populations x 39001 classes need 936024 bytes of 8-byte cells"),
    (dict(edges=[0.0, 1.0], variants=np.arange(40) * 70), "3 populations x 2731 classes need 65544 bytes of 8-byte cells"),
    (dict(edges=[0.0, 1.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[1, 1]), "distinct"),
    (dict(edges=[0.0, 1.0], counts=False), "counts=False needs summary"),
    (dict(edges=[0.0, 1.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(edges=[0.0, 1.0], summary=dict(method='nearest')), "method must be"),
    (dict(edges=[0.0, 1.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=('tau', True)).tau_flows(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate_tau"), (('direct', True), "tau chains only"), (('tau', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=last).tau_flows(edges=[0.0, 1.0])
    with pytest.raises(ValueError, match="flows\\(\\) counts direct chains only"):   # the direct call still refuses tau chains
        bare_ensemble(last=('tau', True)).flows(edges=[0.0, 1.0])
