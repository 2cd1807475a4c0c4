"""The flows rule of the device pass (vgsim_amd/csrc/vgx_flows.h: the cell a record counts in, the two forms of a workgroup's
table, the walk of a tile), compiled for the host and reached through vgx_test_flows: the chains of the golden fixtures (recorded
from the reference), every tile size, both forms, against the two restatements below and, for the margins, against the
independent vgx_test_incidence (never against the code under test), all with array_equal on integers; a hand-made chain; the
refusals; the methods of the Flows object; and the argument checks of Ensemble.flows, which are raised before the library is
called.  No GPU."""
import numpy as np
import pytest

import helpers
import models
from test_incidence_rule import bare_ensemble, columns, cuts

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
GOLDEN_CASES = ("g9_short", "c3_s5_p16", "p70", "stress_h256", "recomb_a")
LDS = 65536


def restate(times, cols, P, edges, variant_of, V, within=True):
    """The rule as a Python loop over the events: (counts [T, P, P, V] int64 in src, dst, class order, outside [2])."""
    T, n, H = len(edges) - 1, len(times), len(variant_of)
    cut = cuts(times, edges)
    counts = np.zeros((T, P, P, V), dtype=np.int64)
    for b in range(T):
        for i in range(cut[b], cut[b + 1]):
            t, hap, pop, _, npop = (int(c[i]) for c in cols)
            if t == BIRTH:
                if not within:
                    continue
                src, dst = pop, pop
            elif t == MIGRATION:
                src, dst = pop, npop
            else:
                continue
            if not (0 <= src < P and 0 <= dst < P and 0 <= hap < H):
                continue
            c = int(variant_of[hap])
            if c < 0:
                continue
            counts[b, src, dst, c] += 1
    return counts, np.array([cut[0], n - cut[T]], dtype=np.int64)


def restate_sorted(times, cols, P, edges, variant_of, V, within=True):
    """The same for a chain whose times do not decrease (asserted): searchsorted and np.add.at."""
    times = np.asarray(times, dtype=np.float64)
    assert np.all(np.diff(times) >= 0)
    T, H = len(edges) - 1, len(variant_of)
    typ, hap, pop, _, npop = (np.asarray(c, dtype=np.int64) for c in cols)
    b = np.searchsorted(edges, times, side='right') - 1
    dst = np.where(typ == MIGRATION, npop, pop)
    ok = (b >= 0) & (b < T) & ((typ == MIGRATION) | ((typ == BIRTH) & bool(within)))
    ok &= (pop >= 0) & (pop < P) & (dst >= 0) & (dst < P) & (hap >= 0) & (hap < H)
    cls = np.full(len(times), -1, dtype=np.int64)
    cls[ok] = np.asarray(variant_of, dtype=np.int64)[hap[ok]]
    ok &= cls >= 0
    counts = np.zeros((T, P, P, V), dtype=np.int64)
    np.add.at(counts, (b[ok], pop[ok], dst[ok], cls[ok]), 1)
    return counts, np.array([(b < 0).sum(), (b >= T).sum()], dtype=np.int64)


def hook(times, cols, P, H, edges, variant_of, V, within=True, tile=0, form=None):
    from vgsim_amd import _capi
    return _capi.replay_flows(times, *cols, P, H, edges, variant_of, V, within, tile, form)


def forms_that_fit(P, V):
    return [f for f, cells in (("dense", P * P * V), ("split", P * V)) if 4 * cells <= LDS]


def golden_chain(name):
    """(times, the five columns as int64, P, H) of a fixture recorded from the reference."""
    meta, z = helpers.load_golden(name)
    n = meta["stats"]["ptr"]
    ctor = models.CASES[name][0]
    ints = z["ints"]
    assert ints.shape[0] == 5
    return z["times"][:n].copy(), [np.ascontiguousarray(ints[k, :n], dtype=np.int64) for k in range(5)], ctor["populations_number"], 4 ** ctor["number_of_sites"]


def variant_maps(H):
    """every haplotype its own class; one class; three classes (fewer when H < 3) with untracked haplotypes (h % 4 == 3)"""
    three = np.arange(H, dtype=np.int32) % 4
    three[three == 3] = -1
    return {"own": (np.arange(H, dtype=np.int32), H), "one": (np.zeros(H, dtype=np.int32), 1), "three": (three, min(H, 3))}


@pytest.fixture(scope="module")
def chains():
    return {name: golden_chain(name) for name in GOLDEN_CASES}


def window_of(t, T):
    return np.linspace(0.05 * t[-1], 0.9 * t[-1], T + 1)


def offdiagonal_pairs(block):
    """distinct (src, dst), src != dst, with a count anywhere in a [T, P, P, V] block"""
    m = block.sum(axis=(0, 3)) > 0
    np.fill_diagonal(m, False)
    return int(m.sum())


# ---- the golden chains
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_chains_equal_both_restatements_in_every_tile_and_form(chains, name):
    t, cols, P, H = chains[name]
    n = len(t)
    assert n > 1000 and (cols[0] == MIGRATION).sum() > 0 and not (cols[2][cols[0] == MIGRATION] == cols[4][cols[0] == MIGRATION]).any()
    for key, (vo, V) in variant_maps(H).items():
        edges = window_of(t, 5 if key == "own" else 40)
        forms = forms_that_fit(P, V)
        assert "split" in forms, (name, key)
        for within in (1, 0):
            want, wout = restate(t, cols, P, edges, vo, V, within)
            fast = restate_sorted(t, cols, P, edges, vo, V, within)
            assert np.array_equal(want, fast[0]) and np.array_equal(wout, fast[1])
            # the expected block shows what it is there for: transmissions across, and within when asked for
            diag = np.einsum('bppc->', want)
            assert want.sum() - diag > 0 and (diag > 0) == bool(within), (name, key, within)
            for form in forms:
                for tile in (1, 7, 64, n + 1):
                    got, out, ran = hook(t, cols, P, H, edges, vo, V, within, tile, form)
                    assert ran == form and got.dtype == np.int32 and got.shape == want.shape
                    assert np.array_equal(got, want), (name, key, within, form, tile)
                    assert np.array_equal(out, wout)
            auto, _, ran = hook(t, cols, P, H, edges, vo, V, within)
            assert ran == forms[0] and np.array_equal(auto, want)   # dense where it fits, else split; the default tile


def test_the_fixtures_hold_what_they_are_there_for(chains):
    # p70: a table that fits the dense form with one class and not with four; hundreds of scattered pairs
    t, cols, P, H = chains["p70"]
    assert (P, H) == (70, 4) and forms_that_fit(P, 1) == ["dense", "split"] and forms_that_fit(P, 4) == ["split"]
    want, _ = restate_sorted(t, cols, P, window_of(t, 40), np.zeros(H, dtype=np.int32), 1)
    assert offdiagonal_pairs(want) >= 100
    whole, out = restate_sorted(t, cols, P, np.array([0.0, np.nextafter(t[-1], np.inf)]), np.zeros(H, dtype=np.int32), 1)
    assert out.tolist() == [0, 0] and offdiagonal_pairs(whole) == 854 and whole.sum() - np.einsum('bppc->', whole) == 1569
    # stress_h256: every pair of 8 populations, many haplotypes among the migrations; own classes fill the dense budget exactly
    t, cols, P, H = chains["stress_h256"]
    assert (P, H) == (8, 256) and 4 * P * P * H == LDS
    vo, V = variant_maps(H)["own"]
    whole, _ = restate_sorted(t, cols, P, np.array([0.0, np.nextafter(t[-1], np.inf)]), vo, V, within=False)
    assert whole.sum() == 1049 and offdiagonal_pairs(whole) == 56 and (whole.sum(axis=(0, 1, 2)) > 0).sum() == 154
    # c3_s5_p16: the probe's workload; own classes fill the split budget exactly
    t, cols, P, H = chains["c3_s5_p16"]
    assert (P, H) == (16, 1024) and 4 * P * H == LDS
    whole, _ = restate_sorted(t, cols, P, np.array([0.0, np.nextafter(t[-1], np.inf)]), np.zeros(H, dtype=np.int32), 1, within=False)
    assert whole.sum() == 72 and offdiagonal_pairs(whole) == 21


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_margins_are_the_channels_of_the_incidence_hook(chains, name):
    """vgx_test_incidence is older code with its own rule and its own tests: with hap_mask = the members of class c, births are
    this block's diagonal, arrivals its off-diagonal sum over src, departures its off-diagonal sum over dst."""
    from vgsim_amd import _capi
    t, cols, P, H = chains[name]
    edges = window_of(t, 12)
    maps = variant_maps(H)
    seen = 0
    for key in ("one", "three") + (("own",) if H <= 16 else ()):
        vo, V = maps[key]
        for form in forms_that_fit(P, V):
            got, out, _ = hook(t, cols, P, H, edges, vo, V, True, 257, form)
            got = got.astype(np.int64)
            diag = np.einsum('bppc->bpc', got)
            for c in range(V):
                members = np.flatnonzero(vo == c)
                inc, iout = _capi.replay_incidence(t, *cols, P, H, edges, _capi.haplotype_mask(members, H))
                inc = inc.astype(np.int64)
                assert np.array_equal(out, iout)
                assert np.array_equal(got[..., c].sum(axis=1), inc[..., 0] + inc[..., 5]), (name, key, c)    # over src: new infections in dst
                assert np.array_equal(got[..., c].sum(axis=2) - diag[..., c], inc[..., 6]), (name, key, c)   # over dst, off the diagonal
                assert np.array_equal(diag[..., c], inc[..., 0]), (name, key, c)
                seen += int(inc[..., 5].sum())
    assert seen > 0


# ---- a hand-made chain
def test_hand_made_chain():
    P, H, V = 3, 4, 2
    vo = np.array([0, 1, -1, 1], dtype=np.int32)                  # haplotype 2 is not tracked
    edges = np.array([1.0, 2.0, 2.5, 4.0])                        # non-uniform, T = 3
    recs = [(BIRTH, 0, 0, 0, 0),                                  # t = 0.5: before the window
            (BIRTH, 1, 1, 0, 0),                                  # t = 1.0 = edges[0]: bin 0, (1, 1, class 1)
            (MIGRATION, 0, 2, 0, 2),                              # equal keys: the diagonal (2, 2, class 0), bin 0
            (MIGRATION, 3, 0, 0, 1),                              # t = 2.0 = edges[1]: bin 1, (0, 1, class 1)
            (MIGRATION, 0, -1, 0, 1), (MIGRATION, 0, 1, 0, 3), (MIGRATION, 0, 3, 0, 0), (BIRTH, 0, 3, 0, 0), (BIRTH, 0, -1, 0, 0),   # keys -1 and P
            (BIRTH, 4, 0, 0, 0), (MIGRATION, -1, 0, 0, 1), (BIRTH, 2, 0, 0, 0),   # haplotype hapNum, -1, and one that is not tracked
            (-1, 0, 0, 0, 0), (6, 0, 0, 0, 1), (DEATH, 0, 0, 0, 1), (SAMPLING, 0, 0, 0, 1), (MUTATION, 0, 0, 1, 1), (SUSCCHANGE, 0, 0, 1, 1),
            (MIGRATION, 1, 2, 2, 0),                              # t = 2.5 = edges[2]: bin 2, (2, 0, class 1): newHaplotype is not looked at
            (BIRTH, 3, 2, 0, 0),                                  # t = 2.2 after 2.5: the loop does not go back, bin 2
            (BIRTH, 0, 0, 0, 0),                                  # t = 3.999: bin 2
            (MIGRATION, 0, 0, 0, 1)]                              # t = 4.0 = edges[T]: after the window
    times = [0.5, 1.0, 1.5, 2.0] + [2.1] * 5 + [2.2] * 3 + [2.3] * 6 + [2.5, 2.2, 3.999, 4.0]
    assert len(times) == len(recs)
    cols = columns(recs)
    want = np.zeros((3, P, P, V), dtype=np.int64)
    want[0, 1, 1, 1] = want[0, 2, 2, 0] = want[1, 0, 1, 1] = want[2, 2, 0, 1] = want[2, 2, 2, 1] = want[2, 0, 0, 0] = 1
    across = want.copy()
    across[0, 1, 1, 1] = across[2, 2, 2, 1] = across[2, 0, 0, 0] = 0   # within = 0: the births go, the migration with equal keys stays
    for within, block in ((1, want), (0, across)):
        lit, lout = restate(times, cols, P, edges, vo, V, within)
        assert np.array_equal(lit, block) and lout.tolist() == [1, 1]
        for form in ("dense", "split", None):
            for tile in (1, 2, 3, 5, len(recs), 0):
                got, out, ran = hook(times, cols, P, H, edges, vo, V, within, tile, form)
                assert np.array_equal(got, block), (within, form, tile)
                assert out.tolist() == [1, 1] and ran == (form or "dense")
    empty, out, _ = hook([], columns([]), P, H, edges, vo, V)
    assert empty.shape == (3, P, P, V) and not empty.any() and out.tolist() == [0, 0]


# ---- refusals of the hook
def test_refusals_name_what_is_wrong():
    P, H = 2, 2
    one = columns([(BIRTH, 0, 0, 0, 0)])
    vo = np.zeros(H, dtype=np.int32)
    for edges in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], [0.0, float("inf")], [0.0]):
        with pytest.raises(ValueError, match="vgx_test_flows: (edges|T = 0)"):
            hook([0.1], one, P, H, np.array(edges), vo, 1)
    with pytest.raises(ValueError, match="vgx_test_flows: V = 0 must be at least 1"):
        hook([0.1], one, P, H, np.array([0.0, 1.0]), vo, 0)
    with pytest.raises(ValueError, match=r"vgx_test_flows: variant_of\[1\] = 2 is outside \[-1, 2\)"):
        hook([0.1], one, P, H, np.array([0.0, 1.0]), np.array([0, 2], dtype=np.int32), 2)
    with pytest.raises(ValueError, match=r"vgx_test_flows: variant_of\[0\] = -2 is outside \[-1, 2\)"):
        hook([0.1], one, P, H, np.array([0.0, 1.0]), np.array([-2, 0], dtype=np.int32), 2)
    with pytest.raises(ValueError, match="tile must not be negative"):
        hook([0.1], one, P, H, np.array([0.0, 1.0]), vo, 1, tile=-1)


def test_the_lds_budgets_are_refusals_that_name_the_bytes():
    edges = np.array([0.0, 1.0])
    # P = 70: 19600 bytes of dense cells with one class; 78400 with four, where the automatic choice is the split form
    cols = columns([(MIGRATION, 3, 69, 0, 68), (BIRTH, 2, 69, 0, 0)])
    vo = np.arange(4, dtype=np.int32)
    got, _, ran = hook([0.5, 0.6], cols, 70, 4, edges, vo, 4)
    assert ran == "split" and got[0, 69, 68, 3] == 1 and got[0, 69, 69, 2] == 1 and got.sum() == 2
    with pytest.raises(ValueError, match="vgx_test_flows: 70 populations x 4 classes need 78400 bytes of cells in the dense form, above the 65536 bytes"):
        hook([0.5, 0.6], cols, 70, 4, edges, vo, 4, form="dense")
    assert hook([0.5, 0.6], cols, 70, 4, edges, np.zeros(4, dtype=np.int32), 1)[2] == "dense"
    # the limits themselves: 128^2 * 4 = 65536 bytes of dense cells fit, 129^2 * 4 do not
    assert hook([], columns([]), 128, 1, edges, np.zeros(1, dtype=np.int32), 1)[2] == "dense"
    assert hook([], columns([]), 129, 1, edges, np.zeros(1, dtype=np.int32), 1)[2] == "split"
    # 4 P V over the budget: no form is left
    last = columns([(BIRTH, 16383, 0, 0, 0)])
    got, _, ran = hook([0.5], last, 1, 16384, edges, np.arange(16384, dtype=np.int32), 16384, form="split")
    assert ran == "split" and got[0, 0, 0, 16383] == 1 and got.sum() == 1
    for form in (None, "split"):
        with pytest.raises(ValueError, match="vgx_test_flows: 1 populations x 16385 classes need 65540 bytes of cells in the split form, above the 65536 bytes"):
            hook([0.5], last, 1, 16385, edges, np.arange(16385, dtype=np.int32), 16385, form=form)
    with pytest.raises(ValueError, match="form must be"):
        hook([0.5], last, 1, 1, edges, np.zeros(1, dtype=np.int32), 1, form="sparse")


# ---- the Flows object
def test_flows_methods_on_a_block_made_by_hand():
    from vgsim_amd.ensemble import Flows
    rng = np.random.default_rng(5)
    n, T, P, V = 2, 3, 4, 2
    fl = Flows()
    fl.counts = rng.integers(0, 9, (n, T, P, P, V)).astype(np.int32)
    fl.counts[0, 0, :, 2, 1] = 0                                   # no new infection of class 1 in population 2, bin 0 of replicate 0
    c = fl.counts.astype(np.int64)
    imports, exports, local, new = np.zeros((n, T, P, V), dtype=np.int64), np.zeros((n, T, P, V), dtype=np.int64), np.zeros((n, T, P, V), dtype=np.int64), np.zeros((n, T, P, V), dtype=np.int64)
    for s in range(P):
        for d in range(P):
            new[:, :, d] += c[:, :, s, d]
            if s == d:
                local[:, :, s] += c[:, :, s, d]
            else:
                imports[:, :, d] += c[:, :, s, d]
                exports[:, :, s] += c[:, :, s, d]
    assert np.array_equal(fl.imports(), imports) and np.array_equal(fl.exports(), exports)
    assert np.array_equal(fl.local(), local) and np.array_equal(fl.new_infections(), new)
    share = fl.imported_share()
    assert share.shape == (n, T, P, V) and np.isnan(share[0, 0, 2, 1]) and np.isnan(share).sum() == (new == 0).sum()
    assert np.array_equal(share[new > 0], imports[new > 0] / new[new > 0])


# ---- Ensemble.flows: refusals before the library
@pytest.mark.parametrize("kwargs, text", [
    (dict(), "either edges or bins"),
    (dict(edges=[0.0, 1.0], bins=4, window=(0, 1)), "either edges or bins"),
    (dict(bins=4), "window"),
    (dict(edges=[0.0, 1.0, 1.0]), "increase strictly"),
    (dict(edges=[0.0, float("nan")]), "finite"),
    (dict(edges=[0.0, 1.0], variants=[[40]]), "haplotype index out of range"),
    (dict(edges=[0.0, 1.0], variants=[[1], [1]]), "listed twice"),
    (dict(edges=[0.0, 1.0], variants=np.zeros(39, dtype=np.int64)), "one class per haplotype"),
    (dict(edges=[0.0, 1.0], variants=np.arange(40) * 1000), "3 populations x 39001 classes need 468012 bytes of cells"),
    (dict(edges=[0.0, 1.0], replicates=[0, 6]), "replicate index out of range"),
    (dict(edges=[0.0, 1.0], replicates=[1, 1]), "distinct"),
    (dict(edges=[0.0, 1.0], counts=False), "counts=False needs summary"),
    (dict(edges=[0.0, 1.0], summary=dict(quantiles=(1.5,))), "quantiles must lie in"),
    (dict(edges=[0.0, 1.0], summary=dict(ranks=3)), "summary takes"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(scenarios=2).flows(**kwargs)


@pytest.mark.parametrize("last, text", [(None, "simulate"), (('tau', True), "direct chains only"), (('direct', False), "record_events")])
def test_the_wrong_last_call_is_refused(last, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(last=last).flows(edges=[0.0, 1.0])
