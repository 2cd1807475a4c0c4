"""One tau-leap step of every draw path of the engine against the exact law (tests/tau_law.py).

R replicates of ONE step from ONE common state are R i.i.d. samples of a product of Poissons whose means the law gives in closed
form: a one-sample test per channel, where tests/test_hip_tau.py compares aggregates of whole runs between two samples.  Cases
(tau_law.CASES; tests/test_tau_step_law.py shows on the CPU that the oracle stays inside every bound used here and that no first try
is ever rejected):

  A  2 sites, 4 populations, non-uniform migration matrix with zero pairs, sampling multipliers, a lockdown that is ON, S = 2
  B  3 sites, 2 populations, per-site mutation rates, unequal weights and a zero-weight derived state, three rate classes
  C  1 site, 2 populations, S = 6: births into groups 4 and 5, susceptibility exactly 0, immunity transitions 4 <-> 5

each with compartments of about 20, 300, 3000 and 30 000 hosts, i.e. with < 1, 1-16, 16-64 and >= 64 expected events per step.

Paths: ``loop`` the on-device step loop of vgx_taus.hip (one draw per channel); ``steps`` the step kernels of vgx_tau.hip with the
thresholds of small models (VGX_TAU_STEP_KERNELS=1, launches of at most 2^18 / (P H) replicates: inversion search and multinomial
walk below a mean of 16, vgx_tau_draw_big_kernel from 16 on); ``large`` the step kernels with the thresholds of large models
(VGX_TAU_LARGE_MODEL_THRESHOLDS=1: the walk below 16, one draw per kind in [16, 64), the channel-by-channel kernel from 64 on).
The test asserts from the law's means that every one of these forms has compartments to draw.

R = 2^17 per (case, path) (tau_law.GPU_REPLICATES, derived there), in launches of 1024 replicates on one engine (a tau call keeps 32 MB of
cross-compartment list per replicate): 3 % on a channel of mean 0.5 and 1 % on a (kind, population) total of mean 3 fall outside the totals
bound; the resolution of every class is printed.  Case D (sparse states, two steps): the last test of this file.  Asserted per cell: 0 rejected tries and the oracle's tau (rel 1e-9)
for EVERY replicate, rows of zero-rate channels never, totals, dispersion, full pmf, independence, and the integer bookkeeping of every replicate.
Seeds are fixed and disjoint between launches; family-wise alpha = 1e-6 per statistic."""
import numpy as np
import pytest

import helpers
import tau_law as L

pytestmark = pytest.mark.gpu

PATHS = {"loop": {}, "steps": {"VGX_TAU_STEP_KERNELS": "1"}, "large": {"VGX_TAU_LARGE_MODEL_THRESHOLDS": "1"}}
SWITCHES = ("VGX_TAU_STEP_KERNELS", "VGX_TAU_LARGE_MODEL_THRESHOLDS", "VGX_TAU_NO_OCCLIST", "VGX_TAU_NO_FRONT")
SMALL_MODEL_CELLS = 1 << 18      # P H R up to which the step kernels switch to the channel-by-channel kernel at a mean of 16 (vgx_tau_run.hip)
LAUNCH = 1 << 10                 # replicates per launch: a tau call sizes its cross-compartment list at 2^22 entries (32 MB) per replicate


def _build(name):
    with helpers.quiet():
        return L.CASES[name]()


def _set_path(monkeypatch, path):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _launch(ens, seed0, ch, start, tau, first):
    """One launch of the ensemble (every replicate one step from the model's state, seeds seed0 ...): per-channel counts [n, K], after the
    per-replicate assertions."""
    from vgsim_amd import _capi
    m, n = ens.model, ens.R
    res = ens.simulate_tau(1, sample_size=10 ** 12, record_events=True, seeds=seed0 + np.arange(n, dtype=np.int64))
    assert (res.events == 2).all() and (res.restarts == 0).all(), "one step per replicate"
    off, rows = ens.replicate_multievents()
    inf, sus, cnt, t = ens.replicate_states_tau()
    tries = np.array([ens.engine.tau_tries(r, 0, 1)[0] for r in range(n)])
    probe = {r: ens.engine.multievents(r) for r in ((0, 1, n - 1) if first else ())}
    assert (tries == 0).all(), "replicate %d: %d rejected tries" % (np.argmax(tries != 0), tries.max())
    np.testing.assert_allclose(t, tau, rtol=1e-9, atol=0, err_msg="the leap of every replicate is the oracle's tau")
    assert (rows["num"] > 0).all() and (rows["steps"] == 0).all()
    rep = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    counts = L.counts_from_rows(ch, rep, rows["types"], rows["haplotypes"], rows["populations"], rows["newHaplotypes"], rows["newPopulations"],
                                rows["num"], n)
    if first:
        for r, one in probe.items():           # the batched read-out against the per-replicate one
            for k in ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations"):
                assert np.array_equal(one[k], rows[k][off[r]:off[r + 1]]), (r, k)
    if True:
        # the reference's order and granularity (as HipEngine._absorb forms them): every replicate as one step of a long log
        starts, ends = off[:-1].copy(), off[1:].copy()
        canon = _capi.canonical_multievents(dict(rows, times=np.zeros(len(rep))), starts, ends, m.sites, m.susNum)
        crep = np.repeat(np.arange(n, dtype=np.int64), ends - starts)
        again = L.counts_from_rows(ch, crep, canon["types"], canon["haplotypes"], canon["populations"], canon["newHaplotypes"],
                                   canon["newPopulations"], canon["num"], n)
        assert np.array_equal(again, counts), "canonical_multievents keeps every event on its channel"
        key = ch.key[ch.index_of(canon["types"], canon["haplotypes"], canon["populations"], canon["newHaplotypes"], canon["newPopulations"])]
        assert len(key) == int((counts > 0).sum()), "one canonical row per channel that fired"
    L.check_bookkeeping(ch, counts, start, m.suscType, inf, sus, cnt[:, :6])
    assert np.array_equal(cnt[:, 6], inf.sum(axis=(1, 2))) and (cnt[:, 7] == 2).all()
    return counts


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", sorted(L.CASES))
def test_one_step_follows_the_law(oracle_mod, monkeypatch, capsys, name, path):
    _set_path(monkeypatch, path)
    m0 = _build(name).simulation
    start = L.Snapshot(m0)
    ch = L.channel_table(m0)
    _, tau, tries_ref, _ = L.oracle_step(_build(name))
    assert tries_ref == 0
    mu = ch.rate * tau
    R = L.GPU_REPLICATES[name]
    q = L.first_try_rejection_bound(m0, ch, tau)
    assert q * R <= 0.01, "inadmissible case: q = %.3g" % q
    # every form of the path has compartments to draw
    lam = L.compartment_means(ch, mu)
    lam = lam[lam > 0]
    cells = m0.popNum * m0.hapNum
    n = LAUNCH
    if path == "steps":
        n = min(LAUNCH, SMALL_MODEL_CELLS // cells)
        assert cells * n <= SMALL_MODEL_CELLS and R % n == 0
        assert (lam < 1).any() and ((lam >= 1) & (lam < 16)).any() and (lam >= 16).any()
    else:
        L.check_regimes(ch, mu)
    lines = ["case %s, path %s: R = %d in launches of %d, tau = %.6g, q R = %.3g, compartment means %s" % (
        name, path, R, n, tau, q * R, np.round(np.sort(lam), 2).tolist())]
    case_no = sorted(L.CASES).index(name) * len(PATHS) + sorted(PATHS).index(path)
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(_build(name), n)
    try:
        counts = np.concatenate([_launch(ens, 10 ** 7 * (case_no + 1) + i * n, ch, start, tau, i == 0) for i in range(R // n)])
    finally:
        ens.close()
    # the resolution this R gives
    classes = L.pooled_classes(ch, mu, R)
    z, res = L.resolution(classes, mu, R)
    single = [res[i] for i, (_, idx) in enumerate(classes) if len(idx) == 1 and mu[idx[0]] >= 0.5]
    assert max(single) <= 0.03, "a 3 %% error on a channel of mean >= 0.5 must fall outside the bound: %.4f" % max(single)
    tot = [(lab, res[i], mu[idx].sum()) for i, (lab, idx) in enumerate(classes) if " total of " in lab]
    need = (z / 0.01) ** 2 / R
    assert all(r <= 0.01 for _, r, mean in tot if mean >= need)
    lines.append("resolution: z = %.2f; channels of mean >= 0.5: %.2f %% at worst; (kind, population) totals: 1 %% from a mean of %.2f on, else %s" % (
        z, 100 * max(single), need, ["%s: %.1f %%" % (lab, 100 * r) for lab, r, mean in tot if mean < need]))
    L.check_step_law(ch, mu, counts, report=lines.append)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------ case D: the sparse-state forms
D_PATHS = {   # environment, replicates per launch
    "single": ({}, 1),                 # one trajectory per call: the front pass on its own, speculative rounds, small-model thresholds (P H R <= 2^18)
    "ensemble": ({}, L.GPU_REPLICATES["D"]),   # all replicates in one call: their tries end at different places, large-model thresholds
    "no_occlist": ({"VGX_TAU_NO_OCCLIST": "1"}, 1),
    "no_front": ({"VGX_TAU_NO_FRONT": "1"}, 1),
    "large": ({"VGX_TAU_LARGE_MODEL_THRESHOLDS": "1"}, 1),
}


@pytest.mark.parametrize("path", sorted(D_PATHS))
def test_sparse_state_two_steps_follow_the_law(oracle_mod, monkeypatch, capsys, path):
    """Case D (7 sites: 16 384 haplotypes, 2 populations, 0.7 % of the compartments occupied), TWO steps per replicate: the tries over the
    lists of occupied compartments and the front pass in both, the sparse drift pass (which starts at a call's second step) in the second.
    Step one against the channel table of the common state (per channel where R resolves one, pooled otherwise); step two against the law's
    sums over each replicate's OWN state after step one (its first step's rows applied to the start state), pooled by (kind, population);
    the leap of step two against the oracle's ChooseTau for that state; 0 rejected tries in both steps of every replicate, with the
    bound on the rejection probability summed over the replicates' states <= 0.01; the integer bookkeeping over both steps.
    (VGX_TAU_STEP_KERNELS=1 changes nothing here: 32 768 compartments are beyond the on-device loop.)"""
    env, n = D_PATHS[path]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim = L.case_D()
    m0 = sim.simulation
    start = L.Snapshot(m0)
    ch = L.channel_table(m0)
    _, tau, tries_ref, _ = L.oracle_step(_build_d())
    assert tries_ref == 0
    mu = ch.rate * tau
    live = np.nonzero(mu > 0)[0]
    chl, mul = ch.subset(live), mu[live]
    R = L.GPU_REPLICATES["D"]
    assert m0.sites >= 7 and len(np.nonzero(m0.infectious)[0]) < 0.01 * m0.infectious.size
    assert L.first_try_rejection_bound(m0, chl, tau) * R <= 0.01
    L.check_regimes(chl, mul)
    cols = ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations", "steps")
    got = {k: [] for k in cols + ("rep",)}
    inf, sus, cnt, leaps, tries = [], [], [], [], []
    ens = Ensemble(sim, n)
    try:
        for i in range(R // n):
            res = ens.simulate_tau(2, sample_size=10 ** 12, record_events=True,
                                   seeds=4 * 10 ** 8 + 1000 * sorted(D_PATHS).index(path) + i * n + np.arange(n, dtype=np.int64))
            assert (res.events == 3).all() and (res.restarts == 0).all(), "two steps per replicate"
            off, rows = ens.replicate_multievents()
            for k in cols:
                got[k].append(rows[k])
            got["rep"].append(i * n + np.repeat(np.arange(n, dtype=np.int64), np.diff(off)))
            a, b, c, _ = ens.replicate_states_tau()
            inf.append(a); sus.append(b); cnt.append(c)
            for r in range(n):
                tries.append(ens.engine.tau_tries(r, 0, 2))
                t = ens.replicate_events(r)[0]
                leaps.append([t[1] - t[0], t[2] - t[1]])
    finally:
        ens.close()
    got = {k: np.concatenate(v) for k, v in got.items()}
    inf, sus, cnt, leaps, tries = np.concatenate(inf), np.concatenate(sus), np.concatenate(cnt), np.array(leaps), np.array(tries)
    assert (tries == 0).all(), "replicate %d: rejected tries %s" % (np.argmax(tries.any(axis=1)), tries[np.argmax(tries.any(axis=1))])
    np.testing.assert_allclose(leaps[:, 0], tau, rtol=1e-9, atol=0)
    assert (got["num"] > 0).all()
    args = lambda sel: (got["rep"][sel], got["types"][sel], got["haplotypes"][sel], got["populations"][sel], got["newHaplotypes"][sel],  # noqa: E731
                        got["newPopulations"][sel], got["num"][sel])
    # bookkeeping over both steps
    fi, fs, fc = L.apply_sparse_rows(*args(slice(None)), start.arrays["infectious"], start.arrays["susceptible"], m0.suscType, R)
    assert np.array_equal(fi, inf) and np.array_equal(fs, sus) and np.array_equal(fc, cnt[:, :6])
    # step one: the common state's channels
    s1 = got["steps"] == 0
    counts = L.counts_from_rows(ch, *args(s1), R, live=live)
    lines = ["case D, path %s: R = %d in launches of %d, tau = %.6g, %d channels with a positive rate" % (path, R, n, tau, len(live))]
    L.check_totals(chl, mul, counts.sum(axis=0, dtype=np.int64), R, report=lines.append)
    L.check_dispersion(chl, mul, counts, report=lines.append)
    L.check_correlations(chl, mul, counts, report=lines.append)
    # step two: every replicate's own state
    i1, x1, _ = L.apply_sparse_rows(*args(s1), start.arrays["infectious"], start.arrays["susceptible"], m0.suscType, R)
    scratch = _build_d()
    tau2 = np.array([L.oracle_tau(scratch, start, i1[r], x1[r]) for r in range(R)])
    np.testing.assert_allclose(leaps[:, 1], tau2, rtol=1e-9, atol=0, err_msg="the second leap is ChooseTau's for the replicate's state")
    q2 = sum(L.state_rejection_bound(scratch, i1[r], x1[r], tau2[r]) for r in range(R))
    assert q2 <= 0.01, "inadmissible second step: the replicates' rejection bounds sum to %.3g" % q2
    expected = (L.kind_population_rates(m0, i1, x1) * tau2[:, None, None]).sum(axis=0)
    observed = np.zeros((6, m0.popNum), dtype=np.int64)
    np.add.at(observed, (got["types"][~s1], got["populations"][~s1]), got["num"][~s1])
    lines.append("second step: sum of the rejection bounds %.3g" % q2)
    L.check_pooled_totals(observed, expected, report=lines.append)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def _build_d():
    with helpers.quiet():
        return L.case_D().simulation
