"""The law of one tau-leap step (tests/tau_law.py: plain numpy, written from the formulas) against the CPU oracle's draws.

The oracle is pinned draw for draw on fixtures recorded from the reference, so it is the authority both for the restatement of
the law (row keys, rates) and for the calibration of the statistics: the reference alone must stay inside every bound that the
GPU test (tests/test_hip_tau_step_law.py) then applies to the engine's draw paths.  Per case (tau_law.CASES: A a non-uniform
migration matrix, sampling multipliers and a lockdown; B per-site mutation rates with unequal weights and three rate classes;
C six susceptibility groups), from ONE common start state (the sparse case D of 16 384 haplotypes: 64 seeds, totals only, last test):

* the oracle's dense multievent block names the channels of ``channel_table`` in the same order (row keys equal);
* admissibility: the bound q on the probability that a replicate's first try is rejected satisfies q R <= 0.01 for the R of the
  GPU test, every oracle run reports 0 rejected tries, and every run's leap is the same tau;
* N = 16384 seeds of one step: zero-rate channels never fire, totals (exact Poisson tails), dispersion, full pmf per kind and mean
  regime, independence of kinds and of neighbouring compartments, and the integer bookkeeping of every run;
* all four mean regimes (< 1, 1-16, 16-64, >= 64 events per compartment and step) are present in every case's state.

Family-wise alpha = 1e-6 per statistic (fixed seeds).  Wall time: about 10 s per case on one core (N = 16384; 0.5 ms per oracle step
with its Python hand-over)."""
import numpy as np
import pytest

import helpers
import tau_law as L

N = 16384


def _build(name):
    with helpers.quiet():
        return L.CASES[name]().simulation


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_oracle_step_follows_the_law(oracle_mod, name, capsys):
    m = _build(name)
    start = L.Snapshot(m)
    ch = L.channel_table(m)
    K = len(ch)
    assert K == oracle_mod.prop_num(m)
    lines = []
    counts = np.zeros((N, K), dtype=np.int32)
    final_i = np.zeros((N,) + m.infectious.shape, dtype=np.int64)
    final_s = np.zeros((N,) + m.susceptible.shape, dtype=np.int64)
    counters = np.zeros((N, 6), dtype=np.int64)
    tau = None
    for r in range(N):
        start.restore(m)
        num, leap, tries, mev = L.oracle_step(m, seed=1000 + r)
        if tau is None:
            tau = leap
            for col, attr in (("types", "kind"), ("haplotypes", "hap"), ("populations", "pop"), ("newHaplotypes", "nh"), ("newPopulations", "npop")):
                assert np.array_equal(mev[col][:K], getattr(ch, attr)), "row keys: column %s" % col
        assert tries == 0, "seed %d: %d rejected tries" % (1000 + r, tries)
        assert leap == pytest.approx(tau, rel=1e-9)
        counts[r] = num
        final_i[r], final_s[r] = m.infectious, m.susceptible
        counters[r] = [m.bCounter, m.dCounter, m.sCounter, m.mCounter, m.iCounter, m.migPlus]
    mu = ch.rate * tau
    q = L.first_try_rejection_bound(_build(name), ch, tau)
    assert q * max(N, L.GPU_REPLICATES[name]) <= 0.01, "inadmissible case: q = %.3g" % q
    regimes = L.check_regimes(ch, mu)
    lines.append("case %s: K = %d channels (%d with a positive rate), tau = %.6g, q = %.3g, compartments per regime %s" % (
        name, K, int((mu > 0).sum()), tau, q, {r: len(v) for r, v in sorted(regimes.items())}))
    L.check_bookkeeping(ch, counts, start, m.suscType, final_i, final_s, counters)
    L.check_step_law(ch, mu, counts, report=lines.append)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_poisson_tails_against_direct_sums():
    """The log-space tails of the helper against plain sums of the pmf (math.lgamma per term), on both sides of the mean."""
    import math
    for mu in (0.3, 7.0, 150.0, 9000.0):
        pmf = [math.exp(-mu + k * math.log(mu) - math.lgamma(k + 1.0)) for k in range(int(mu + 60 * math.sqrt(mu) + 80))]
        for x in (0, int(mu * 0.9), int(mu), int(mu + 1), int(mu + 4 * math.sqrt(mu) + 3)):
            assert L.poisson_cdf(x, mu) == pytest.approx(sum(pmf[:x + 1]), rel=1e-9, abs=1e-300)
            assert L.poisson_sf(x, mu) == pytest.approx(sum(pmf[x + 1:]), rel=1e-9, abs=1e-300)
    assert L.poisson_two_sided(0, 0.0) == 1.0 and L.poisson_two_sided(1, 0.0) == 0.0
    assert L.z_of(0.0026997960632601866) == pytest.approx(3.0, abs=1e-9)


def test_statistics_catch_a_wrong_sampler():
    """The statistics on synthetic draws (numpy's sampler): the exact law passes; 3 % more on one channel of mean 0.5, a mean-preserving
    variance inflation, and a copy of one kind's count into another each fail the statistic made for it."""
    m = _build("C")
    ch = L.channel_table(m)
    _, tau, _, _ = L.oracle_step(_build("C"))
    mu = ch.rate * tau
    R = L.GPU_REPLICATES["C"]
    rng = np.random.default_rng(12345)
    counts = rng.poisson(mu[None, :], size=(R, len(ch))).astype(np.int32)
    L.check_step_law(ch, mu, counts)
    c = int(np.argmin(np.where(mu >= 0.5, mu, np.inf)))                     # the smallest channel the resolution is stated for
    bad = counts.copy()
    bad[:, c] = rng.poisson(1.03 * mu[c], size=R)
    with pytest.raises(AssertionError, match="total of"):
        L.check_totals(ch, mu, bad.sum(axis=0, dtype=np.int64), R)
    bad = counts.copy()
    big = int(np.argmax(mu))
    bad[:, big] = rng.poisson(rng.gamma(400.0, mu[big] / 400.0, size=R))     # same mean, variance mu (1 + mu / 400)
    with pytest.raises(AssertionError, match="dispersion of"):
        L.check_dispersion(ch, mu, bad)
    with pytest.raises(AssertionError, match="pmf of"):
        L.check_pmf("x", bad[:, big], float(mu[big]), L.ALPHA, 1)
    comp = int(ch.comp[big])
    rec = int(np.nonzero((ch.comp == comp) & (ch.kind == L.DEATH))[0][0])
    bad = counts.copy()
    bad[:, rec] = rng.poisson(mu[rec], size=R) // 2 + (counts[:, big] * (mu[rec] / mu[big]) / 2).astype(np.int32)
    with pytest.raises(AssertionError, match="correlation"):
        L.check_correlations(ch, mu, bad)


def test_sparse_case_oracle_totals_and_admissibility(oracle_mod, capsys):
    """Case D (16 384 haplotypes, 0.7 % of the compartments occupied): 64 oracle seeds, totals only (the law's code is shape-independent).
    Step one from the common state against the channel table; then the oracle's own second step from every run's state against the
    closed-form sums of the law over that state, pooled by (kind, population) — the form the GPU test uses — with the admissibility of
    both steps: q R <= 0.01 for the first, the sum of the states' bounds scaled to the GPU test's R for the second."""
    n = 64
    m = _build_case_d()
    start = L.Snapshot(m)
    ch = L.channel_table(m)
    assert len(ch) == oracle_mod.prop_num(m)
    R = L.GPU_REPLICATES["D"]
    tau = None
    rows = {k: [] for k in ("rep", "kind", "hap", "pop", "nh", "npop", "num")}
    states, obs2, exp2, q2 = [], np.zeros((6, m.popNum), dtype=np.int64), np.zeros((6, m.popNum)), 0.0
    for r in range(n):
        start.restore(m)
        num, leap, tries, mev = L.oracle_step(m, seed=3000 + r)
        if tau is None:
            tau = leap
            for col, attr in (("types", "kind"), ("haplotypes", "hap"), ("populations", "pop"), ("newHaplotypes", "nh"), ("newPopulations", "npop")):
                assert np.array_equal(mev[col][:len(ch)], getattr(ch, attr)), "row keys: column %s" % col
        assert tries == 0 and leap == pytest.approx(tau, rel=1e-9)
        c = np.nonzero(num)[0]
        for k, v in (("rep", np.full(len(c), r)), ("kind", ch.kind[c]), ("hap", ch.hap[c]), ("pop", ch.pop[c]), ("nh", ch.nh[c]), ("npop", ch.npop[c]), ("num", num[c])):
            rows[k].append(v)
        I1, X1 = m.infectious.copy(), m.susceptible.copy()
        states.append((I1, X1))
        # the second step, from this run's own state
        L.set_state(m, start, I1, X1)
        num2, leap2, tries2, _ = L.oracle_step(m)
        assert tries2 == 0, "seed %d: the second step had %d rejected tries" % (3000 + r, tries2)
        exp2 += L.kind_population_rates(m, I1[None], X1[None])[0] * leap2
        np.add.at(obs2, (ch.kind, ch.pop), num2)
        q2 += L.state_rejection_bound(m, I1, X1, leap2)
    rows = {k: np.concatenate(v) for k, v in rows.items()}
    mu = ch.rate * tau
    live = np.nonzero(mu > 0)[0]
    assert len(np.nonzero(m.infectious)[0]) < 0.01 * m.infectious.size
    chl = ch.subset(live)
    counts = L.counts_from_rows(ch, rows["rep"], rows["kind"], rows["hap"], rows["pop"], rows["nh"], rows["npop"], rows["num"], n, live=live)
    inf, sus, cnt = L.apply_sparse_rows(rows["rep"], rows["kind"], rows["hap"], rows["pop"], rows["nh"], rows["npop"], rows["num"],
                                        start.arrays["infectious"], start.arrays["susceptible"], m.suscType, n)
    for r, (I1, X1) in enumerate(states):
        assert np.array_equal(inf[r], I1) and np.array_equal(sus[r], X1), r
    q = L.first_try_rejection_bound(_build_case_d(), chl, tau)
    assert q * R <= 0.01 and q2 / n * R <= 0.01, (q, q2 / n)
    # the closed-form sums are the table's sums
    sums = L.kind_population_rates(m, start.arrays["infectious"][None], start.arrays["susceptible"][None])[0]
    for k in range(6):
        for pn in range(m.popNum):
            assert sums[k, pn] == pytest.approx(ch.rate[(ch.kind == k) & (ch.pop == pn)].sum(), rel=1e-12)
    L.check_regimes(chl, mu[live])
    lines = ["case D: %d channels, %d with a positive rate, tau = %.6g, q = %.3g, mean bound of the second step %.3g" % (len(ch), len(live), tau, q, q2 / n)]
    L.check_totals(chl, mu[live], counts.sum(axis=0, dtype=np.int64), n, report=lines.append)
    L.check_pooled_totals(obs2, exp2, report=lines.append)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def _build_case_d():
    with helpers.quiet():
        return L.case_D().simulation
