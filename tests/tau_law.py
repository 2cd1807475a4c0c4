"""The exact law of ONE tau-leap step, in plain numpy, and the statistics that test an engine's draws against it.

Given the state and the leap ``tau`` (both deterministic) the reference draws one independent ``Poisson(a_c * tau)`` per channel
``c`` (propensities pyx:2351-2417, draws pyx:2454-2529) and logs channel ``c`` under exactly one multievent row
``(type, haplotype, population, newHaplotype, newPopulation)`` (pyx:2536-2593).  R replicates of one step from one common state
are therefore R i.i.d. samples of a product of Poissons with known means.  This module holds

* ``channel_table`` / ``channel_means``: every channel's row key and rate ``a_c`` in float64, written from the formulas (no sampling
  code); the derived quantities of the model that enter them (``effectiveMigration``, ``actualSizes``) come from the oracle's
  ``update_all_rates``, the rest from the model object;
* ``first_try_rejection_bound``: an upper bound on the probability that a replicate's first try is rejected (a rejected try, pyx:2316-2321,
  halves tau and redraws: the accepted draw would then be conditioned, and the law above would no longer be exact);
* the statistics — all of them derived from the law; no constant here is fitted to an engine's output:

  - ``check_totals``   two-sided exact Poisson tail of every channel's total over the replicates (small channels pooled, never dropped);
  - ``check_dispersion`` index of dispersion against chi-square(R - 1);
  - ``check_pmf``      chi-square of a channel's counts against the exact Poisson pmf;
  - ``check_correlations`` sample correlations of counts that Poisson splitting makes independent;
  - ``apply_rows``    the integer bookkeeping of a step (state and counters from the rows);

* the cases (start states written straight into the arrays) shared by the CPU test (oracle against the law) and the GPU test (every draw
  path of the engine against the law).

Family-wise error: every test function takes ``alpha`` and tests each of its K hypotheses at ``alpha / K`` (Bonferroni).
"""
import math
from statistics import NormalDist

import numpy as np

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
KIND_NAMES = ("BIRTH", "DEATH", "SAMPLING", "MUTATION", "SUSCCHANGE", "MIGRATION")
ALPHA = 1e-6          # family-wise, per test function (fixed seeds: a correct engine fails with this probability once, not per run)


# ------------------------------------------------------------------------------------------------ the law
def mutate(sites, hn, s, i):
    """Haplotype reached from ``hn`` by the i-th (0..2) derived state of site ``s`` (pyx:2420-2427); numpy arrays allowed."""
    digit4 = 4 ** (sites - s - 1)
    AS = (hn // digit4) % 4
    DS = i + (i >= AS)
    return hn + (DS - AS) * digit4


class Channels:
    """All channels of a model in the reference's order (pyx:2540-2593): ``kind, hap, pop, nh, npop`` (the row a channel is logged
    under) and ``rate`` (a_c, events per unit time).  ``comp`` is the infectious compartment ``pop * H + hap`` that emits the channel
    (-1 for immunity transitions), ``sub`` tells a compartment's kinds apart for the independence test (0 recovery, 1 sampling,
    2 mutation, 3 migration, 4 + sn birth into group sn)."""

    def __init__(self, kind, hap, pop, nh, npop, rate, comp, sub, dims):
        self.kind, self.hap, self.pop, self.nh, self.npop = kind, hap, pop, nh, npop
        self.rate, self.comp, self.sub = rate, comp, sub
        self.sites, self.H, self.P, self.S = dims
        self.key = row_key(kind, hap, pop, nh, npop, self.H, self.P, self.S)
        self.order = np.argsort(self.key, kind="stable")
        self.sorted_key = self.key[self.order]
        assert (np.diff(self.sorted_key) > 0).all(), "two channels under one row key"

    def __len__(self):
        return len(self.kind)

    def index_of(self, kind, hap, pop, nh, npop):
        """Channel index of every row; -1 for a row that names no channel."""
        k = row_key(kind, hap, pop, nh, npop, self.H, self.P, self.S)
        j = np.searchsorted(self.sorted_key, k)
        j[j >= len(self.sorted_key)] = 0
        return np.where(self.sorted_key[j] == k, self.order[j], -1)

    def subset(self, keep):
        """The channels ``keep`` (index array) as a table of their own (row keys unchanged)."""
        return Channels(self.kind[keep], self.hap[keep], self.pop[keep], self.nh[keep], self.npop[keep], self.rate[keep], self.comp[keep],
                        self.sub[keep], (self.sites, self.H, self.P, self.S))

    def label(self, c):
        return "%s(hap %d, pop %d, new %d, newpop %d)" % (KIND_NAMES[self.kind[c]], self.hap[c], self.pop[c], self.nh[c], self.npop[c])


def row_key(kind, hap, pop, nh, npop, H, P, S):
    w = max(H, S)
    return (((np.asarray(kind, dtype=np.int64) * w + hap) * P + pop) * w + nh) * P + npop


def derived_rates(model):
    """effectiveMigration [P, P] and actualSizes [P] as the oracle's update_all_rates (pyx:279-351) leaves them; it also writes the
    diagonal of ``migrationRates`` (1 - the row's off-diagonal sum) into the model, as the reference does before every simulation."""
    from oracle import oracle
    st = oracle.update_all_rates(model)
    return st.effectiveMigration.copy(), model.actualSizes.copy()


def channel_table(model, infectious=None, susceptible=None):
    """The channels of ``model`` with their rates for the state (``infectious`` [P, H], ``susceptible`` [P, S]; default: the model's)."""
    m = model
    sites, H, P, S = int(m.sites), int(m.hapNum), int(m.popNum), int(m.susNum)
    eff, actual = derived_rates(m)
    I = np.asarray(m.infectious if infectious is None else infectious, dtype=np.float64)
    X = np.asarray(m.susceptible if susceptible is None else susceptible, dtype=np.float64)
    b, d, s_ = m.bRate.astype(np.float64), m.dRate.astype(np.float64), m.sRate.astype(np.float64)
    susc = m.susceptibility.astype(np.float64)                # [H, S]
    mig = m.migrationRates.astype(np.float64)                 # [P, P], diagonal = share that stays
    cd = m.contactDensity.astype(np.float64)
    hn = np.arange(H, dtype=np.int64)
    cols = {k: [] for k in ("kind", "hap", "pop", "nh", "npop", "rate", "comp", "sub")}

    def add(kind, hap, pop, nh, npop, rate, comp, sub):
        n = len(np.atleast_1d(rate))
        for k, v in (("kind", kind), ("hap", hap), ("pop", pop), ("nh", nh), ("npop", npop), ("comp", comp), ("sub", sub)):
            cols[k].append(np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)))
        cols["rate"].append(np.broadcast_to(np.asarray(rate, dtype=np.float64), (n,)))

    # migration (pyx:2366-2367): a host of group sn in the TARGET population tpn is infected by haplotype hn of the SOURCE population spn
    for spn in range(P):
        for tpn in range(P):
            if spn == tpn:
                continue
            for sn in range(S):
                a = eff[tpn, spn] * X[tpn, sn] * I[spn] * b * susc[:, sn] * mig[spn, spn]
                add(MIGRATION, hn, spn, sn, tpn, a, spn * H + hn, 3)
    # transmission inside a population (pyx:2412-2414): contacts wherever both hosts may be (every population spn they both visit)
    contact = ((mig * mig) * (cd / actual)[None, :]).sum(axis=1)            # [P]: sum over spn of m[tpn, spn]^2 cd[spn] / actualSizes[spn]
    per_hap = 2 + 3 * sites + S
    for pn in range(P):
        for ssn in range(S):                                                # immunity transitions (pyx:2376-2378)
            for tsn in range(S):
                if ssn != tsn:
                    add(SUSCCHANGE, ssn, pn, tsn, 0, [m.suscepTransition[ssn, tsn] * X[pn, ssn]], -1, 0)
        blk = {k: np.zeros((H, per_hap), dtype=np.int64) for k in ("kind", "nh", "sub")}
        rate = np.zeros((H, per_hap))
        blk["kind"][:, 0], blk["nh"][:, 0], blk["sub"][:, 0] = DEATH, m.suscType, 0
        rate[:, 0] = d * I[pn]                                              # recovery (pyx:2386)
        blk["kind"][:, 1], blk["nh"][:, 1], blk["sub"][:, 1] = SAMPLING, m.suscType, 1
        rate[:, 1] = s_ * I[pn] * m.samplingMultiplier[pn]                  # sampling (pyx:2392)
        for s in range(sites):                                              # mutation (pyx:2400-2401)
            w = m.hapMutType[:, s, :].astype(np.float64)
            for i in range(3):
                j = 2 + 3 * s + i
                blk["kind"][:, j], blk["nh"][:, j], blk["sub"][:, j] = MUTATION, mutate(sites, hn, s, i), 2
                rate[:, j] = m.mRate[:, s] * w[:, i] / w.sum(axis=1) * I[pn]
        for sn in range(S):
            j = 2 + 3 * sites + sn
            blk["kind"][:, j], blk["nh"][:, j], blk["sub"][:, j] = BIRTH, sn, 4 + sn
            rate[:, j] = b * susc[:, sn] * contact[pn] * X[pn, sn] * I[pn]
        hap = np.repeat(hn, per_hap)
        add(blk["kind"].ravel(), hap, pn, blk["nh"].ravel(), 0, rate.ravel(), pn * H + hap, blk["sub"].ravel())
    out = {k: np.concatenate(v) for k, v in cols.items()}
    return Channels(out["kind"], out["hap"], out["pop"], out["nh"], out["npop"], out["rate"], out["comp"], out["sub"], (sites, H, P, S))


def channel_means(model):
    """dict: row key (type, haplotype, population, newHaplotype, newPopulation) -> a_c."""
    ch = channel_table(model)
    return {(int(k), int(h), int(p), int(n), int(q)): float(a)
            for k, h, p, n, q, a in zip(ch.kind, ch.hap, ch.pop, ch.nh, ch.npop, ch.rate)}


# ------------------------------------------------------------------------------------------------ Poisson tails
def _log_pmf_range(mu, lo, hi):
    """log P(X = k), k = lo..hi, X ~ Poisson(mu): -mu + k log mu - lgamma(k + 1), the lgamma by a running sum of logs."""
    ks = np.arange(lo, hi + 1, dtype=np.float64)
    lg = math.lgamma(lo + 1.0) + np.concatenate(([0.0], np.cumsum(np.log(ks[1:])))) if len(ks) > 1 else np.array([math.lgamma(lo + 1.0)])
    return -mu + ks * math.log(mu) - lg


def poisson_sf(k, mu):
    """P(X > k) (k >= -1), summed in log space from k + 1 upwards until the terms no longer matter."""
    if mu <= 0.0:
        return 0.0
    k = int(k)
    if k < 0:
        return 1.0
    if k < mu:
        return 1.0 - poisson_cdf(k, mu)
    if k > 20.0 * mu + 200.0:       # far tail: the Chernoff bound exp(-mu) (e mu / k)^k, an UPPER bound (used by the admissibility bound only)
        return math.exp(min(0.0, k - mu + k * math.log(mu / k)))
    hi = int(max(k + 1, mu) + 40.0 * math.sqrt(max(mu, k + 1.0)) + 60)
    lp = _log_pmf_range(mu, k + 1, hi)
    mx = lp.max()
    return float(min(1.0, math.exp(mx) * np.exp(lp - mx).sum()))


def poisson_cdf(k, mu):
    """P(X <= k), summed in log space."""
    if k < 0:
        return 0.0
    if mu <= 0.0:
        return 1.0
    k = int(k)
    if k > mu:
        return 1.0 - poisson_sf(k, mu)
    lo = int(max(0, min(k, mu) - 40.0 * math.sqrt(max(mu, 1.0)) - 60))
    lp = _log_pmf_range(mu, lo, k)
    mx = lp.max()
    return float(min(1.0, math.exp(mx) * np.exp(lp - mx).sum()))


def poisson_two_sided(x, mu):
    """Two-sided tail probability of an observed Poisson(mu) count x: 2 min(P(X <= x), P(X >= x)), capped at 1.  Exact (log-space
    sums) up to a mean of 10^4, the normal approximation (relative error of the tail below a per cent there) beyond."""
    if mu <= 0.0:
        return 1.0 if x == 0 else 0.0
    if mu > 1.0e4:
        return math.erfc(abs(x - mu) / math.sqrt(2.0 * mu))
    return min(1.0, 2.0 * min(poisson_cdf(x, mu), poisson_sf(x - 1, mu)))


def z_of(p_two_sided):
    """Normal quantile z with P(|Z| > z) = p."""
    return NormalDist().inv_cdf(1.0 - 0.5 * p_two_sided)


def wilson_hilferty(dof, z):
    """chi-square(dof) quantile at normal deviate z (Wilson-Hilferty, as tests/test_samplers.py)."""
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


# ------------------------------------------------------------------------------------------------ admissibility
def first_try_rejection_bound(model, ch, tau):
    """Upper bound q on the probability that a replicate's first try is rejected (GenerateEvents_tau's bounds, pyx:2522-2528): a
    compartment falls below zero only if its OUT channels draw more than it holds, and rises above ``sizes[pn]`` only if its IN
    channels draw more than the room left; union bound over all infectious and susceptible compartments.  (The reference books a
    migrant on its SOURCE compartment in that check, pyx:2473: counted as an arrival there.)"""
    H, P, S = ch.H, ch.P, ch.S
    I, X = np.asarray(model.infectious), np.asarray(model.susceptible)
    out_i, in_i = np.zeros(P * H), np.zeros(P * H)
    out_s, in_s = np.zeros(P * S), np.zeros(P * S)
    k, a = ch.kind, ch.rate
    sel = (k == DEATH) | (k == SAMPLING)
    np.add.at(out_i, ch.comp[sel], a[sel])
    np.add.at(in_s, ch.pop[sel] * S + ch.nh[sel], a[sel])
    sel = k == MUTATION
    np.add.at(out_i, ch.comp[sel], a[sel])
    np.add.at(in_i, ch.pop[sel] * H + ch.nh[sel], a[sel])
    sel = k == BIRTH
    np.add.at(in_i, ch.comp[sel], a[sel])
    np.add.at(out_s, ch.pop[sel] * S + ch.nh[sel], a[sel])
    sel = k == MIGRATION
    np.add.at(in_i, ch.comp[sel], a[sel])
    np.add.at(out_s, ch.npop[sel] * S + ch.nh[sel], a[sel])
    sel = k == SUSCCHANGE
    np.add.at(out_s, ch.pop[sel] * S + ch.hap[sel], a[sel])
    np.add.at(in_s, ch.pop[sel] * S + ch.nh[sel], a[sel])
    q = 0.0
    for out, inn, cnt, n in ((out_i, in_i, I.reshape(-1), H), (out_s, in_s, X.reshape(-1), S)):
        size = np.repeat(np.asarray(model.sizes), n)
        for c in np.nonzero(out > 0)[0]:
            q += poisson_sf(int(cnt[c]), out[c] * tau)
        for c in np.nonzero(inn > 0)[0]:
            q += poisson_sf(int(size[c] - cnt[c]), inn[c] * tau)
    return q


# ------------------------------------------------------------------------------------------------ rows -> counts, bookkeeping
def counts_from_rows(ch, rep, kind, hap, pop, nh, npop, num, R, live=None):
    """Dense [R, K] int32 channel counts from sparse rows (``rep``: the replicate of every row).  A row that names no channel
    fails at once.  ``live``: the channels (index array) that get a column — large sparse models, whose other channels have rate 0:
    a row on one of those fails as well."""
    idx = ch.index_of(kind, hap, pop, nh, npop)
    bad = np.nonzero(idx < 0)[0]
    assert len(bad) == 0, "row (%d, %d, %d, %d, %d) of replicate %d names no channel of the model" % (
        kind[bad[0]], hap[bad[0]], pop[bad[0]], nh[bad[0]], npop[bad[0]], rep[bad[0]])
    K = len(ch)
    if live is not None:
        col = np.full(K, -1, dtype=np.int64)
        col[live] = np.arange(len(live))
        bad = np.nonzero(col[idx] < 0)[0]
        assert len(bad) == 0, "replicate %d: %d events on %s, whose rate is 0" % (rep[bad[0]], num[bad[0]], ch.label(idx[bad[0]]))
        idx, K = col[idx], len(live)
    flat = np.bincount(np.asarray(rep, dtype=np.int64) * K + idx, weights=np.asarray(num, dtype=np.float64), minlength=R * K)
    return np.rint(flat).astype(np.int32).reshape(R, K)


def effect_matrices(ch, suscType):
    """[K, P*H] and [K, P*S]: what ONE event of channel c adds to infectious / susceptible (UpdateCompartmentCounts_tau, pyx:2536-2593:
    a migrant infects the TARGET population; a mutant moves to Mutate(hn, s, i); a recovered or sampled host joins group suscType[hn])."""
    H, P, S, K = ch.H, ch.P, ch.S, len(ch)
    EI, ES = np.zeros((K, P * H)), np.zeros((K, P * S))
    c = np.arange(K)
    k = ch.kind
    sel = k == MIGRATION
    EI[c[sel], ch.npop[sel] * H + ch.hap[sel]] += 1
    ES[c[sel], ch.npop[sel] * S + ch.nh[sel]] -= 1
    sel = k == SUSCCHANGE
    ES[c[sel], ch.pop[sel] * S + ch.nh[sel]] += 1
    ES[c[sel], ch.pop[sel] * S + ch.hap[sel]] -= 1
    sel = (k == DEATH) | (k == SAMPLING)
    EI[c[sel], ch.pop[sel] * H + ch.hap[sel]] -= 1
    ES[c[sel], ch.pop[sel] * S + np.asarray(suscType)[ch.hap[sel]]] += 1
    sel = k == MUTATION
    EI[c[sel], ch.pop[sel] * H + ch.nh[sel]] += 1
    EI[c[sel], ch.pop[sel] * H + ch.hap[sel]] -= 1
    sel = k == BIRTH
    EI[c[sel], ch.pop[sel] * H + ch.hap[sel]] += 1
    ES[c[sel], ch.pop[sel] * S + ch.nh[sel]] -= 1
    return EI, ES


def apply_rows(ch, counts, model0_infectious, model0_susceptible, suscType):
    """Final infectious [R, P, H], susceptible [R, P, S] and the six counters [R, 6] (by kind) that the rows of every replicate
    give from the common start state.  Integer arithmetic carried in float64 (exact below 2^53)."""
    if getattr(ch, "_effects", None) is None:      # (kept with the table: the GPU test applies them launch by launch)
        byk = np.zeros((len(ch), 6))
        byk[np.arange(len(ch)), ch.kind] = 1
        ch._effects = effect_matrices(ch, suscType) + (byk,)
    EI, ES, byk = ch._effects
    fired = np.nonzero(counts.any(axis=0))[0]          # (most channels of a sparse state never fire: their rows of the matrices are left out)
    x = counts[:, fired].astype(np.float64)
    EI, ES, byk = EI[fired], ES[fired], byk[fired]
    inf = np.rint(x @ EI).astype(np.int64) + np.asarray(model0_infectious, dtype=np.int64).reshape(1, -1)
    sus = np.rint(x @ ES).astype(np.int64) + np.asarray(model0_susceptible, dtype=np.int64).reshape(1, -1)
    cnt = np.rint(x @ byk).astype(np.int64)
    return inf.reshape(-1, ch.P, ch.H), sus.reshape(-1, ch.P, ch.S), cnt


# ------------------------------------------------------------------------------------------------ the statistics
def pooled_classes(ch, mu, R, floor=50.0):
    """The hypotheses of the totals test: every channel with R mu >= floor on its own, the smaller ones pooled by (kind, population)
    (sums of independent Poissons are Poisson: nothing is dropped), and every (kind, population) total.  Returns a list of
    (label, channel index array)."""
    out = []
    live = mu > 0
    big = live & (R * mu >= floor)
    for c in np.nonzero(big)[0]:
        out.append((ch.label(c), np.array([c])))
    for k in range(6):
        for pn in range(ch.P):
            sel = (ch.kind == k) & (ch.pop == pn) & live
            small = np.nonzero(sel & ~big)[0]
            if len(small):
                out.append(("%s small channels of population %d (%d pooled)" % (KIND_NAMES[k], pn, len(small)), small))
            if sel.any():
                out.append(("%s total of population %d" % (KIND_NAMES[k], pn), np.nonzero(sel)[0]))
    return out


def resolution(classes, mu, R, alpha=ALPHA):
    """Relative error of a class's mean that falls outside the totals bound: z(alpha / K) sqrt(1 / (R mean)), per class."""
    z = z_of(alpha / len(classes))
    return z, np.array([z * math.sqrt(1.0 / (R * mu[idx].sum())) for _, idx in classes])


def check_zero_channels(ch, mu, totals):
    """A row whose channel has mean 0 (zero weight, zero susceptibility, empty source) must never appear: exact."""
    dead = np.nonzero((mu == 0) & (totals != 0))[0]
    assert len(dead) == 0, "%d events on %s, whose rate is 0" % (totals[dead[0]], ch.label(dead[0]))


def check_totals(ch, mu, totals, R, alpha=ALPHA, report=None):
    """``totals[c]``: channel c's count summed over R replicates, exactly Poisson(R mu_c).  Fails when a class's two-sided tail
    probability is below alpha / K."""
    classes = pooled_classes(ch, mu, R)
    K = len(classes)
    worst = (1.0, None)
    for label, idx in classes:
        m, x = R * float(mu[idx].sum()), int(totals[idx].sum())
        p = poisson_two_sided(x, m)
        if p < worst[0]:
            worst = (p, (label, x, m))
        assert p >= alpha / K, "total of %s: %d observed, %.6g expected (relative %.3g), two-sided tail %.3g < %.3g (K = %d)" % (
            label, x, m, x / m - 1.0, p, alpha / K, K)
    if report is not None:
        report("totals: K = %d, smallest tail %.3g at %s" % (K, worst[0], worst[1]))
    return K




def dispersion_classes(ch, mu, floor=0.05):
    """Channels with mean >= floor on their own; the smaller ones pooled by (kind, population) if the pool reaches the floor."""
    out = []
    big = mu >= floor
    for c in np.nonzero(big)[0]:
        out.append((ch.label(c), np.array([c])))
    for k in range(6):
        for pn in range(ch.P):
            small = np.nonzero((ch.kind == k) & (ch.pop == pn) & (mu > 0) & ~big)[0]
            if len(small) and mu[small].sum() >= floor:
                out.append(("%s small channels of population %d (%d pooled)" % (KIND_NAMES[k], pn, len(small)), small))
    return out


def check_dispersion(ch, mu, counts, alpha=ALPHA, report=None):
    """Index of dispersion D = sum_r (x_r - mean)^2 / mean, two-sided against chi-square(R - 1) (Wilson-Hilferty), for every channel or
    pooled class with mean >= 0.05: a splitter whose counts have the right mean and the wrong variance.

    ``mean`` is the SAMPLE mean in both places.  Conditional on the class's total T the R counts of a Poisson sample are
    multinomial(T; 1/R, ..., 1/R) and D is that multinomial's Pearson statistic: mean R - 1, variance 2 (R - 1)(1 - 1/T), i.e.
    chi-square(R - 1) to second order at ANY mean.  With the law's mean a tau in the denominator instead, D is multiplied by
    (sample mean / a tau) and its variance becomes (R - 1)(2 + 1 / (a tau)): at a mean of 0.05 eleven times chi-square's, so that a
    correct sampler would exceed the bound routinely.  The mean itself is what check_totals bounds, exactly."""
    R = counts.shape[0]
    # ... and an expected total of at least 0.05 * 2^14 events (the floor above at the smallest ensemble it was set for): with few events
    # the Pearson statistic is a count of coincidences, far from chi-square (a small ensemble of a large model: case D)
    classes = dispersion_classes(ch, mu, floor=max(0.05, 0.05 * (1 << 14) / R))
    K = len(classes)
    if K == 0:
        return 0
    z = z_of(alpha / K)
    lo, hi = wilson_hilferty(R - 1, -z), wilson_hilferty(R - 1, z)
    worst = (0.0, None)
    for label, idx in classes:
        x = counts[:, idx].sum(axis=1, dtype=np.float64) if len(idx) > 1 else counts[:, idx[0]].astype(np.float64)
        mean = x.mean()
        assert mean > 0, "no event at all on %s (mean %.4g per step)" % (label, mu[idx].sum())
        D = float(((x - mean) ** 2).sum() / mean)
        dev = (D - (R - 1)) / math.sqrt(2.0 * (R - 1))
        if abs(dev) > abs(worst[0]):
            worst = (dev, label)
        assert lo <= D <= hi, "dispersion of %s (mean %.4g): D = %.1f outside [%.1f, %.1f] (variance / mean = %.4f, K = %d)" % (
            label, mu[idx].sum(), D, lo, hi, D / (R - 1), K)
    if report is not None:
        report("dispersion: K = %d, z = %.2f, largest deviation %.2f sigma at %s" % (K, z, worst[0], worst[1]))
    return K




def check_pmf(label, x, mean, alpha, K):
    """Chi-square of the counts ``x`` of one channel against the exact Poisson(mean) pmf; classes merged from both ends until every
    expected count is >= 8 (the rule of tests/test_samplers.py); bound: Wilson-Hilferty at z(alpha / K), one-sided."""
    n = len(x)
    lo, hi = max(int(mean - 8 * math.sqrt(mean) - 10), 0), int(mean + 8 * math.sqrt(mean) + 20)
    pmf = np.exp(_log_pmf_range(mean, 0, hi))
    exp = pmf[lo:hi + 1] * n
    exp[0] += pmf[:lo].sum() * n
    exp[-1] += max(1.0 - pmf.sum(), 0.0) * n
    obs = np.bincount(np.clip(x, lo, hi) - lo, minlength=hi - lo + 1).astype(float)
    while len(exp) > 2 and exp[0] < 8:
        exp[1] += exp[0]; obs[1] += obs[0]; exp, obs = exp[1:], obs[1:]
    while len(exp) > 2 and exp[-1] < 8:
        exp[-2] += exp[-1]; obs[-2] += obs[-1]; exp, obs = exp[:-1], obs[:-1]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    dof = len(exp) - 1
    bound = wilson_hilferty(dof, NormalDist().inv_cdf(1.0 - alpha / K))
    assert chi2 <= bound, "pmf of %s (mean %.4g): chi-square %.1f over %d classes (bound %.1f, K = %d)" % (label, mean, chi2, dof + 1, bound, K)
    return chi2, dof




def regime_of(lam):
    """The mean regime of a compartment (expected events per step): 0: < 1, 1: [1, 16), 2: [16, 64), 3: >= 64."""
    return 0 if lam < 1.0 else 1 if lam < 16.0 else 2 if lam < 64.0 else 3


def compartment_means(ch, mu):
    """Expected events per step of every infectious compartment [P * H] (all the channels it emits)."""
    lam = np.zeros(ch.P * ch.H)
    sel = ch.comp >= 0
    np.add.at(lam, ch.comp[sel], mu[sel])
    return lam


def pmf_channels(ch, mu):
    """For the full-pmf test: for every kind and every mean regime of the EMITTING compartment that the state holds, the channel of
    that kind with the largest mean (immunity transitions, which no compartment emits: the largest per population)."""
    lam = compartment_means(ch, mu)
    out = []
    for k in (BIRTH, DEATH, SAMPLING, MUTATION, MIGRATION):
        for reg in range(4):
            sel = np.nonzero((ch.kind == k) & (mu > 0) & np.array([regime_of(v) == reg for v in lam[np.maximum(ch.comp, 0)]]))[0]
            if len(sel):
                out.append((int(sel[np.argmax(mu[sel])]), reg))
    for pn in range(ch.P):
        sel = np.nonzero((ch.kind == SUSCCHANGE) & (ch.pop == pn) & (mu > 0))[0]
        if len(sel):
            out.append((int(sel[np.argmax(mu[sel])]), -1))
    return out


def kind_sums(ch, counts, comp):
    """[R, n] counts of compartment ``comp`` by kind (``Channels.sub``), and the kinds' labels."""
    sel = np.nonzero(ch.comp == comp)[0]
    subs = np.unique(ch.sub[sel])
    cols = [counts[:, sel[ch.sub[sel] == s]].sum(axis=1, dtype=np.float64) for s in subs]
    return np.stack(cols, axis=1), subs


def check_correlations(ch, mu, counts, alpha=ALPHA, report=None, floor=16.0):
    """Poisson splitting makes these independent; the sample correlation r of two independent samples of R values each is, to first
    order, normal with standard deviation 1 / sqrt(R) — good for counts with mean >= 16, and such are used:
      (i)  all pairs of kinds within an infectious compartment (recoveries, samples, mutants, migrants, births per group);
      (ii) total events — and the events of each kind — of compartments that are neighbours in the stream key (same haplotype in two
           populations, adjacent haplotypes), and total events of every pair of compartments drawn by different forms (mean regimes).
    For the neighbours in the stream key (ii) smaller means are admitted as well where R carries the approximation: the first Edgeworth
    term of the tail of r at deviate z is z^3 k3 / (6 sqrt(R)) with k3 = 1 / sqrt(mean_x mean_y) (the skewness of a product of two
    standardised Poisson counts); it stays below 0.1 — a tail probability right to 10 % — where mean_x mean_y >= (z^3 / (0.6 sqrt(R)))^2,
    taken at z = 6.6 (alpha / K for up to 10^4 pairs): a product of 1.75 at R = 2^17, 14 at 2^14.  Two compartments that shared a random
    stream would be caught there even where both are drawn event by event (means below 16).
    Fails when |r| > z(alpha / K) / sqrt(R)."""
    R = counts.shape[0]
    lam = compartment_means(ch, mu)
    H = ch.H
    prod_floor = (6.6 ** 3 / (0.6 * math.sqrt(R))) ** 2
    pairs = []                                   # (label, x, y)
    tot = {}

    def total(c):
        if c not in tot:
            tot[c] = counts[:, ch.comp == c].sum(axis=1, dtype=np.float64)
        return tot[c]

    comps = np.nonzero(lam >= floor)[0]
    for c in comps:
        x, subs = kind_sums(ch, counts, c)
        keep = [j for j in range(len(subs)) if mu[(ch.comp == c) & (ch.sub == subs[j])].sum() >= floor]
        for a in range(len(keep)):
            for b_ in range(a + 1, len(keep)):
                pairs.append(("kinds %d, %d of compartment (pop %d, hap %d)" % (subs[keep[a]], subs[keep[b_]], c // H, c % H),
                              x[:, keep[a]], x[:, keep[b_]]))
    occupied = np.nonzero(lam > 0)[0]
    for i, c1 in enumerate(occupied):
        for c2 in occupied[i + 1:]:
            both = lam[c1] >= floor and lam[c2] >= floor
            same_hap, adjacent = c1 % H == c2 % H, (c1 // H == c2 // H and abs(c1 - c2) == 1)
            if ((same_hap or adjacent) and (both or lam[c1] * lam[c2] >= prod_floor)) or (both and regime_of(lam[c1]) != regime_of(lam[c2])):
                pairs.append(("totals of compartments (pop %d, hap %d), (pop %d, hap %d)" % (c1 // H, c1 % H, c2 // H, c2 % H), total(c1), total(c2)))
            if same_hap or adjacent:
                # ... and kind by kind: a compartment's number of events may come from another stream than the choice of each event's
                # kind (the step kernels' bucketed first uniform), so shared streams can leave the totals independent and still tie the kinds
                for sub in np.unique(ch.sub[ch.comp == c1]):
                    s1, s2 = (ch.comp == c1) & (ch.sub == sub), (ch.comp == c2) & (ch.sub == sub)
                    m1, m2 = mu[s1].sum(), mu[s2].sum()
                    if (m1 >= floor and m2 >= floor) or m1 * m2 >= prod_floor:
                        pairs.append(("kind %d of compartments (pop %d, hap %d), (pop %d, hap %d)" % (sub, c1 // H, c1 % H, c2 // H, c2 % H),
                                      counts[:, s1].sum(axis=1, dtype=np.float64), counts[:, s2].sum(axis=1, dtype=np.float64)))
    K = len(pairs)
    assert K > 0
    bound = z_of(alpha / K) / math.sqrt(R)
    worst = (0.0, None)
    for label, x, y in pairs:
        r = float(np.corrcoef(x, y)[0, 1])
        if abs(r) > abs(worst[0]):
            worst = (r, label)
        assert abs(r) <= bound, "correlation %.5f of %s exceeds %.5f (K = %d, R = %d)" % (r, label, bound, K, R)
    if report is not None:
        report("correlations: K = %d, bound %.5f, largest %.5f at %s" % (K, bound, worst[0], worst[1]))
    return K




# ------------------------------------------------------------------------------------------------ the cases
def _start(sim, infectious, susceptible_split, lockdown=()):
    """Write the common start state into the model: ``infectious`` [P, H]; ``susceptible_split`` [P, S]: hosts per group taken from
    group 0 (column 0 ignored: group 0 keeps the rest); ``lockdown``: populations whose lockdown is ON (contact density after lockdown).
    The log holds one placeholder record, so that a call of ONE iteration makes exactly one step (capacity rule of events.pxi:52-68:
    on an empty log a tau call of n iterations makes 2 n steps)."""
    m = sim.simulation
    m.infectious[:] = infectious
    split = np.array(susceptible_split, dtype=np.int64)
    split[:, 0] = 0
    m.susceptible[:] = split
    m.susceptible[:, 0] = m.sizes - m.infectious.sum(axis=1) - split.sum(axis=1)
    assert (m.susceptible >= 0).all()
    for pn in lockdown:
        m.lockdownON[pn] = 1
        m.contactDensity[pn] = m.contactDensityAfterLockdown[pn]
    m.totalInfectious[:] = m.infectious.sum(axis=1)
    m.totalSusceptible[:] = m.susceptible.sum(axis=1)
    m.globalInfectious = int(m.totalInfectious.sum())
    m.first_simulation = True
    m.initial_infectious[:] = m.infectious
    m.initial_susceptible[:] = m.susceptible
    m.events.CreateEvents(1)
    m.events.ptr = 1
    return sim


def case_A(seed=1):
    """2 sites, 4 populations, a non-uniform migration matrix (six of the twelve pairs are 0), sampling multipliers, population 2
    with its lockdown ON, two susceptibility groups."""
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=2, populations_number=4, number_of_susceptible_groups=2, seed=seed)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.02)
    s.set_susceptibility_type(1); s.set_susceptibility(0.3, susceptibility_type=1)
    s.set_immunity_transition(0.002, source=1, target=0); s.set_immunity_transition(0.0005, source=0, target=1)
    s.set_population_size(4 * 10 ** 6); s.set_population_size(2 * 10 ** 6, population=3)
    for (src, dst), p in {(0, 1): 0.004, (0, 2): 0.001, (1, 0): 0.002, (1, 3): 0.003, (2, 3): 0.0005, (3, 0): 0.0025}.items():
        s.set_migration_probability(p, source=src, target=dst)
    s.set_sampling_multiplier(2.5, population=1); s.set_sampling_multiplier(0.5, population=3)
    s.set_contact_density(1.3, population=1)
    s.set_npi([0.4, 0.001, 0.0001], population=2)
    inf = np.zeros((4, 16), dtype=np.int64)
    inf[0, [0, 1, 5, 10]] = [30000, 1200, 20, 6000]
    inf[1, [0, 1, 2, 15]] = [20, 30000, 5000, 300]
    inf[2, [1, 3, 4, 10, 11]] = [1500, 300, 25, 30000, 4000]     # haplotype 1 in populations 0 and 2: both below a mean of 16
    inf[3, [0, 7, 8, 15]] = [2500, 40, 400, 20000]
    split = np.zeros((4, 2), dtype=np.int64)
    split[:, 1] = [10 ** 6, 5 * 10 ** 5, 3 * 10 ** 5, 2 * 10 ** 5]
    return _start(s, inf, split, lockdown=(2,))


def case_B(seed=2):
    """3 sites, 2 populations, per-site mutation rates and unequal weights of the derived states (one of them 0), three rate classes:
    haplotype 21 with a transmission, recovery and sampling rate of its own, haplotype 5 with a transmission rate of its own."""
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=3, populations_number=2, number_of_susceptible_groups=1, seed=seed)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1)
    s.set_transmission_rate(3.4, haplotype=21); s.set_recovery_rate(0.6, haplotype=21); s.set_sampling_rate(0.25, haplotype=21)
    s.set_transmission_rate(1.9, haplotype=5)
    s.set_mutation_rate(0.004, mutation=0); s.set_mutation_rate(0.02, mutation=1); s.set_mutation_rate(0.012, mutation=2)
    s.set_mutation_probabilities([1, 2, 0.5, 1.5], mutation=0)
    s.set_mutation_probabilities([3, 1, 0, 2], mutation=1)            # derived state G of site 1: weight 0, never drawn
    s.set_mutation_probabilities([1, 1, 4, 1], mutation=2)
    s.set_mutation_rate(0.03, haplotype=21, mutation=2)
    s.set_population_size(10 ** 7); s.set_population_size(3 * 10 ** 6, population=1)
    s.set_migration_probability(0.002)
    inf = np.zeros((2, 64), dtype=np.int64)
    inf[0, [0, 5, 21, 22, 40, 63]] = [30000, 600, 3000, 20, 2500, 250]
    inf[1, [0, 1, 5, 21, 37, 38]] = [25, 3000, 800, 20000, 300, 60]   # haplotype 5 in both populations, both below a mean of 16
    return _start(s, inf, np.zeros((2, 1), dtype=np.int64))


def case_C(seed=3):
    """1 site, 2 populations, SIX susceptibility groups: susceptibilities from 0 (exactly) to 1 with per-haplotype rows, immunity
    transitions among the groups (4 <-> 5 included), haplotypes whose recovered hosts join groups 4 and 5."""
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=1, populations_number=2, number_of_susceptible_groups=6, seed=seed)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.02)
    for sn, v in enumerate([1.0, 0.8, 0.5, 0.0, 0.3, 0.6]):
        s.set_susceptibility(v, susceptibility_type=sn)
    s.set_susceptibility(0.9, haplotype=2, susceptibility_type=4); s.set_susceptibility(0.0, haplotype=2, susceptibility_type=5)
    s.set_susceptibility(0.1, haplotype=3, susceptibility_type=3)
    for hn, st in enumerate([1, 4, 5, 3]):
        s.set_susceptibility_type(st, haplotype=hn)
    for (a, b), v in {(1, 0): 0.01, (2, 1): 0.004, (3, 2): 0.002, (4, 5): 0.003, (5, 4): 0.006, (5, 0): 0.001, (0, 4): 0.0002}.items():
        s.set_immunity_transition(v, source=a, target=b)
    s.set_population_size(6 * 10 ** 6); s.set_population_size(3 * 10 ** 6, population=1)
    s.set_migration_probability(0.003, source=0, target=1); s.set_migration_probability(0.001, source=1, target=0)
    inf = np.array([[30000, 3000, 300, 20], [2500, 20000, 350, 25]], dtype=np.int64)
    split = np.array([[0, 10 ** 6, 5 * 10 ** 5, 2 * 10 ** 5, 10 ** 6, 3 * 10 ** 5],
                      [0, 2 * 10 ** 5, 0, 10 ** 5, 4 * 10 ** 5, 10 ** 6]], dtype=np.int64)
    return _start(s, inf, split)


def case_D(seed=4):
    """7 sites (16 384 haplotypes), 2 populations, one rate class, equal weights, uniform migration; 236 of the 32 768 compartments
    occupied (0.7 %): the step kernels' lists of occupied compartments, front pass and (from a call's second step on) sparse drift pass.
    Mutation and migration are rare, so that after one step only a handful of compartments hold a single host (see
    ``state_rejection_bound``)."""
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=7, populations_number=2, number_of_susceptible_groups=1, seed=seed)
    s.set_transmission_rate(6.0); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.001)
    s.set_total_migration_probability(0.001); s.set_population_size(10 ** 8)
    rng = np.random.default_rng(20240 + seed)
    inf = np.zeros((2, 16384), dtype=np.int64)
    for pn in range(2):
        haps = rng.choice(16384, size=118, replace=False)
        inf[pn, haps] = np.concatenate(([30000], [1500] * 5, [300] * 32, rng.integers(20, 41, size=80)))
    return _start(s, inf, np.zeros((2, 1), dtype=np.int64))


CASES = {"A": case_A, "B": case_B, "C": case_C}

# Replicates of the GPU test (tests/test_hip_tau_step_law.py).  From the resolution wanted: a relative error of 3 % in a channel whose mean
# is 0.5 events per step falls outside the totals bound when z(alpha / K) sqrt(1 / (R 0.5)) <= 0.03; with K of the order of 10^2..10^3
# hypotheses z is 5.9 .. 6.3, so R >= 2 (6.3 / 0.03)^2 = 88 200: the next power of two.  A (kind, population) total is then resolved to
# 1 % from a mean of (z / 0.01)^2 / R = 3.0 events per step on (the tests print the resolution of every class and assert these two).
# Case D (tau_law.case_D, two steps): 256.  Its second step starts from states that hold a few compartments of ONE host (the first step's
# mutants and migrants), each of which is rejected with probability (out tau)^2 / 2 = 4e-6: the sum of the replicates' bounds must stay below
# 0.01, which allows 256 replicates and no more.  Resolution at 256: 1.5 % on the births of a population, 4 % on its recoveries, 12 % on its
# samples, 30-40 % on its mutants and migrants (z sqrt(1 / (R mean)), printed by the test); single channels of the first step from a mean of
# 140 events per step on (the largest compartments) to 3 %.
GPU_REPLICATES = {"A": 1 << 17, "B": 1 << 17, "C": 1 << 17, "D": 1 << 8}


def check_pooled_totals(observed, expected, alpha=ALPHA, report=None):
    """[6, P] observed totals by (kind, population) against Poisson(expected) (sums of independent Poissons, given the states they were
    drawn from); a class of rate 0 never fires."""
    classes = [(k, pn) for k in range(6) for pn in range(observed.shape[1]) if expected[k, pn] > 0]
    for k in range(6):
        for pn in range(observed.shape[1]):
            assert expected[k, pn] > 0 or observed[k, pn] == 0, "%d %s events in population %d, whose rate is 0" % (observed[k, pn], KIND_NAMES[k], pn)
    K = len(classes)
    z = z_of(alpha / K)
    for k, pn in classes:
        p = poisson_two_sided(int(observed[k, pn]), float(expected[k, pn]))
        if report is not None:
            report("%s of population %d: %d observed, %.6g expected, tail %.3g, resolution %.2f %%" % (
                KIND_NAMES[k], pn, observed[k, pn], expected[k, pn], p, 100 * z / math.sqrt(expected[k, pn])))
        assert p >= alpha / K, "%s total of population %d: %d observed, %.6g expected (relative %.3g), two-sided tail %.3g < %.3g" % (
            KIND_NAMES[k], pn, observed[k, pn], expected[k, pn], observed[k, pn] / expected[k, pn] - 1.0, p, alpha / K)
    return K


class Snapshot:
    """The start state of a case, to run many seeds on one model object."""
    NAMES = ("infectious", "susceptible", "totalInfectious", "totalSusceptible", "lockdownON", "contactDensity")

    def __init__(self, model):
        self.arrays = {k: getattr(model, k).copy() for k in self.NAMES}
        self.scalars = {k: getattr(model, k) for k in model.COUNTERS + ("globalInfectious", "currentTime", "tau_l", "good_attempt")}

    def restore(self, model):
        from oracle import oracle
        for k, a in self.arrays.items():
            getattr(model, k)[:] = a
        for k, v in self.scalars.items():
            setattr(model, k, v)
        model.events.ptr = 1
        oracle.get_state(model).mev_ptr = 0


def check_bookkeeping(ch, counts, start, suscType, infectious, susceptible, counters):
    """Every replicate's final state is the start state with its own rows applied, and its counters (bCounter, dCounter, sCounter,
    mCounter, iCounter, migPlus: increments over the step) are the row sums by kind.  Integers, bit for bit."""
    inf, sus, cnt = apply_rows(ch, counts, start.arrays["infectious"], start.arrays["susceptible"], suscType)
    bad = np.nonzero((inf != infectious).any(axis=(1, 2)) | (sus != susceptible).any(axis=(1, 2)))[0]
    assert len(bad) == 0, "replicate %d: the final compartments are not the start state with its rows applied" % bad[0]
    bad = np.nonzero((cnt != counters).any(axis=1))[0]
    assert len(bad) == 0, "replicate %d: counters %s, row sums %s" % (bad[0], counters[bad[0]], cnt[bad[0]])


def check_step_law(ch, mu, counts, alpha=ALPHA, report=None):
    """All the distributional statistics of one case: zero-rate channels, totals, dispersion, full pmf, correlations."""
    R = counts.shape[0]
    totals = counts.sum(axis=0, dtype=np.int64)
    check_zero_channels(ch, mu, totals)
    check_totals(ch, mu, totals, R, alpha, report)
    check_dispersion(ch, mu, counts, alpha, report)
    sel = pmf_channels(ch, mu)
    for c, reg in sel:
        chi2, dof = check_pmf(ch.label(c), counts[:, c], float(mu[c]), alpha, len(sel))
        if report is not None:
            report("pmf: %s, mean %.4g (compartment regime %d): chi-square %.1f over %d dof" % (ch.label(c), mu[c], reg, chi2, dof))
    check_correlations(ch, mu, counts, alpha, report)


def check_regimes(ch, mu, wanted=(0, 1, 2, 3)):
    """The state holds at least one infectious compartment in each of the wanted mean regimes (events per step < 1, [1, 16), [16, 64),
    >= 64), and every kind of event has a channel in each: a later change of a case cannot silently empty a cell of the matrix."""
    lam = compartment_means(ch, mu)
    have = {regime_of(v) for v in lam[lam > 0]}
    assert set(wanted) <= have, "mean regimes present: %s" % sorted(have)
    return {r: [int(c) for c in np.nonzero(lam > 0)[0] if regime_of(lam[c]) == r] for r in have}


def oracle_step(sim_or_model, seed=None):
    """One tau step of the oracle on the model (in place), multievents recorded: returns (dense per-channel counts in the reference's
    order, leap, rejected tries, the oracle's row descriptors)."""
    from oracle import oracle
    m = getattr(sim_or_model, "simulation", sim_or_model)
    if seed is not None:
        m.user_seed = int(seed)
    t0 = m.currentTime
    rc = oracle.run_tau(m, 1, 10 ** 12, -1, 200, record_multievents=True)
    assert rc == 0, "oracle error %d" % rc
    st = oracle.get_state(m)
    assert m.events.ptr == 2 and st.mev_ptr == oracle.prop_num(m), "one step, one dense block of rows"
    return st.mev["num"][:st.mev_ptr].copy(), m.currentTime - t0, oracle.tau_tries(0), st.mev


# ------------------------------------------------------------------------------------------------ sums of the law over a state (case D)
def kind_population_rates(model, infectious, susceptible):
    """[R, 6, P]: the summed rate of every (kind, population) class for the states ``infectious`` [R, P, H], ``susceptible`` [R, P, S] — the
    channel formulas of ``channel_table`` summed in closed form (a test compares the two on the start state); MIGRATION by SOURCE population,
    as its rows are logged."""
    m = model
    eff, actual = derived_rates(m)
    I, X = np.asarray(infectious, dtype=np.float64), np.asarray(susceptible, dtype=np.float64)
    mig, cd = m.migrationRates.astype(np.float64), m.contactDensity.astype(np.float64)
    contact = ((mig * mig) * (cd / actual)[None, :]).sum(axis=1)
    out = np.zeros((I.shape[0], 6, m.popNum))
    bs = m.bRate[:, None] * m.susceptibility                                              # [H, S]
    force = np.einsum("rph,hs->rps", I, bs)                                                # [R, P, S]: sum_h b_h susc[h, s] I[p, h]
    out[:, BIRTH] = (force * X).sum(axis=2) * contact[None, :]
    out[:, DEATH] = I @ m.dRate
    out[:, SAMPLING] = (I @ m.sRate) * m.samplingMultiplier[None, :]
    out[:, MUTATION] = I @ m.mRate.sum(axis=1)
    out[:, SUSCCHANGE] = X @ (m.suscepTransition * (1 - np.eye(m.susNum))).sum(axis=1)
    off = eff.T * (1 - np.eye(m.popNum))                                                   # [spn, tpn] = eff[tpn, spn]
    out[:, MIGRATION] = np.einsum("rps,pt,rts->rp", force, off, X) * np.diag(mig)[None, :]
    return out


def state_rejection_bound(model, infectious, susceptible, tau):
    """Upper bound on the probability that the first try from ONE state is rejected, without the channel table (large models): a compartment
    of X hosts falls below zero only if its out-channels (recovery, sampling, mutation; for susceptible hosts infection and immunity
    transitions) draw more than X; nothing can rise above ``sizes`` unless ALL events of the step together exceed the smallest room left."""
    m = model
    I, X = np.asarray(infectious, dtype=np.float64), np.asarray(susceptible, dtype=np.float64)
    out_i = (m.dRate[None, :] + m.sRate[None, :] * m.samplingMultiplier[:, None] + m.mRate.sum(axis=1)[None, :]) * I
    rates = kind_population_rates(m, I[None], X[None])[0]
    q = 0.0
    for pn, hn in zip(*np.nonzero(I)):
        q += poisson_sf(int(I[pn, hn]), out_i[pn, hn] * tau)
    eff, _ = derived_rates(m)
    bs = m.bRate[:, None] * m.susceptibility
    force = I @ bs                                                                         # [P, S]
    mig, cd = m.migrationRates, m.contactDensity
    contact = ((mig * mig) * (cd / m.actualSizes)[None, :]).sum(axis=1)
    arrive = (eff * (1 - np.eye(m.popNum))) @ (force * np.diag(mig)[:, None])              # [tpn, sn]: migrants that infect group sn of tpn
    out_s = X * (force * contact[:, None] + arrive + (m.suscepTransition * (1 - np.eye(m.susNum))).sum(axis=1)[None, :])
    for pn, sn in zip(*np.nonzero(out_s)):
        q += poisson_sf(int(X[pn, sn]), out_s[pn, sn] * tau)
    room = float(min((m.sizes[:, None] - I).min(), (m.sizes[:, None] - X)[X > 0].min()))
    q += (I.size + X.size) * poisson_sf(int(room), rates.sum() * tau)
    return q


def set_state(model, start, infectious, susceptible):
    """The snapshot ``start`` with the compartments replaced (totals kept consistent)."""
    start.restore(model)
    model.infectious[:] = infectious
    model.susceptible[:] = susceptible
    model.totalInfectious[:] = model.infectious.sum(axis=1)
    model.totalSusceptible[:] = model.susceptible.sum(axis=1)
    model.globalInfectious = int(model.totalInfectious.sum())


def oracle_tau(model, start, infectious, susceptible):
    """The leap ChooseTau (pyx:2432-2450) gives a state: the oracle's first step from it, its leap times 2^(rejected tries)."""
    from oracle import oracle
    set_state(model, start, infectious, susceptible)
    assert oracle.run_tau(model, 1, 10 ** 12, -1, 200) == 0
    return model.currentTime * 2.0 ** oracle.tau_tries(0)


def apply_sparse_rows(rep, kind, hap, pop, nh, npop, num, start_i, start_s, suscType, R):
    """``apply_rows`` for models too large for dense effect matrices: the rows scattered into [R, P, H] / [R, P, S] directly."""
    inf = np.repeat(np.asarray(start_i, dtype=np.int64)[None], R, axis=0)
    sus = np.repeat(np.asarray(start_s, dtype=np.int64)[None], R, axis=0)
    cnt = np.zeros((R, 6), dtype=np.int64)
    np.add.at(cnt, (rep, kind), num)
    st = np.asarray(suscType)
    k = kind == MIGRATION
    np.add.at(inf, (rep[k], npop[k], hap[k]), num[k]); np.add.at(sus, (rep[k], npop[k], nh[k]), -num[k])
    k = kind == SUSCCHANGE
    np.add.at(sus, (rep[k], pop[k], nh[k]), num[k]); np.add.at(sus, (rep[k], pop[k], hap[k]), -num[k])
    k = (kind == DEATH) | (kind == SAMPLING)
    np.add.at(inf, (rep[k], pop[k], hap[k]), -num[k]); np.add.at(sus, (rep[k], pop[k], st[hap[k]]), num[k])
    k = kind == MUTATION
    np.add.at(inf, (rep[k], pop[k], nh[k]), num[k]); np.add.at(inf, (rep[k], pop[k], hap[k]), -num[k])
    k = kind == BIRTH
    np.add.at(inf, (rep[k], pop[k], hap[k]), num[k]); np.add.at(sus, (rep[k], pop[k], nh[k]), -num[k])
    return inf, sus, cnt
