// vgx_gwalk_tau.h — the backward walk of a TAU chain (GetGenealogy's MULTITYPE branch, reference src/_BirthDeath.pyx:873-994),
// written once for the host and the device, beside the direct walk of vgx_gwalk.h whose workspace (VgxGwRep), compartment table,
// result and statuses it reuses.  vgx_tau_genealogies.hip runs it one replicate per wavefront over rows its canonicalise kernel
// wrote; the same file runs the host instance behind vgx_test_tau_genealogy_walk.  Operation for operation the row rule is
// Pass::row of vgx_genealogy.cpp: the same hypergeometric calls with the same arguments, the same floor(lbs * u) indices, the same
// swap / pop order in every lineage list, the arrivals of a row appended after it in reverse order, infectiousDelta after the row.
//
// Three parts:
//   * the canonical key of a multievent row (two 64-bit words) and the merge rule: _capi.canonical_multievents is the
//     specification — within a step rows are ordered by (migration first, population, target population or transition / other,
//     group or haplotype, channel code) and rows with equal keys are one row with the sum of their `num`;
//   * numpy's random_hypergeometric on PCG64 (distributions.c: hypergeometric_sample below 10 draws, HRUA from 10 on) with the
//     bit generator's buffered 32-bit half as part of the state.  HRUA's logarithms (Stirling's ln k! from k = 126, 2 ln U <= T)
//     are vgx_log of vgx_rng.h: +, -, *, / on binary64 without contraction, so the device and the host instance of this header
//     agree bit for bit.  vgx_get_genealogy calls libm's log instead: against it a draw can differ only where one of HRUA's
//     comparisons is decided within the last ulp of a logarithm (include/vgx.h);
//   * the walk: a chain is the prefix (events of the model before the tau call: direct events take VgxGwWalk::single, MULTITYPE
//     events the row rule on the model's rows, which are canonical already), then the replicate's own steps as canonical rows.
// A row has one arrival compartment and at most two count deltas: the arrivals of a row live in one scratch segment of
// 2 sCounter - 1 entries, not in a map.  A compartment's lineage segment holds min(possible pushes, sCounter) entries: a list never
// holds more lineages than are alive.
#pragma once
#include "vgx_gwalk.h"
#include "vgx_logfact.h"

enum {
    VGX_GW_STEP_ROWS = 10,          // arg = the step (0-based, of the replicate's own steps) with more raw rows than VGX_GT_STEP_ROWS_MAX
    VGX_GW_UNKNOWN_ROW_TYPE = 11,   // arg = the type of a multievent row
    VGX_GW_BAD_ROW = 12             // arg = the chain's event index: an index outside the model, or more
                                    // events than the compartment's counts allow (numpy's hypergeometric raises); vgx_get_genealogy does not check these
};

// The most raw rows of one step the canonicalise kernel sorts: the sort holds a 16-byte key and a 2-byte row index per row in
// LDS, 18 x 8192 + 64 = 147 520 of the 163 840 bytes (160 KiB) a workgroup may declare; 16 384 rows would need 288 KiB.
#define VGX_GT_STEP_ROWS_MAX 8192
#define VGX_GT_ROW_DIRECT (1 << 30)   // in VgxGtRow.type: a prefix event of direct type (one row, the single-event rule)

struct VgxGtRow {   // 32 bytes
    int64_t num;
    int32_t type, hap, pop, nh, np, pad;
};

// ---- canonical key -------------------------------------------------------------------------------------------------------
// (k1, k2, k3, k4, k5) of _capi.canonical_multievents as two words that compare like the tuple: hi = k1 | k2 | k3, lo = k4 | k5.
// Every field is below 2^31 for a row the tau kernels write (an all-ones hi word is never a key: the sort's padding).
VGX_HD void vgx_gt_row_key(int64_t sites, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np, uint64_t &hi, uint64_t &lo) {
    const bool mig = type == VGX_GW_MIGRATION;
    const uint64_t k1 = mig ? 0 : 1;
    const uint64_t k2 = (uint64_t)pop & 0x7fffffffull;
    const uint64_t k3 = (uint32_t)(mig ? np : (type == VGX_GW_SUSCCHANGE ? 0 : 1));
    const uint64_t k4 = (uint32_t)(mig ? nh : hap);
    int64_t k5 = 0;
    if (mig) k5 = hap;
    else if (type == VGX_GW_SUSCCHANGE) k5 = nh;
    else if (type == VGX_GW_SAMPLING) k5 = 1;
    else if (type == VGX_GW_MUTATION) {
        int64_t d = nh > hap ? nh - hap : hap - nh, low = 0, digit4 = 1;
        while (d >= 4) { d /= 4; low += 1; digit4 *= 4; }
        const int64_t AS = (hap / digit4) % 4, DS = (nh / digit4) % 4;
        k5 = 2 + (sites - 1 - low) * 3 + (DS > AS ? DS - 1 : DS);
    } else if (type == VGX_GW_BIRTH) k5 = 2 + 3 * sites + nh;
    hi = (k1 << 63) | (k2 << 32) | k3;
    lo = (k4 << 32) | (uint32_t)k5;
}

// a row the walk can take: indices inside the model (the walk's table look-ups rely on it)
VGX_HD bool vgx_gt_row_ok(int64_t P, int64_t H, int64_t num, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np) {
    if (num < 0) return false;
    switch (type) {
    case VGX_GW_BIRTH: case VGX_GW_DEATH: case VGX_GW_SAMPLING: return pop >= 0 && pop < P && hap >= 0 && hap < H;
    case VGX_GW_MUTATION: return pop >= 0 && pop < P && hap >= 0 && hap < H && nh >= 0 && nh < H;
    case VGX_GW_MIGRATION: return pop >= 0 && pop < P && hap >= 0 && hap < H && np >= 0 && np < P;
    default: return true;   // SUSCCHANGE touches no lineage; an unknown type is reported where the walk meets it
    }
}

// ---- numpy's bit generator front end and random_hypergeometric --------------------------------------------------------------
struct VgxGtGen {
    VgxPcg64 g;
    int32_t has32;      // numpy's bitgen buffer: a 32-bit half of the last 64-bit output is waiting
    uint32_t spare;
};

VGX_HD uint32_t vgx_gt_next32(VgxGtGen &r) {
    if (r.has32) { r.has32 = 0; return r.spare; }
    const uint64_t x = vgx_pcg64_next(r.g);
    r.has32 = 1;
    r.spare = (uint32_t)(x >> 32);
    return (uint32_t)x;
}

VGX_HD uint64_t vgx_gt_interval(VgxGtGen &r, uint64_t max) {   // distributions.c random_interval: uniform on [0, max]
    if (max == 0) return 0;
    uint64_t mask = max, v;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16; mask |= mask >> 32;
    if (max <= 0xffffffffull) { while ((v = (vgx_gt_next32(r) & mask)) > max) {} }
    else { while ((v = (vgx_pcg64_next(r.g) & mask)) > max) {} }
    return v;
}

VGX_HD double vgx_gt_logfact(int64_t k) {   // ln(k!): table below 126, Stirling above — numpy logfactorial.c
    if (k < 126) return vgx_logfact_table[k];
    const double halfln2pi = 0.9189385332046728;
    return (k + 0.5) * vgx_log((double)k) - k + (halfln2pi + (1.0 / k) * (1 / 12.0 - 1 / (360.0 * k * k)));
}

VGX_HD int64_t vgx_gt_hyper_small(VgxGtGen &r, int64_t good, int64_t bad, int64_t sample) {   // hypergeometric_sample
    const int64_t total = good + bad;
    int64_t left = (sample > total / 2) ? total - sample : sample;
    int64_t rem_total = total, rem_good = good;
    while (left > 0 && rem_good > 0 && rem_total > rem_good) {
        --rem_total;
        if ((int64_t)vgx_gt_interval(r, (uint64_t)rem_total) < rem_good) --rem_good;
        --left;
    }
    if (rem_total == rem_good) rem_good -= left;
    return (sample > total / 2) ? rem_good : good - rem_good;
}

VGX_HD int64_t vgx_gt_hyper_hrua(VgxGtGen &r, int64_t good, int64_t bad, int64_t sample) {   // hypergeometric_hrua (Stadlober 1990)
    const double D1 = 1.7155277699214135, D2 = 0.8989161620588988;
    const int64_t popsize = good + bad;
    const int64_t cs = sample < popsize - sample ? sample : popsize - sample;
    const int64_t mn = good < bad ? good : bad, mx = good < bad ? bad : good;
    const double p = ((double)mn) / popsize, q = ((double)mx) / popsize;
    const double mu = cs * p, a = mu + 0.5;
    const double var = ((double)(popsize - cs) * cs * p * q / (popsize - 1));
    const double c = sqrt(var + 0.5), h = D1 * c + D2;
    const int64_t m = (int64_t)floor((double)(cs + 1) * (mn + 1) / (popsize + 2));
    const double g = vgx_gt_logfact(m) + vgx_gt_logfact(mn - m) + vgx_gt_logfact(cs - m) + vgx_gt_logfact(mx - cs + m);
    const double b0 = (double)((cs < mn ? cs : mn) + 1), b1 = floor(a + 16 * c);
    const double b = b0 < b1 ? b0 : b1;
    int64_t K;
    while (true) {
        const double U = vgx_pcg64_double(r.g), V = vgx_pcg64_double(r.g);
        const double X = a + h * (V - 0.5) / U;
        if (X < 0.0 || X >= b) continue;
        K = (int64_t)floor(X);
        const double gp = vgx_gt_logfact(K) + vgx_gt_logfact(mn - K) + vgx_gt_logfact(cs - K) + vgx_gt_logfact(mx - cs + K);
        const double T = g - gp;
        if ((U * (4.0 - U) - 3.0) <= T) break;
        if (U * (U - T) >= 1) continue;
        if (2.0 * vgx_log(U) <= T) break;
    }
    if (good > bad) K = cs - K;
    if (cs < sample) K = good - K;
    return K;
}

// random_hypergeometric; the caller keeps 0 <= good, 0 <= bad, 0 <= sample <= good + bad (numpy raises otherwise)
VGX_HD int64_t vgx_gt_hypergeometric(VgxGtGen &r, int64_t good, int64_t bad, int64_t sample) {
    if (sample >= 10 && sample <= good + bad - 10) return vgx_gt_hyper_hrua(r, good, bad, sample);
    return vgx_gt_hyper_small(r, good, bad, sample);
}

// ---- the chain ---------------------------------------------------------------------------------------------------------------
// events [0, n_pre) are the prefix, event e with rows pre[pre_off[e] .. pre_off[e + 1]) (a direct event: one row with
// VGX_GT_ROW_DIRECT in its type); events n_pre + k are the replicate's own steps with rows can[can_off[k] .. can_off[k + 1]).
struct VgxGtChain {
    const VgxGtRow *pre;
    const int32_t *pre_off;
    int64_t n_pre;
    const VgxGtRow *can;
    const int32_t *can_off;
    int64_t n_steps;
    VGX_HD void rows(int64_t e, const VgxGtRow *&r, int64_t &n) const {
        if (e < n_pre) { r = pre + pre_off[e]; n = pre_off[e + 1] - pre_off[e]; }
        else { r = can + can_off[e - n_pre]; n = can_off[e - n_pre + 1] - can_off[e - n_pre]; }
    }
};

// table slots for a chain of n_rows rows (prefix and canonical): vgx_gw_table_size
// pushes a row can make into its arrival compartment, capped at sCounter
VGX_HD int64_t vgx_gt_row_pushes(int64_t type, int64_t num, int64_t sCounter) {
    const bool direct = (type & VGX_GT_ROW_DIRECT) != 0;
    const int64_t t = type & ~(int64_t)VGX_GT_ROW_DIRECT;
    if (t != VGX_GW_BIRTH && t != VGX_GW_SAMPLING && t != VGX_GW_MUTATION && t != VGX_GW_MIGRATION) return 0;
    if (direct) return t == VGX_GW_BIRTH ? 0 : 1;
    return num < sCounter ? num : sCounter;
}

// Pre-pass: every compartment the chain touches goes into the table; every possible push reserves a slot of the arrival
// compartment's segment, up to sCounter slots.  Returns VGX_GW_OK or VGX_GW_WORKSPACE.
VGX_HD int vgx_gt_prepass(VgxGwRep &w, const VgxGtChain &c) {
    for (int64_t e = w.n_ev - 1; e >= 0; --e) {
        const VgxGtRow *r;
        int64_t n;
        c.rows(e, r, n);
        for (int64_t j = 0; j < n; j++) {
            const int64_t type = r[j].type & ~(int32_t)VGX_GT_ROW_DIRECT, hap = r[j].hap, pop = r[j].pop, nh = r[j].nh, np = r[j].np;
            int64_t s0 = 0, sa = -2;   // sa: the arrival compartment
            switch (type) {
            case VGX_GW_BIRTH: s0 = sa = vgx_gw_insert(w, pop * w.H + hap); break;
            case VGX_GW_DEATH: s0 = vgx_gw_insert(w, pop * w.H + hap); break;
            case VGX_GW_SAMPLING: s0 = sa = vgx_gw_insert(w, pop * w.H + hap); break;
            case VGX_GW_MUTATION: s0 = vgx_gw_insert(w, pop * w.H + nh); sa = vgx_gw_insert(w, pop * w.H + hap); break;
            case VGX_GW_MIGRATION: s0 = vgx_gw_insert(w, np * w.H + hap); sa = vgx_gw_insert(w, pop * w.H + hap); break;
            default: break;
            }
            if (s0 < 0 || sa == -1) return VGX_GW_WORKSPACE;
            if (sa >= 0) {
                const int64_t cap = w.lcap[sa] + vgx_gt_row_pushes(r[j].type, r[j].num, w.sCounter);
                w.lcap[sa] = (int32_t)(cap < w.sCounter ? cap : w.sCounter);
            }
        }
    }
    int64_t acc = 0;
    for (int64_t s = 0; s < w.tsize; s++) {
        if (w.key[s] < 0) continue;
        w.base[s] = (int32_t)acc;
        acc += w.lcap[s];
    }
    return acc <= w.arena_cap ? VGX_GW_OK : VGX_GW_WORKSPACE;
}

// one multievent row (pyx:873-994) of chain event e; `fresh`: scratch of 2 sCounter - 1 entries; false = the walk stops.  The
// observer (vgx_gwalk.h) is told where the row changes a lineage list, with the meanings of VgxGwWalkT::single: split at every
// coalescence of a BIRTH row and of a MIGRATION row (there with pop = the row's newPopulation, where the lineage it takes away
// lay), tip at every tip of a SAMPLING row, mutation at every lineage a MUTATION row takes, move at every lineage a MIGRATION row
// moves without coalescing.  All records of a step carry the same e.
template <class Obs>
VGX_HD bool vgx_gt_row(VgxGwWalkT<Obs> &k, VgxGtGen &gen, int32_t *fresh, const VgxGtRow &row, int64_t e) {
    VgxGwRep &w = k.w;
    const int64_t num = row.num, type = row.type, hap = row.hap, pop = row.pop, nh = row.nh, np = row.np, H = w.H;
    int64_t nf = 0, sa = -1;                       // arrivals of this row and their compartment
    int64_t ds0 = -1, dv0 = 0, ds1 = -1, dv1 = 0;  // infectiousDelta
    auto bad = [&]() { k.res.status = VGX_GW_BAD_ROW; k.res.arg = e; return false; };
    auto arrive = [&](int64_t id) {
        if (nf >= k.nodes) { k.res.status = VGX_GW_WORKSPACE; return false; }
        fresh[nf++] = (int32_t)id;
        return true;
    };
    auto hyper = [&](int64_t good, int64_t bd, int64_t sample, int64_t &out) {
        if (good < 0 || bd < 0 || sample > good + bd) return false;
        out = vgx_gt_hypergeometric(gen, good, bd, sample);
        return true;
    };
    switch (type) {
    case VGX_GW_BIRTH: {
        const int64_t s = vgx_gw_find(w, pop * H + hap);
        int64_t lbs = w.len[s];
        const int64_t lbs_e = w.cnt[s];
        int64_t kk = 0;
        if (!(num == 0 || lbs == 0) &&
            !hyper((int64_t)(lbs * (lbs - 1.0) / 2.0), (int64_t)(lbs_e * (lbs_e - 1) / 2 - lbs * (lbs - 1) / 2), num, kk)) return bad();
        sa = s;
        for (int64_t i = 0; i < kk; ++i) {
            if (lbs < 2) return bad();
            int64_t n1 = (int64_t)floor(lbs * k.uniform());
            int64_t n2 = (int64_t)floor((lbs - 1) * k.uniform());
            if (n2 >= n1) n2 += 1;
            const int64_t id1 = k.at(s, n1), id2 = k.at(s, n2), id3 = k.ptr;
            if (!arrive(id3)) return false;
            if (n1 == lbs - 1) k.at(s, n2) = k.at(s, lbs - 2);
            else if (n2 == lbs - 1) k.at(s, n1) = k.at(s, lbs - 2);
            else { k.at(s, n1) = k.at(s, lbs - 1); k.at(s, n2) = k.at(s, lbs - 2); }
            w.len[s] -= 2;
            k.parent(id1, id3); k.parent(id2, id3);
            k.node(pop, e);
            k.obs.split(e, hap, pop);
            lbs -= 2;
        }
        ds0 = s; dv0 = -num;
        break;
    }
    case VGX_GW_DEATH: ds0 = vgx_gw_find(w, pop * H + hap); dv0 = num; break;
    case VGX_GW_SAMPLING:
        sa = ds0 = vgx_gw_find(w, pop * H + hap);
        dv0 = num;
        for (int64_t i = 0; i < num; ++i) {
            if (k.ptr >= k.nodes) { k.res.status = VGX_GW_TREE_OVERFLOW; return false; }
            if (!arrive(k.ptr)) return false;
            k.node(pop, e);
            k.obs.tip(e, hap, pop);
        }
        break;
    case VGX_GW_MUTATION: {
        const int64_t s = vgx_gw_find(w, pop * H + nh);
        sa = vgx_gw_find(w, pop * H + hap);
        int64_t lbs = w.len[s], kk = 0;
        if (!(num == 0 || lbs == 0) && !hyper(lbs, w.cnt[s] - lbs, num, kk)) return bad();
        for (int64_t i = 0; i < kk; ++i) {
            int64_t n1 = (int64_t)floor(lbs * k.uniform());
            const int64_t id1 = k.at(s, n1);
            k.at(s, n1) = k.at(s, lbs - 1);
            w.len[s] -= 1;
            if (!arrive(id1)) return false;
            if (!k.mutation(id1, hap, nh, e)) return false;
            k.obs.mutation(e, hap, pop, nh);
            lbs -= 1;
        }
        ds0 = s; dv0 = -num;
        ds1 = sa; dv1 = num;
        break;
    }
    case VGX_GW_SUSCCHANGE: break;
    case VGX_GW_MIGRATION: {
        const int64_t ss = vgx_gw_find(w, pop * H + hap), st = vgx_gw_find(w, np * H + hap);
        sa = ss;
        int64_t lbs = w.len[st];
        if (!(num == 0 || lbs == 0)) {
            int64_t kk = 0, k2 = 0;
            if (!hyper(lbs, w.cnt[st] - lbs, num, kk)) return bad();
            int64_t lbss = w.len[ss];
            if (!(kk == 0 || lbss == 0) && !hyper(lbss, w.cnt[ss] - lbss, kk, k2)) return bad();
            for (int64_t i = 0; i < k2; ++i) {
                int64_t nt = (int64_t)floor(lbs * k.uniform());
                int64_t ns = (int64_t)floor(lbss * k.uniform());
                const int64_t idt = k.at(st, nt), ids = k.at(ss, ns), id3 = k.ptr;
                k.swap_pop(ss, ns);
                k.at(st, nt) = k.at(st, lbs - 1);
                w.len[st] -= 1;
                if (!arrive(id3)) return false;
                k.parent(idt, id3); k.parent(ids, id3);
                k.node(pop, e);
                if (!k.migration(idt, e, pop, np)) return false;
                k.obs.split(e, hap, np);
                lbss -= 1;
                lbs -= 1;
            }
            for (int64_t i = 0; i < kk - k2; ++i) {
                int64_t nt = (int64_t)floor(lbs * k.uniform());
                if (!arrive(k.at(st, nt))) return false;
                k.at(st, nt) = k.at(st, lbs - 1);
                w.len[st] -= 1;
                k.obs.move(e, hap, pop, np);
                lbs -= 1;
            }
        }
        ds0 = st; dv0 = -num;
        break;
    }
    default: k.res.status = VGX_GW_UNKNOWN_ROW_TYPE; k.res.arg = type; return false;
    }
    // pyx:988-994 for the compartments this row touched
    if (ds0 >= 0) w.cnt[ds0] += dv0;
    if (ds1 >= 0) w.cnt[ds1] += dv1;
    while (nf > 0)
        if (!k.push(sa, fresh[--nf])) return false;
    return true;
}

// The walk over the chain from the last event back, then the closing pass (pyx:998-1000).  The table holds the pre-pass's
// compartments with their final infectious counts.  `gen` advances by the draws made.  The draws, their order and the generator
// afterwards do not depend on the observer; prefix events of direct type reach it through VgxGwWalkT::single, the closing pass
// tells it nothing, and an observer without records leaves tree_pop, node_ev and the mutation and migration tables untouched.
template <class Obs = VgxGwNoObserver>
VGX_HD void vgx_gt_walk(VgxGwRep &w, const VgxGtChain &c, int32_t *fresh, VgxGtGen &gen, VgxGwResult &res, Obs obs = Obs{}) {
    res.status = VGX_GW_OK; res.arg = 0; res.nodes_used = 0; res.mut_n = 0; res.mig_n = 0;
    if (w.sCounter < 2) { res.status = VGX_GW_FEW_SAMPLES; return; }
    const int64_t nodes = 2 * w.sCounter - 1;
    for (int64_t i = 0; i < nodes; i++) {
        w.tree[i] = 0;
        if (Obs::records) { w.tree_pop[i] = 0; w.node_ev[i] = -1; }
    }
    VgxGwWalkT<Obs> k{w, gen.g, res, 0, nodes, obs};
    for (int64_t e = w.n_ev - 1; e >= 0; --e) {
        const VgxGtRow *r;
        int64_t n;
        c.rows(e, r, n);
        if (n == 1 && (r[0].type & VGX_GT_ROW_DIRECT)) {
            const int32_t ev[5] = {r[0].type & ~(int32_t)VGX_GT_ROW_DIRECT, r[0].hap, r[0].pop, r[0].nh, r[0].np};
            if (k.ptr >= nodes && ev[0] == VGX_GW_SAMPLING) { res.status = VGX_GW_EXTRA_SAMPLING; return; }
            if (!k.single(e, ev)) return;
        } else {
            for (int64_t j = 0; j < n; j++)
                if (!vgx_gt_row(k, gen, fresh, r[j], e)) return;
        }
        if (k.ptr > nodes) { res.status = VGX_GW_TREE_OVERFLOW; return; }
    }
    res.nodes_used = k.ptr;
    for (int64_t i = 0; i < 2 * w.sCounter - 2; i++) {
        const int64_t par = w.tree[i];
        if (par < 0 || par >= nodes) { res.status = VGX_GW_NOT_COALESCED; res.arg = i; return; }
        if (Obs::records && w.tree_pop[par] != w.tree_pop[i] && !k.migration(i, w.node_ev[i], w.tree_pop[par], w.tree_pop[i])) return;
    }
}

// ---- device plumbing (host driver <-> kernels of vgx_tau_genealogies.hip) ---------------------------------------------------
// one selected replicate of a canonicalise launch
struct VgxGtCanonDesc {
    int64_t rep, n_steps, sCounter;
    int64_t step_off;     // its steps' raw row ranges: mrange[step_off + k] = m0 of step k, [step_off + n_steps] = the last m1
    int64_t row_off;      // its canonical rows start at can[row_off] (room for as many as it has raw rows)
    int64_t off_off;      // its canonical row ranges: can_off[off_off .. off_off + n_steps]
};
// what the canonicalise kernel reports per replicate
struct VgxGtCanonStat {
    int64_t status, arg;          // VGX_GW_OK, VGX_GW_STEP_ROWS (arg = step) or VGX_GW_BAD_ROW (arg = step)
    int64_t n_rows;               // canonical rows
    int64_t pushes;               // sum of vgx_gt_row_pushes over them
};
struct VgxGtCanonLaunch {
    int64_t n;
    const VgxGtCanonDesc *desc;
    const int64_t *mev;           // t_mev: [R][mev_cap][6], read only
    int64_t mev_cap;
    const int32_t *mrange;
    int64_t P, H, sites;
    int cap;                      // rows the launch's LDS holds (a power of two, at most VGX_GT_STEP_ROWS_MAX)
    VgxGtRow *can;
    int32_t *can_off;
    VgxGtCanonStat *stat;
};
// one selected replicate of a walk launch: offsets into the pass's workspace and outputs (elements)
struct VgxGtDesc {
    int64_t rep, n_pre, n_steps, sCounter, tsize, tab_off, arena_off, arena_cap, node_off, mut_off, mut_cap, mig_off, mig_cap;
    int64_t row_off, off_off;     // as in its VgxGtCanonDesc
    int64_t status, arg;          // what the canonicalise kernel reported (a replicate that failed there is not walked)
    uint64_t rng[4];
    int64_t has32, spare;
};
struct VgxGtLaunch {
    int64_t n;
    const VgxGtDesc *desc;
    const VgxGtRow *pre;          // the flattened prefix, shared by the replicates that did not restart
    const int32_t *pre_off;
    const VgxGtRow *can;
    const int32_t *can_off;
    const int32_t *I;             // t_I: [R][P][H] final infectious counts
    int64_t P, H;
    int64_t *key, *cnt;
    int32_t *base, *len, *lcap, *arena, *fresh;   // fresh: [node_off ...] like the node outputs
    int32_t *tree, *tree_pop, *node_ev;
    int32_t *mut_node, *mut_AS, *mut_DS, *mut_site, *mut_ev;
    int32_t *mig_node, *mig_old, *mig_new, *mig_ev;
    int64_t *res;                 // [n][5] VgxGwResult
    uint64_t *rng_out;            // [n][6] generator state after the walk: PCG64 words, has32, spare
};
