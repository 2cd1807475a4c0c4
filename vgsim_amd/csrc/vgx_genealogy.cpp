// vgx_genealogy.cpp — backward (coalescent) pass over the event log: replaces BirthDeathModel.GetGenealogy
// (reference src/_BirthDeath.pyx:743-1000) and its recorders Mutations/Migrations (src/models.pxi:1-48).
//
// Host code of libvgx (the pass is one sequential walk, O(events); SURVEY.md §8f rank 1: "C++ first").  Unlike the
// reference, which allocates two std::vector per (population, haplotype) up front (P x H x 48 B: 200 MB at
// 65 536 x 64, 12 GB at 2^20 x 256) and sweeps all P x H compartments after every multievent row (pyx:988-994), the
// live lineages are kept per OCCUPIED compartment in a hash map and only compartments touched by a row are swept —
// same operations on the same vectors in the same order, so trees, times and records are identical.
// Random numbers: the wrapper's uniform() = PCG64 next_double (pyx:801 ...), numpy's random_hypergeometric on the
// same bit generator for MULTITYPE thinning (pyx:905, 933, 950, 956).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vgx.h"
#include "vgx_gwalk.h"
#include "vgx_gwalk_tau.h"
#include "vgx_lineages.h"
#include "vgx_tree_events.h"
#include "vgx_tree_shape.h"
#include "vgx_mutation_spectrum.h"
#include "vgx_introductions.h"
#include "vgx_logfact.h"
#include "vgx_rng.h"

namespace {

enum { BIRTH = 0, DEATH = 1, SAMPLING = 2, MUTATION = 3, SUSCCHANGE = 4, MIGRATION = 5, MULTITYPE = 6 };  // ev:2-8

// numpy bit-generator front end on PCG64: next_double, next_uint64, buffered next_uint32 (pcg64.h)
struct Gen {
    VgxPcg64 g;
    bool has32;
    uint32_t spare;
    uint64_t next64() { return vgx_pcg64_next(g); }
    double uniform() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
    uint32_t next32() {
        if (has32) { has32 = false; return spare; }
        uint64_t x = next64();
        has32 = true;
        spare = (uint32_t)(x >> 32);
        return (uint32_t)x;
    }
    uint64_t interval(uint64_t max) {  // distributions.c random_interval: uniform on [0, max]
        if (max == 0) return 0;
        uint64_t mask = max, v;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16; mask |= mask >> 32;
        if (max <= 0xffffffffull) { while ((v = (next32() & mask)) > max) {} }
        else { while ((v = (next64() & mask)) > max) {} }
        return v;
    }
};

// ln(k!): table below 126, Stirling above — numpy logfactorial.c
double logfact(int64_t k) {
    if (k < 126) return vgx_logfact_table[k];
    const double halfln2pi = 0.9189385332046728;
    return (k + 0.5) * std::log((double)k) - k + (halfln2pi + (1.0 / k) * (1 / 12.0 - 1 / (360.0 * k * k)));
}

int64_t hyper_small(Gen &r, int64_t good, int64_t bad, int64_t sample) {  // hypergeometric_sample
    const int64_t total = good + bad;
    int64_t left = (sample > total / 2) ? total - sample : sample;
    int64_t rem_total = total, rem_good = good;
    while (left > 0 && rem_good > 0 && rem_total > rem_good) {
        --rem_total;
        if ((int64_t)r.interval((uint64_t)rem_total) < rem_good) --rem_good;
        --left;
    }
    if (rem_total == rem_good) rem_good -= left;
    return (sample > total / 2) ? rem_good : good - rem_good;
}

int64_t hyper_hrua(Gen &r, int64_t good, int64_t bad, int64_t sample) {  // hypergeometric_hrua (Stadlober 1990)
    const double D1 = 1.7155277699214135, D2 = 0.8989161620588988;
    const int64_t popsize = good + bad;
    const int64_t cs = std::min(sample, popsize - sample);
    const int64_t mn = std::min(good, bad), mx = std::max(good, bad);
    const double p = ((double)mn) / popsize, q = ((double)mx) / popsize;
    const double mu = cs * p, a = mu + 0.5;
    const double var = ((double)(popsize - cs) * cs * p * q / (popsize - 1));
    const double c = std::sqrt(var + 0.5), h = D1 * c + D2;
    const int64_t m = (int64_t)std::floor((double)(cs + 1) * (mn + 1) / (popsize + 2));
    const double g = logfact(m) + logfact(mn - m) + logfact(cs - m) + logfact(mx - cs + m);
    const double b = std::min((double)(std::min(cs, mn) + 1), std::floor(a + 16 * c));
    int64_t K;
    while (true) {
        double U = r.uniform(), V = r.uniform();
        double X = a + h * (V - 0.5) / U;
        if (X < 0.0 || X >= b) continue;
        K = (int64_t)std::floor(X);
        double gp = logfact(K) + logfact(mn - K) + logfact(cs - K) + logfact(mx - cs + K);
        double T = g - gp;
        if ((U * (4.0 - U) - 3.0) <= T) break;
        if (U * (U - T) >= 1) continue;
        if (2.0 * std::log(U) <= T) break;
    }
    if (good > bad) K = cs - K;
    if (cs < sample) K = good - K;
    return K;
}

int64_t hypergeometric(Gen &r, int64_t good, int64_t bad, int64_t sample) {  // random_hypergeometric
    if (sample >= 10 && sample <= good + bad - 10) return hyper_hrua(r, good, bad, sample);
    return hyper_small(r, good, bad, sample);
}

struct Pass {
    vgx_genealogy_io &io;
    const int64_t H;
    Gen rng;
    int64_t ptr = 0;
    std::unordered_map<int64_t, std::vector<int64_t>> live, fresh;  // lineages per compartment; arrivals of a row
    std::unordered_map<int64_t, int64_t> delta;                      // infectiousDelta of the current row
    std::string err;

    explicit Pass(vgx_genealogy_io &x) : io(x), H(x.hapNum) {}
    int64_t key(int64_t p, int64_t h) const { return p * H + h; }
    int64_t &inf(int64_t p, int64_t h) { return io.infectious[p * H + h]; }
    void node(int64_t pop, double t) { io.tree[ptr] = -1; io.tree_pop[ptr] = pop; io.times[ptr] = t; ptr += 1; }
    bool mutation(int64_t nodeId, int64_t hap, int64_t nh, double t) {  // models.pxi:13-29
        if (io.mut_n >= io.mut_cap) { err = "mutation record capacity exceeded"; return false; }
        int64_t d = nh > hap ? nh - hap : hap - nh, site = 0, digit4 = 1;
        while (d >= 4) { d /= 4; site += 1; digit4 *= 4; }
        int64_t k = io.mut_n++;
        io.mut_node[k] = nodeId; io.mut_DS[k] = (nh / digit4) % 4; io.mut_AS[k] = (hap / digit4) % 4;
        io.mut_site[k] = site; io.mut_time[k] = t;
        return true;
    }
    bool migration(int64_t nodeId, double t, int64_t oldPop, int64_t newPop) {  // models.pxi:44-48
        if (io.mig_n >= io.mig_cap) { err = "migration record capacity exceeded"; return false; }
        int64_t k = io.mig_n++;
        io.mig_node[k] = nodeId; io.mig_time[k] = t; io.mig_old[k] = oldPop; io.mig_new[k] = newPop;
        return true;
    }
    static void swap_pop(std::vector<int64_t> &v, int64_t i) { v[(size_t)i] = v.back(); v.pop_back(); }

    bool single(int64_t e) {  // one event of the direct path (pyx:797-872)
        const double t = io.ev_times[e];
        const int64_t type = io.ev_types[e], hap = io.ev_haplotypes[e], pop = io.ev_populations[e];
        const int64_t nh = io.ev_newHaplotypes[e], np = io.ev_newPopulations[e];
        switch (type) {
        case BIRTH: {
            auto it = live.find(key(pop, hap));
            const int64_t lbs = it == live.end() ? 0 : (int64_t)it->second.size(), lbs_e = inf(pop, hap);
            const double p = (double)lbs * ((double)lbs - 1.0) / (double)lbs_e / ((double)lbs_e - 1.0);
            if (rng.uniform() < p) {
                auto &b = it->second;
                int64_t n1 = (int64_t)std::floor(lbs * rng.uniform());
                int64_t n2 = (int64_t)std::floor((lbs - 1) * rng.uniform());
                if (n2 >= n1) n2 += 1;
                const int64_t id1 = b[(size_t)n1], id2 = b[(size_t)n2], id3 = ptr;
                b[(size_t)n1] = id3;
                swap_pop(b, n2);
                io.tree[id1] = id3; io.tree[id2] = id3;
                node(pop, t);
            }
            inf(pop, hap) -= 1;
            return true;
        }
        case DEATH: inf(pop, hap) += 1; return true;
        case SAMPLING:
            inf(pop, hap) += 1;
            live[key(pop, hap)].push_back(ptr);
            node(pop, t);
            return true;
        case MUTATION: {
            auto it = live.find(key(pop, nh));
            const int64_t lbs = it == live.end() ? 0 : (int64_t)it->second.size();
            const double p = (double)lbs / (double)inf(pop, nh);
            if (rng.uniform() < p) {
                int64_t n1 = (int64_t)std::floor(lbs * rng.uniform());
                const int64_t id1 = it->second[(size_t)n1];
                swap_pop(it->second, n1);
                live[key(pop, hap)].push_back(id1);
                if (!mutation(id1, hap, nh, t)) return false;
            }
            inf(pop, nh) -= 1;
            inf(pop, hap) += 1;
            return true;
        }
        case SUSCCHANGE: return true;
        case MIGRATION: {
            auto it = live.find(key(np, hap));
            const int64_t lbs = it == live.end() ? 0 : (int64_t)it->second.size();
            const double p = (double)lbs / (double)inf(np, hap);
            if (rng.uniform() < p) {
                int64_t nt = (int64_t)std::floor(lbs * rng.uniform());
                auto &bs = live[key(pop, hap)];
                auto &bt = live[key(np, hap)];  // (a rehash by the line above would invalidate `it`)
                const int64_t lbss = (int64_t)bs.size();
                const double p1 = (double)lbss / (double)inf(pop, hap);
                if (rng.uniform() < p1) {
                    int64_t ns = (int64_t)std::floor(lbss * rng.uniform());
                    const int64_t idt = bt[(size_t)nt], ids = bs[(size_t)ns], id3 = ptr;
                    bs[(size_t)ns] = id3;
                    swap_pop(bt, nt);
                    io.tree[idt] = id3; io.tree[ids] = id3;
                    node(pop, t);
                    if (!migration(idt, t, pop, np)) return false;
                } else {
                    bs.push_back(bt[(size_t)nt]);
                    swap_pop(bt, nt);
                }
            }
            inf(np, hap) -= 1;
            return true;
        }
        case MULTITYPE:
            for (int64_t r = hap; r < pop; ++r)
                if (!row(r)) return false;
            return true;
        default: err = "unknown event type " + std::to_string(type); return false;
        }
    }

    bool row(int64_t r) {  // one multievent row (pyx:873-994)
        if (!io.mev_num) { err = "MULTITYPE event without a multievent log"; return false; }
        if (r < 0 || r >= io.mev_rows) { err = "multievent row out of range"; return false; }
        const int64_t num = io.mev_num[r], type = io.mev_types[r], hap = io.mev_haplotypes[r], pop = io.mev_populations[r];
        const int64_t nh = io.mev_newHaplotypes[r], np = io.mev_newPopulations[r];
        const double t = io.mev_times[r];
        switch (type) {
        case BIRTH: {
            auto &b = live[key(pop, hap)];
            int64_t lbs = (int64_t)b.size();
            const int64_t lbs_e = inf(pop, hap);
            int64_t k = 0;
            if (!(num == 0 || lbs == 0))
                k = hypergeometric(rng, (int64_t)(lbs * (lbs - 1.0) / 2.0), (int64_t)(lbs_e * (lbs_e - 1) / 2 - lbs * (lbs - 1) / 2), num);
            for (int64_t i = 0; i < k; ++i) {
                int64_t n1 = (int64_t)std::floor(lbs * rng.uniform());
                int64_t n2 = (int64_t)std::floor((lbs - 1) * rng.uniform());
                if (n2 >= n1) n2 += 1;
                const int64_t id1 = b[(size_t)n1], id2 = b[(size_t)n2], id3 = ptr;
                fresh[key(pop, hap)].push_back(id3);
                if (n1 == lbs - 1) { b.pop_back(); b[(size_t)n2] = b[(size_t)(lbs - 2)]; b.pop_back(); }
                else if (n2 == lbs - 1) { b.pop_back(); b[(size_t)n1] = b[(size_t)(lbs - 2)]; b.pop_back(); }
                else { b[(size_t)n1] = b[(size_t)(lbs - 1)]; b.pop_back(); b[(size_t)n2] = b[(size_t)(lbs - 2)]; b.pop_back(); }
                io.tree[id1] = id3; io.tree[id2] = id3;
                node(pop, t);
                lbs -= 2;
            }
            delta[key(pop, hap)] -= num;
            break;
        }
        case DEATH: delta[key(pop, hap)] += num; break;
        case SAMPLING:
            delta[key(pop, hap)] += num;
            for (int64_t i = 0; i < num; ++i) { fresh[key(pop, hap)].push_back(ptr); node(pop, t); }
            break;
        case MUTATION: {
            auto &b = live[key(pop, nh)];
            int64_t lbs = (int64_t)b.size(), k = 0;
            if (!(num == 0 || lbs == 0)) k = hypergeometric(rng, lbs, inf(pop, nh) - lbs, num);
            for (int64_t i = 0; i < k; ++i) {
                int64_t n1 = (int64_t)std::floor(lbs * rng.uniform());
                const int64_t id1 = b[(size_t)n1];
                b[(size_t)n1] = b[(size_t)(lbs - 1)];
                b.pop_back();
                fresh[key(pop, hap)].push_back(id1);
                if (!mutation(id1, hap, nh, t)) return false;
                lbs -= 1;
            }
            delta[key(pop, nh)] -= num;
            delta[key(pop, hap)] += num;
            break;
        }
        case SUSCCHANGE: break;
        case MIGRATION: {
            auto &bs = live[key(pop, hap)];
            auto &bt = live[key(np, hap)];
            int64_t lbs = (int64_t)bt.size();
            if (!(num == 0 || lbs == 0)) {
                const int64_t k = hypergeometric(rng, lbs, inf(np, hap) - lbs, num);
                int64_t lbss = (int64_t)bs.size(), k2 = 0;
                if (!(k == 0 || lbss == 0)) k2 = hypergeometric(rng, lbss, inf(pop, hap) - lbss, k);
                for (int64_t i = 0; i < k2; ++i) {
                    int64_t nt = (int64_t)std::floor(lbs * rng.uniform());
                    int64_t ns = (int64_t)std::floor(lbss * rng.uniform());
                    const int64_t idt = bt[(size_t)nt], ids = bs[(size_t)ns], id3 = ptr;
                    swap_pop(bs, ns);
                    bt[(size_t)nt] = bt[(size_t)(lbs - 1)];
                    bt.pop_back();
                    fresh[key(pop, hap)].push_back(id3);
                    io.tree[idt] = id3; io.tree[ids] = id3;
                    node(pop, t);
                    if (!migration(idt, t, pop, np)) return false;
                    lbss -= 1;
                    lbs -= 1;
                }
                for (int64_t i = 0; i < k - k2; ++i) {
                    int64_t nt = (int64_t)std::floor(lbs * rng.uniform());
                    fresh[key(pop, hap)].push_back(bt[(size_t)nt]);
                    bt[(size_t)nt] = bt[(size_t)(lbs - 1)];
                    bt.pop_back();
                    lbs -= 1;
                }
            }
            delta[key(np, hap)] -= num;
            break;
        }
        default: err = "unknown multievent type " + std::to_string(type); return false;
        }
        // pyx:988-994, restricted to the compartments this row touched
        for (auto &d : delta) io.infectious[d.first] += d.second;
        delta.clear();
        for (auto &f : fresh) {
            auto &dst = live[f.first];
            while (!f.second.empty()) { dst.push_back(f.second.back()); f.second.pop_back(); }
        }
        fresh.clear();
        return true;
    }
};

}  // namespace

extern "C" int vgx_get_genealogy(vgx_genealogy_io *io, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->infectious || !io->tree || !io->tree_pop || !io->times) return fail("vgx_get_genealogy: null argument");
    if (io->sCounter < 2) return fail("Less than two cases were sampled...");  // pyx:762-765
    const int64_t nodes = 2 * io->sCounter - 1;
    std::memset(io->tree, 0, (size_t)nodes * 8);
    std::memset(io->tree_pop, 0, (size_t)nodes * 8);
    std::memset(io->times, 0, (size_t)nodes * 8);
    io->mut_n = 0;
    io->mig_n = 0;
    Pass ps(*io);
    ps.rng.g.sh = io->rng_state[0]; ps.rng.g.sl = io->rng_state[1]; ps.rng.g.ih = io->rng_state[2]; ps.rng.g.il = io->rng_state[3];
    ps.rng.has32 = io->rng_has_uint32 != 0;
    ps.rng.spare = (uint32_t)io->rng_uinteger;
    for (int64_t e = io->ev_ptr - 1; e >= 0; --e) {
        if (ps.ptr >= nodes && (io->ev_types[e] == SAMPLING)) return fail("vgx_get_genealogy: more sampling events than sCounter");
        if (!ps.single(e)) return fail("vgx_get_genealogy: " + ps.err);
        if (ps.ptr > nodes) return fail("vgx_get_genealogy: tree overflow (event log and sCounter disagree)");
    }
    io->nodes_used = ps.ptr;
    for (int64_t i = 0; i < 2 * io->sCounter - 2; ++i) {  // pyx:998-1000
        const int64_t par = io->tree[i];
        if (par < 0 || par >= nodes) return fail("vgx_get_genealogy: lineage " + std::to_string(i) + " never coalesced (several roots)");
        if (io->tree_pop[par] != io->tree_pop[i] && !ps.migration(i, io->times[i], io->tree_pop[par], io->tree_pop[i]))
            return fail("vgx_get_genealogy: " + ps.err);
    }
    io->rng_state[0] = ps.rng.g.sh; io->rng_state[1] = ps.rng.g.sl; io->rng_state[2] = ps.rng.g.ih; io->rng_state[3] = ps.rng.g.il;
    io->rng_has_uint32 = ps.rng.has32 ? 1 : 0;
    io->rng_uinteger = ps.rng.spare;
    return VGX_OK;
}

// PCG64 (state, inc) of numpy's PCG64(SeedSequence(seed, spawn_key=(attempt,))) advanced by `draws` outputs: the
// position of the reference's self.seed after a simulate call that drew `draws` uniforms in its last attempt.
extern "C" void vgx_rng_position(int64_t seed, int64_t attempt, int64_t draws, uint64_t out[4]) {
    VgxPcg64 g;
    vgx_pcg64_seed(g, (uint64_t)seed, (uint32_t)attempt);
    // jump ahead: state' = A^n state + (A^n - 1)/(A - 1) inc, by repeated squaring (O(log n))
    uint64_t ah = 0x2360ED051FC65DA4ull, al = 0x4385DF649FCCF645ull;   // multiplier
    uint64_t ch = g.ih, cl = g.il;                                      // increment
    uint64_t acc_mh = 0, acc_ml = 1, acc_ph = 0, acc_pl = 0;
    uint64_t n = (uint64_t)draws;
    while (n > 0) {
        if (n & 1) {
            uint64_t th, tl;
            vgx_mul128(acc_mh, acc_ml, ah, al, th, tl); acc_mh = th; acc_ml = tl;
            vgx_mul128(acc_ph, acc_pl, ah, al, th, tl); acc_ph = th; acc_pl = tl;
            vgx_add128(acc_ph, acc_pl, ch, cl);
        }
        uint64_t th, tl, a1h = ah, a1l = al;
        vgx_add128(a1h, a1l, 0, 1);
        vgx_mul128(a1h, a1l, ch, cl, th, tl); ch = th; cl = tl;
        vgx_mul128(ah, al, ah, al, th, tl); ah = th; al = tl;
        n >>= 1;
    }
    uint64_t sh, sl;
    vgx_mul128(acc_mh, acc_ml, g.sh, g.sl, sh, sl);
    vgx_add128(sh, sl, acc_ph, acc_pl);
    out[0] = sh; out[1] = sl; out[2] = g.ih; out[3] = g.il;
}

// ---- the shared walk (vgx_gwalk.h) ---------------------------------------------------------------------------------------
// What vgx_get_genealogy reports for each walk status (the device pass's statuses become the host pass's messages).
static std::string walk_message(int64_t status, int64_t arg) {
    switch (status) {
    case VGX_GW_OK: return "";
    case VGX_GW_FEW_SAMPLES: return "Less than two cases were sampled...";
    case VGX_GW_EXTRA_SAMPLING: return "vgx_get_genealogy: more sampling events than sCounter";
    case VGX_GW_TREE_OVERFLOW: return "vgx_get_genealogy: tree overflow (event log and sCounter disagree)";
    case VGX_GW_NOT_COALESCED: return "vgx_get_genealogy: lineage " + std::to_string(arg) + " never coalesced (several roots)";
    case VGX_GW_UNKNOWN_TYPE: return "vgx_get_genealogy: unknown event type " + std::to_string(arg);
    case VGX_GW_MULTITYPE: return "vgx_get_genealogy: MULTITYPE event without a multievent log";
    case VGX_GW_MUT_CAP: return "vgx_get_genealogy: mutation record capacity exceeded";
    case VGX_GW_MIG_CAP: return "vgx_get_genealogy: migration record capacity exceeded";
    case VGX_GW_WORKSPACE: return "vgx_get_genealogy: walk workspace exhausted";
    case VGX_GW_STEP_ROWS:
        return "vgx_get_tau_genealogies: step " + std::to_string(arg) + " of the call has more multievent rows than the device sorts (" +
               std::to_string(VGX_GT_STEP_ROWS_MAX) + ")";
    case VGX_GW_UNKNOWN_ROW_TYPE: return "vgx_get_genealogy: unknown multievent type " + std::to_string(arg);
    case VGX_GW_BAD_ROW:
        return "vgx_get_tau_genealogies: a multievent row of event " + std::to_string(arg) + " does not fit the model or the compartment counts";
    case VGX_GW_BAD_TREE:
        return "vgx_get_tree_shapes: node " + std::to_string(arg) + " breaks the tree's structure (every node but the last has a parent of a higher id, " +
               "every node none or two children)";
    case VGX_GW_BAD_RECORD:
        return "vgx_get_mutation_spectrum: mutation record " + std::to_string(arg) + " lies outside the tree or the model (mut_node in [0, nodes), " +
               "mut_site in [0, sites), mut_AS and mut_DS in 0 .. 3)";
    case VGX_GW_BAD_LABEL:
        return "vgx_get_introductions: the label of node " + std::to_string(arg) + " lies outside the model (tree_pop in [0, populations))";
    default: return "vgx_get_genealogy: walk status " + std::to_string(status);
    }
}

extern "C" int vgx_genealogy_message(int64_t status, int64_t arg, char *errbuf, int64_t errcap) {
    if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", walk_message(status, arg).c_str());
    return (int)status;
}

extern "C" int vgx_test_genealogy_walk(vgx_genealogy_io *io, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->infectious || !io->tree || !io->tree_pop || !io->times) return fail("vgx_test_genealogy_walk: null argument");
    if (io->sCounter < 2) return fail(walk_message(VGX_GW_FEW_SAMPLES, 0));
    const int64_t n = io->ev_ptr, PH = io->popNum * io->hapNum;
    if (n < 0 || n >= ((int64_t)1 << 30) || 2 * io->sCounter > ((int64_t)1 << 31)) return fail("vgx_test_genealogy_walk: chain too long");
    // the chain in the device log's record layout
    std::vector<int32_t> log((size_t)n * 6);
    for (int64_t e = 0; e < n; e++) {
        const int64_t v[5] = {io->ev_types[e], io->ev_haplotypes[e], io->ev_populations[e], io->ev_newHaplotypes[e], io->ev_newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_genealogy_walk: log value outside 32 bits");
            log[(size_t)(e * 6 + c)] = (int32_t)v[c];
        }
    }
    const int64_t nodes = 2 * io->sCounter - 1;
    const int64_t tsize = vgx_gw_table_size(n, PH);
    std::vector<int64_t> key((size_t)tsize, -1), cnt((size_t)tsize);
    // (the table's fields other than the key are left as the device leaves them: uninitialised until a slot is taken)
    std::unique_ptr<int32_t[]> base(new int32_t[(size_t)tsize]), len(new int32_t[(size_t)tsize]), lcap(new int32_t[(size_t)tsize]);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(n, 1));
    std::vector<int32_t> tree((size_t)nodes), tree_pop((size_t)nodes), node_ev((size_t)nodes);
    const int64_t mut_cap = std::max<int64_t>(io->mut_cap, 0), mig_cap = std::max<int64_t>(io->mig_cap, 0);
    std::vector<int32_t> mu((size_t)mut_cap * 5 + 1), mg((size_t)mig_cap * 4 + 1);
    VgxGwRep w;
    w.n_ev = n; w.sCounter = io->sCounter; w.H = io->hapNum; w.tsize = tsize;
    w.key = key.data(); w.cnt = cnt.data(); w.base = base.get(); w.len = len.get(); w.lcap = lcap.get();
    w.arena = arena.data(); w.arena_cap = n;
    w.tree = tree.data(); w.tree_pop = tree_pop.data(); w.node_ev = node_ev.data();
    w.mut_cap = mut_cap;
    w.mut_node = mu.data(); w.mut_AS = w.mut_node + mut_cap; w.mut_DS = w.mut_AS + mut_cap; w.mut_site = w.mut_DS + mut_cap;
    w.mut_ev = w.mut_site + mut_cap;
    w.mig_cap = mig_cap;
    w.mig_node = mg.data(); w.mig_old = w.mig_node + mig_cap; w.mig_new = w.mig_old + mig_cap; w.mig_ev = w.mig_new + mig_cap;
    VgxGwFlatReader rd{log.data()};
    VgxGwResult res{};
    res.status = vgx_gw_prepass(w, rd);
    if (res.status != VGX_GW_OK) return fail(walk_message(res.status, res.arg));
    for (int64_t s = 0; s < tsize; s++)   // the counts of the touched compartments
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) cnt[(size_t)s] = io->infectious[key[(size_t)s]];
    VgxPcg64 g{io->rng_state[0], io->rng_state[1], io->rng_state[2], io->rng_state[3]};
    vgx_gw_walk(w, rd, g, res);
    for (int64_t s = 0; s < tsize; s++)   // walked back in place, as the host pass does
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) io->infectious[key[(size_t)s]] = cnt[(size_t)s];
    if (res.status != VGX_GW_OK) return fail(walk_message(res.status, res.arg));
    auto time_of = [&](int32_t e) { return e < 0 ? 0.0 : io->ev_times[e]; };
    for (int64_t i = 0; i < nodes; i++) {
        io->tree[i] = tree[(size_t)i]; io->tree_pop[i] = tree_pop[(size_t)i]; io->times[i] = time_of(node_ev[(size_t)i]);
    }
    io->mut_n = res.mut_n;
    for (int64_t k = 0; k < res.mut_n; k++) {
        io->mut_node[k] = w.mut_node[k]; io->mut_AS[k] = w.mut_AS[k]; io->mut_DS[k] = w.mut_DS[k]; io->mut_site[k] = w.mut_site[k];
        io->mut_time[k] = time_of(w.mut_ev[k]);
    }
    io->mig_n = res.mig_n;
    for (int64_t k = 0; k < res.mig_n; k++) {
        io->mig_node[k] = w.mig_node[k]; io->mig_old[k] = w.mig_old[k]; io->mig_new[k] = w.mig_new[k];
        io->mig_time[k] = time_of(w.mig_ev[k]);
    }
    io->nodes_used = res.nodes_used;
    io->rng_state[0] = g.sh; io->rng_state[1] = g.sl; io->rng_state[2] = g.ih; io->rng_state[3] = g.il;
    return VGX_OK;
}

// ---- lineages on a grid (vgx_lineages.h): the walk with the logging observer, the tile walk and the suffix sum on one chain ------
// With `events` it is vgx_test_tree_events (vgx_tree_events.h): `values` is counts [T + 1][P][V][VGX_TE_K] by vgx_te_tile_host, with no
// root and no suffix sum.
static int lineages_hook(vgx_genealogy_io *io, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile, int32_t *values,
                         int32_t *root, int64_t *records, char *errbuf, int64_t errcap, const bool events, const char *name) {
    const std::string me = std::string(name) + ": ";
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->infectious || !grid || !variant_of || !values || (!events && !root) || !records) return fail(me + "null argument");
    const int64_t P = io->popNum, H = io->hapNum;
    if (T < 1 || T >= VGX_PREV_MAX_POINTS) return fail(me + "T = " + std::to_string(T) + " must be at least 1 and below 2^24");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(grid[k])) return fail(me + "grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(grid[k - 1] < grid[k])) return fail(me + "grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail(me + "bad dimensions");
    if (V < 1 || V > INT32_MAX) return fail(me + "V = " + std::to_string(V) + " must be at least 1");
    if (vgx_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail(me + "" + std::to_string(P) + " populations x " + std::to_string(V) + " classes need " +
                    std::to_string(vgx_prev_lds_bytes(P, V)) + " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) +
                    " bytes of LDS a counting workgroup may use");
    if (events && vgx_te_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail(me + std::to_string(P) + " populations x " + std::to_string(V) + " classes x " + std::to_string(VGX_TE_K) + " channels need " +
                    std::to_string(vgx_te_lds_bytes(P, V)) + " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) +
                    " bytes of LDS a counting workgroup may use");
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return fail(me + "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " +
                        std::to_string(V) + ")");
    if (tile < 0) return fail(me + "tile must not be negative");
    if (tile == 0) tile = VGX_LN_TILE_DEFAULT;
    if (io->sCounter < 2) return fail(walk_message(VGX_GW_FEW_SAMPLES, 0));
    const int64_t n = io->ev_ptr, PH = P * H;
    if (n < 0 || n >= VGX_PREV_MAX_EVENTS) return fail(me + "a chain of " + std::to_string(n) + " events (2^30 or more)");
    if (2 * io->sCounter > ((int64_t)1 << 31)) return fail(me + "sCounter = " + std::to_string(io->sCounter) + " is too large");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail(me + "null event column");
    // the chain in the device log's record layout, and what the sizing kernel counts
    std::vector<int32_t> log((size_t)n * 6);
    int64_t n_mut = 0, n_mig = 0;
    for (int64_t e = 0; e < n; e++) {
        const int64_t v[5] = {io->ev_types[e], io->ev_haplotypes[e], io->ev_populations[e], io->ev_newHaplotypes[e], io->ev_newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail(me + "log value outside 32 bits");
            log[(size_t)(e * 6 + c)] = (int32_t)v[c];
        }
        n_mut += v[0] == VGX_GW_MUTATION;
        n_mig += v[0] == VGX_GW_MIGRATION;
    }
    const int64_t nodes = 2 * io->sCounter - 1;
    const int64_t tsize = vgx_gw_table_size(n, PH);
    std::vector<int64_t> key((size_t)tsize, -1), cnt((size_t)tsize);
    std::unique_ptr<int32_t[]> base(new int32_t[(size_t)tsize]), len(new int32_t[(size_t)tsize]), lcap(new int32_t[(size_t)tsize]);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(n, 1)), tree((size_t)nodes);
    const int64_t rec_cap = vgx_ln_capacity(io->sCounter, n_mut, n_mig);
    std::vector<int32_t> rec((size_t)rec_cap * 6);
    VgxGwRep w{};
    w.n_ev = n; w.sCounter = io->sCounter; w.H = H; w.tsize = tsize;
    w.key = key.data(); w.cnt = cnt.data(); w.base = base.get(); w.len = len.get(); w.lcap = lcap.get();
    w.arena = arena.data(); w.arena_cap = n;
    w.tree = tree.data();   // (the observer keeps no records: the other outputs are never touched)
    VgxGwFlatReader rd{log.data()};
    VgxGwResult res{};
    res.status = vgx_gw_prepass(w, rd);
    if (res.status != VGX_GW_OK) return fail(walk_message(res.status, res.arg));
    for (int64_t s = 0; s < tsize; s++)   // the counts of the touched compartments
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) cnt[(size_t)s] = io->infectious[key[(size_t)s]];
    VgxPcg64 g{io->rng_state[0], io->rng_state[1], io->rng_state[2], io->rng_state[3]};
    VgxLnLog lg{rec.data(), rec_cap, 0, 0};
    vgx_gw_walk(w, rd, g, res, VgxLnObserver{&lg});
    if (res.status == VGX_GW_OK && lg.dropped > 0) res.status = VGX_GW_WORKSPACE;
    for (int64_t s = 0; s < tsize; s++)   // walked back in place, as the host pass does
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) io->infectious[key[(size_t)s]] = cnt[(size_t)s];
    if (res.status != VGX_GW_OK) return fail(walk_message(res.status, res.arg));
    io->nodes_used = res.nodes_used;
    io->rng_state[0] = g.sh; io->rng_state[1] = g.sl; io->rng_state[2] = g.ih; io->rng_state[3] = g.il;
    *records = lg.n;
    // the bounds from the chain's times, the tile walk over the lineage log, the suffix sum
    std::vector<int32_t> bound((size_t)(T + 2));
    VgxPrevCutter ct{grid, T, bound.data()};
    for (int64_t e = 0; e < n; e++) ct.event(e, io->ev_times[e]);
    ct.finish(n);
    if (events) {
        const int64_t cells = P * V * VGX_TE_K;
        for (int64_t i = 0; i < (T + 1) * cells; i++) values[i] = 0;
        std::vector<int32_t> hist((size_t)cells, 0);
        for (int64_t r0 = 0; r0 < lg.n; r0 += tile)
            vgx_te_tile_host(rec.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, variant_of, r0, std::min<int64_t>(r0 + tile, lg.n),
                             hist.data(), values);
        return VGX_OK;
    }
    const int64_t cells = P * V;
    for (int64_t i = 0; i < T * cells; i++) values[i] = 0;
    for (int64_t i = 0; i < cells; i++) root[i] = 0;
    std::vector<int32_t> hist((size_t)cells, 0);
    for (int64_t r0 = 0; r0 < lg.n; r0 += tile)
        vgx_ln_tile_host(rec.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, variant_of, r0, std::min<int64_t>(r0 + tile, lg.n),
                         hist.data(), values, root);
    for (int64_t i = 0; i < cells; i++) vgx_ln_scan_column(values + i, root + i, (int32_t)T, cells);
    return VGX_OK;
}

extern "C" int vgx_test_lineages(vgx_genealogy_io *io, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                                 int32_t *values, int32_t *root, int64_t *records, char *errbuf, int64_t errcap) {
    return lineages_hook(io, grid, T, variant_of, V, tile, values, root, records, errbuf, errcap, false, "vgx_test_lineages");
}

extern "C" int vgx_test_tree_events(vgx_genealogy_io *io, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                                    int32_t *counts, int64_t *records, char *errbuf, int64_t errcap) {
    return lineages_hook(io, grid, T, variant_of, V, tile, counts, nullptr, records, errbuf, errcap, true, "vgx_test_tree_events");
}

// ---- the shape of one tree (vgx_tree_shape.h) -------------------------------------------------------------------
extern "C" int vgx_test_tree_shape(const int32_t *tree, const int32_t *node_ev, const double *times, int64_t nodes, int64_t *stats, double *lengths,
                                   char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!tree || !node_ev || !times || !stats || !lengths) return fail("vgx_test_tree_shape: null argument");
    int64_t bad = vgx_ts_check_parents(tree, nodes);
    if (bad == nodes) return fail("vgx_test_tree_shape: " + std::to_string(nodes) + " nodes: an odd number, at least 3 (node " + std::to_string(nodes) + ")");
    if (bad >= 0)
        return fail("vgx_test_tree_shape: the parent of node " + std::to_string(bad) + " is " + std::to_string(tree[bad]) +
                    " (a higher id inside the tree, -1 at the last node)");
    const size_t N = (size_t)nodes;
    std::vector<int32_t> w32(7 * N);
    std::vector<int64_t> w64(2 * N);
    const VgxTsWork w{w32.data(), w32.data() + N, w32.data() + 2 * N, w32.data() + 3 * N, w32.data() + 4 * N, w32.data() + 5 * N, w32.data() + 6 * N,
                      w64.data(), w64.data() + N};
    bad = vgx_ts_sweep(tree, node_ev, times, nodes, w, stats, lengths);
    if (bad >= 0) return fail("vgx_test_tree_shape: node " + std::to_string(bad) + " has " + std::to_string(w.kids[bad]) + " children (none or two)");
    return VGX_OK;
}

// ---- the mutation spectrum of one tree (vgx_mutation_spectrum.h) ---------------------------------------------------
extern "C" int vgx_test_mutation_spectrum(const int32_t *tree, int64_t nodes, const int32_t *mut_node, const int32_t *mut_AS, const int32_t *mut_DS,
                                          const int32_t *mut_site, int64_t muts, int64_t sites, int64_t *spectrum, int64_t *substitutions, int64_t *sums,
                                          int64_t *stats, int32_t *clade, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    const std::string me = "vgx_test_mutation_spectrum: ";
    if (!tree || !spectrum || !substitutions || !sums || !stats || muts < 0 || (muts > 0 && (!mut_node || !mut_AS || !mut_DS || !mut_site)))
        return fail(me + "null argument");
    if (sites < 0 || sites > VGX_MSP_SITES_MAX) return fail(me + "sites = " + std::to_string(sites) + " (0 .. 15)");
    if (muts >= ((int64_t)1 << 30)) return fail(me + "too many records");
    const int64_t bad = vgx_ts_check_parents(tree, nodes);
    if (bad == nodes) return fail(me + std::to_string(nodes) + " nodes: an odd number, at least 3 (node " + std::to_string(nodes) + ")");
    if (bad >= 0)
        return fail(me + "the parent of node " + std::to_string(bad) + " is " + std::to_string(tree[bad]) + " (a higher id inside the tree, -1 at the last node)");
    const size_t N = (size_t)nodes;
    std::vector<int32_t> w32(4 * N);
    const VgxMspWork w{w32.data(), w32.data() + N, w32.data() + 2 * N, w32.data() + 3 * N};
    int64_t arg = 0;
    const int st = vgx_ms_sweep(tree, nodes, w, mut_node, mut_AS, mut_DS, mut_site, muts, sites, spectrum, substitutions, sums, stats, &arg);
    if (st == VGX_GW_BAD_TREE) return fail(me + "node " + std::to_string(arg) + " has " + std::to_string(w.kids[arg]) + " children (none or two)");
    if (st == VGX_GW_BAD_RECORD)
        return fail(me + "record " + std::to_string(arg) + " (node " + std::to_string(mut_node[arg]) + ", AS " + std::to_string(mut_AS[arg]) + ", DS " +
                    std::to_string(mut_DS[arg]) + ", site " + std::to_string(mut_site[arg]) + ") lies outside the tree of " + std::to_string(nodes) +
                    " nodes or the model of " + std::to_string(sites) + " sites");
    if (clade) std::copy(w.clade, w.clade + N, clade);
    return VGX_OK;
}

// ---- the introductions of one tree (vgx_introductions.h) -----------------------------------------------------------
extern "C" int vgx_test_introductions(const int32_t *tree, const int32_t *pop, int64_t nodes, int64_t pops, int64_t *tips_by_pop, int64_t *imports,
                                      int64_t *into, int64_t *spectrum, int64_t *stats, int32_t *clade, int32_t *local, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) std::snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    const std::string me = "vgx_test_introductions: ";
    if (!tree || !pop || !tips_by_pop || !imports || !into || !spectrum || !stats) return fail(me + "null argument");
    if (pops < 1 || pops > VGX_IN_POPS_MAX) return fail(me + "populations = " + std::to_string(pops) + " (1 .. " + std::to_string(VGX_IN_POPS_MAX) + ")");
    const int64_t bad = vgx_ts_check_parents(tree, nodes);
    if (bad == nodes) return fail(me + std::to_string(nodes) + " nodes: an odd number, at least 3 (node " + std::to_string(nodes) + ")");
    if (bad >= 0)
        return fail(me + "the parent of node " + std::to_string(bad) + " is " + std::to_string(tree[bad]) + " (a higher id inside the tree, -1 at the last node)");
    const size_t N = (size_t)nodes;
    std::vector<int32_t> w32(4 * N);
    const VgxInWork w{w32.data(), w32.data() + N, w32.data() + 2 * N, w32.data() + 3 * N};
    int64_t arg = 0;
    const int st = vgx_in_sweep(tree, pop, nodes, pops, w, clade, local, tips_by_pop, imports, into, spectrum, stats, &arg);
    if (st == VGX_GW_BAD_TREE) return fail(me + "node " + std::to_string(arg) + " has " + std::to_string(w.kids[arg]) + " children (none or two)");
    if (st == VGX_GW_BAD_LABEL)
        return fail(me + "the label of node " + std::to_string(arg) + " is " + std::to_string(pop[arg]) + ", outside the model of " + std::to_string(pops) +
                    " populations");
    return VGX_OK;
}
