// vgx_gwalk.h — the backward walk of a DIRECT event chain (GetGenealogy's event types BIRTH, DEATH, SAMPLING, MUTATION,
// SUSCCHANGE, MIGRATION, reference src/_BirthDeath.pyx:797-872, and the closing pass pyx:998-1000), written once for the
// host and the device.  vgx_genealogies.hip runs it one replicate per lane over the device log; vgx_genealogy.cpp runs the
// host instance behind vgx_test_genealogy_walk.  Operation for operation it is Pass::single of vgx_genealogy.cpp: the same
// PCG64 next_double draws in the same order, the same floor(lbs * u) indices, the same swap-with-last / push-back order in
// every compartment's lineage list, the same IEEE divisions (the build keeps -ffp-contract=off).
//
// State of one replicate, O(events + sCounter) and never O(P x H):
//   * a compartment table, open addressing keyed by pop * H + hap, holding every compartment an event of the chain
//     touches: its infectious count (seeded from the final state, walked back) and its lineage list;
//   * an arena of lineage lists: the list of a compartment is a contiguous segment as long as the number of events that
//     can push a lineage into it (SAMPLING, MUTATION and MIGRATION into their own compartment), found by a pre-pass
//     over the log.  A list never holds more lineages than were pushed into it, so the segment cannot overflow.
// The walk writes event INDICES where the host pass writes times: the caller maps them through its clock (-1 = 0.0).
#pragma once
#include <math.h>
#include <stdint.h>
#include "vgx_rng.h"

// status of one replicate's walk (vgx_genealogy_message gives the host pass's text for each)
enum {
    VGX_GW_OK = 0,
    VGX_GW_FEW_SAMPLES = 1,       // sCounter < 2 (pyx:762-765)
    VGX_GW_EXTRA_SAMPLING = 2,    // more sampling events than sCounter
    VGX_GW_TREE_OVERFLOW = 3,     // more nodes than 2 sCounter - 1
    VGX_GW_NOT_COALESCED = 4,     // arg = the lineage without a parent
    VGX_GW_UNKNOWN_TYPE = 5,      // arg = the event type
    VGX_GW_MULTITYPE = 6,         // a MULTITYPE event with rows: not a direct chain
    VGX_GW_MUT_CAP = 7,
    VGX_GW_MIG_CAP = 8,
    VGX_GW_WORKSPACE = 9          // compartment table or lineage segment full (cannot happen with the sizes of vgx_gw_table_size)
};

enum { VGX_GW_BIRTH = 0, VGX_GW_DEATH = 1, VGX_GW_SAMPLING = 2, VGX_GW_MUTATION = 3, VGX_GW_SUSCCHANGE = 4, VGX_GW_MIGRATION = 5,
       VGX_GW_MULTITYPE_EV = 6 };

// one replicate: workspace and outputs (pointers private to it)
struct VgxGwRep {
    int64_t n_ev;        // the walk covers log indices [0, n_ev)
    int64_t sCounter;
    int64_t H;
    int64_t tsize;       // compartment table slots (power of two)
    int64_t *key;        // [tsize] pop * H + hap, -1 = empty
    int64_t *cnt;        // [tsize] infectious count
    int32_t *base, *len, *lcap;   // [tsize] lineage segment in the arena, its length and capacity
    int32_t *arena;      // [arena_cap]
    int64_t arena_cap;
    int32_t *tree, *tree_pop, *node_ev;                      // [2 sCounter - 1]
    int64_t mut_cap;
    int32_t *mut_node, *mut_AS, *mut_DS, *mut_site, *mut_ev;  // [mut_cap]
    int64_t mig_cap;
    int32_t *mig_node, *mig_old, *mig_new, *mig_ev;           // [mig_cap]
};

struct VgxGwResult {
    int64_t status, arg, nodes_used, mut_n, mig_n;
};

// table slots for a chain of n_ev events on a P x H model: at most two compartments per event, at most P x H in all, at
// load factor <= 1/2
VGX_HD int64_t vgx_gw_table_size(int64_t n_ev, int64_t PH) {
    int64_t distinct = 2 * n_ev < PH ? 2 * n_ev : PH;
    int64_t t = 16;
    while (t < 2 * distinct) t *= 2;
    return t;
}

VGX_HD uint64_t vgx_gw_hash(int64_t k) {
    uint64_t h = (uint64_t)k * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

VGX_HD int64_t vgx_gw_find(const VgxGwRep &w, int64_t k) {   // slot of compartment k, -1 if absent
    const uint64_t m = (uint64_t)w.tsize - 1;
    uint64_t s = vgx_gw_hash(k) & m;
    for (int64_t i = 0; i < w.tsize; i++) {
        const int64_t kk = w.key[s];
        if (kk == k) return (int64_t)s;
        if (kk < 0) return -1;
        s = (s + 1) & m;
    }
    return -1;
}

VGX_HD int64_t vgx_gw_insert(VgxGwRep &w, int64_t k) {   // slot of compartment k, made if absent; -1 = table full
    const uint64_t m = (uint64_t)w.tsize - 1;
    uint64_t s = vgx_gw_hash(k) & m;
    for (int64_t i = 0; i < w.tsize; i++) {
        const int64_t kk = w.key[s];
        if (kk == k) return (int64_t)s;
        if (kk < 0) {
            w.key[s] = k; w.cnt[s] = 0; w.base[s] = 0; w.len[s] = 0; w.lcap[s] = 0;
            return (int64_t)s;
        }
        s = (s + 1) & m;
    }
    return -1;
}

// A log record: type, haplotype, population, newHaplotype, newPopulation.  Rd::at(e, c) fills c[0..4] for log index e.
// Pre-pass: every compartment the chain touches goes into the table; every push into a compartment reserves a slot of
// its segment.  Returns VGX_GW_OK or VGX_GW_WORKSPACE.
template <class Rd>
VGX_HD int vgx_gw_prepass(VgxGwRep &w, Rd &rd) {
    int32_t c[5];
    for (int64_t e = w.n_ev - 1; e >= 0; --e) {
        rd.at(e, c);
        const int64_t type = c[0], hap = c[1], pop = c[2], nh = c[3], np = c[4];
        int64_t s0 = 0, s1 = 0;
        switch (type) {
        case VGX_GW_BIRTH: case VGX_GW_DEATH: s0 = vgx_gw_insert(w, pop * w.H + hap); break;
        case VGX_GW_SAMPLING: s0 = vgx_gw_insert(w, pop * w.H + hap); if (s0 >= 0) w.lcap[s0] += 1; break;
        case VGX_GW_MUTATION:
            s0 = vgx_gw_insert(w, pop * w.H + nh);
            s1 = vgx_gw_insert(w, pop * w.H + hap);
            if (s1 >= 0) w.lcap[s1] += 1;
            break;
        case VGX_GW_MIGRATION:
            s0 = vgx_gw_insert(w, np * w.H + hap);
            s1 = vgx_gw_insert(w, pop * w.H + hap);
            if (s1 >= 0) w.lcap[s1] += 1;
            break;
        default: break;   // (the walk reports what it cannot walk where it meets it)
        }
        if (s0 < 0 || s1 < 0) return VGX_GW_WORKSPACE;
    }
    int64_t acc = 0;   // segments in slot order (the fields of empty slots are not initialised)
    for (int64_t s = 0; s < w.tsize; s++) {
        if (w.key[s] < 0) continue;
        w.base[s] = (int32_t)acc;
        acc += w.lcap[s];
    }
    return acc <= w.arena_cap ? VGX_GW_OK : VGX_GW_WORKSPACE;
}

// The observer of a walk is told where the walk changes a lineage list: a SAMPLING that pushes a lineage (tip), a BIRTH or a
// MIGRATION that coalesces two (split; the migration's with pop = the event's newPopulation, where the lineage it takes away
// lay), a MUTATION that takes a lineage (mutation) and a MIGRATION that moves one without coalescing (move), which leaves no
// record at its own event.  `records` says whether the walk keeps the tree's populations and event indices and the mutation and
// migration records; without them it keeps the parents alone (the closing pass needs them) and counts what it would have
// written.  The default observes nothing and keeps everything: a walk with it is the walk without an observer.
struct VgxGwNoObserver {
    static constexpr bool records = true;
    VGX_HD void tip(int64_t, int64_t, int64_t) {}
    VGX_HD void split(int64_t, int64_t, int64_t) {}
    VGX_HD void mutation(int64_t, int64_t, int64_t, int64_t) {}
    VGX_HD void move(int64_t, int64_t, int64_t, int64_t) {}
};

template <class Obs>
struct VgxGwWalkT {
    VgxGwRep &w;
    VgxPcg64 &g;
    VgxGwResult &res;
    int64_t ptr, nodes;
    Obs obs{};

    VGX_HD double uniform() { return vgx_pcg64_double(g); }
    VGX_HD int32_t &at(int64_t s, int64_t i) { return w.arena[w.base[s] + i]; }
    VGX_HD bool push(int64_t s, int64_t id) {
        if (w.len[s] >= w.lcap[s]) { res.status = VGX_GW_WORKSPACE; return false; }
        w.arena[w.base[s] + w.len[s]] = (int32_t)id;
        w.len[s] += 1;
        return true;
    }
    VGX_HD void swap_pop(int64_t s, int64_t i) { at(s, i) = at(s, w.len[s] - 1); w.len[s] -= 1; }
    VGX_HD void parent(int64_t id, int64_t par) { if (id >= 0 && id < nodes) w.tree[id] = (int32_t)par; }
    VGX_HD void node(int64_t pop, int64_t e) {
        if (ptr < nodes) {
            w.tree[ptr] = -1;
            if (Obs::records) { w.tree_pop[ptr] = (int32_t)pop; w.node_ev[ptr] = (int32_t)e; }
        }
        ptr += 1;
    }
    VGX_HD bool mutation(int64_t nodeId, int64_t hap, int64_t nh, int64_t e) {   // models.pxi:13-29
        if (!Obs::records) { res.mut_n += 1; return true; }
        if (res.mut_n >= w.mut_cap) { res.status = VGX_GW_MUT_CAP; return false; }
        int64_t d = nh > hap ? nh - hap : hap - nh, site = 0, digit4 = 1;
        while (d >= 4) { d /= 4; site += 1; digit4 *= 4; }
        const int64_t k = res.mut_n++;
        w.mut_node[k] = (int32_t)nodeId; w.mut_DS[k] = (int32_t)((nh / digit4) % 4); w.mut_AS[k] = (int32_t)((hap / digit4) % 4);
        w.mut_site[k] = (int32_t)site; w.mut_ev[k] = (int32_t)e;
        return true;
    }
    VGX_HD bool migration(int64_t nodeId, int64_t e, int64_t oldPop, int64_t newPop) {   // models.pxi:44-48
        if (!Obs::records) { res.mig_n += 1; return true; }
        if (res.mig_n >= w.mig_cap) { res.status = VGX_GW_MIG_CAP; return false; }
        const int64_t k = res.mig_n++;
        w.mig_node[k] = (int32_t)nodeId; w.mig_ev[k] = (int32_t)e; w.mig_old[k] = (int32_t)oldPop; w.mig_new[k] = (int32_t)newPop;
        return true;
    }

    // one event (pyx:797-872); false = the walk stops with res.status set
    VGX_HD bool single(int64_t e, const int32_t c[5]) {
        const int64_t type = c[0], hap = c[1], pop = c[2], nh = c[3], np = c[4];
        const int64_t H = w.H;
        switch (type) {
        case VGX_GW_BIRTH: {
            const int64_t s = vgx_gw_find(w, pop * H + hap);
            const int64_t lbs = w.len[s], lbs_e = w.cnt[s];
            const double p = (double)lbs * ((double)lbs - 1.0) / (double)lbs_e / ((double)lbs_e - 1.0);
            if (uniform() < p) {
                int64_t n1 = (int64_t)floor(lbs * uniform());
                int64_t n2 = (int64_t)floor((lbs - 1) * uniform());
                if (n2 >= n1) n2 += 1;
                const int64_t id1 = at(s, n1), id2 = at(s, n2), id3 = ptr;
                at(s, n1) = (int32_t)id3;
                swap_pop(s, n2);
                parent(id1, id3); parent(id2, id3);
                node(pop, e);
                obs.split(e, hap, pop);
            }
            w.cnt[s] -= 1;
            return true;
        }
        case VGX_GW_DEATH: w.cnt[vgx_gw_find(w, pop * H + hap)] += 1; return true;
        case VGX_GW_SAMPLING: {
            const int64_t s = vgx_gw_find(w, pop * H + hap);
            w.cnt[s] += 1;
            if (!push(s, ptr)) return false;
            node(pop, e);
            obs.tip(e, hap, pop);
            return true;
        }
        case VGX_GW_MUTATION: {
            const int64_t sn = vgx_gw_find(w, pop * H + nh), sh = vgx_gw_find(w, pop * H + hap);
            const int64_t lbs = w.len[sn];
            const double p = (double)lbs / (double)w.cnt[sn];
            if (uniform() < p) {
                int64_t n1 = (int64_t)floor(lbs * uniform());
                const int64_t id1 = at(sn, n1);
                swap_pop(sn, n1);
                if (!push(sh, id1)) return false;
                if (!mutation(id1, hap, nh, e)) return false;
                obs.mutation(e, hap, pop, nh);
            }
            w.cnt[sn] -= 1;
            w.cnt[sh] += 1;
            return true;
        }
        case VGX_GW_SUSCCHANGE: return true;
        case VGX_GW_MIGRATION: {
            const int64_t st = vgx_gw_find(w, np * H + hap), ss = vgx_gw_find(w, pop * H + hap);
            const int64_t lbs = w.len[st];
            const double p = (double)lbs / (double)w.cnt[st];
            if (uniform() < p) {
                int64_t nt = (int64_t)floor(lbs * uniform());
                const int64_t lbss = w.len[ss];
                const double p1 = (double)lbss / (double)w.cnt[ss];
                if (uniform() < p1) {
                    int64_t ns = (int64_t)floor(lbss * uniform());
                    const int64_t idt = at(st, nt), ids = at(ss, ns), id3 = ptr;
                    at(ss, ns) = (int32_t)id3;
                    swap_pop(st, nt);
                    parent(idt, id3); parent(ids, id3);
                    node(pop, e);
                    if (!migration(idt, e, pop, np)) return false;
                    obs.split(e, hap, np);
                } else {
                    if (!push(ss, at(st, nt))) return false;
                    swap_pop(st, nt);
                    obs.move(e, hap, pop, np);
                }
            }
            w.cnt[st] -= 1;
            return true;
        }
        case VGX_GW_MULTITYPE_EV:
            if (hap < pop) { res.status = VGX_GW_MULTITYPE; return false; }   // rows [hap, pop): none here
            return true;
        default: res.status = VGX_GW_UNKNOWN_TYPE; res.arg = type; return false;
        }
    }
};
using VgxGwWalk = VgxGwWalkT<VgxGwNoObserver>;

// The walk over [0, n_ev) from the last event back, then the closing pass (pyx:998-1000).  The table must hold the
// pre-pass's compartments with their final infectious counts.  `g` advances by the draws made.  The draws, their order and the
// generator afterwards do not depend on the observer.
template <class Rd, class Obs = VgxGwNoObserver>
VGX_HD void vgx_gw_walk(VgxGwRep &w, Rd &rd, VgxPcg64 &g, VgxGwResult &res, Obs obs = Obs{}) {
    res.status = VGX_GW_OK; res.arg = 0; res.nodes_used = 0; res.mut_n = 0; res.mig_n = 0;
    if (w.sCounter < 2) { res.status = VGX_GW_FEW_SAMPLES; return; }
    const int64_t nodes = 2 * w.sCounter - 1;
    for (int64_t i = 0; i < nodes; i++) {
        w.tree[i] = 0;
        if (Obs::records) { w.tree_pop[i] = 0; w.node_ev[i] = -1; }
    }
    VgxGwWalkT<Obs> k{w, g, res, 0, nodes, obs};
    int32_t c[5];
    for (int64_t e = w.n_ev - 1; e >= 0; --e) {
        rd.at(e, c);
        if (k.ptr >= nodes && c[0] == VGX_GW_SAMPLING) { res.status = VGX_GW_EXTRA_SAMPLING; return; }
        if (!k.single(e, c)) return;
        if (k.ptr > nodes) { res.status = VGX_GW_TREE_OVERFLOW; return; }
    }
    res.nodes_used = k.ptr;
    for (int64_t i = 0; i < 2 * w.sCounter - 2; i++) {
        const int64_t par = w.tree[i];
        if (par < 0 || par >= nodes) { res.status = VGX_GW_NOT_COALESCED; res.arg = i; return; }
        // (these migration records of the closing pass change no lineage list: the observer is not told)
        if (Obs::records && w.tree_pop[par] != w.tree_pop[i] && !k.migration(i, w.node_ev[i], w.tree_pop[par], w.tree_pop[i])) return;
    }
}

// the reader of a log held as int32 records [n][6] (the device log's layout) in memory the caller can address directly
struct VgxGwFlatReader {
    const int32_t *log;
    VGX_HD void at(int64_t e, int32_t c[5]) const {
        const int32_t *r = log + e * 6;
        c[0] = r[0]; c[1] = r[1]; c[2] = r[2]; c[3] = r[3]; c[4] = r[4];
    }
};

// ---- device plumbing (vgx_api.hip <-> vgx_genealogies.hip) ----------------------------------------------------------------
// one selected replicate of a device pass: offsets into the pass's workspace and output arrays (elements)
struct VgxGwDesc {
    int64_t rep, n_ev, sCounter, tsize, tab_off, arena_off, arena_cap, node_off, mut_off, mut_cap, mig_off, mig_cap;
    uint64_t rng[4];
};

struct VgxGwLaunch {
    int64_t n;                      // replicates of this pass
    const VgxGwDesc *desc;          // [n]
    const int32_t *log;             // [R][evcap][6] the device event log (slot 0 = log index 0)
    int64_t evcap;
    const int32_t *nocc, *lhap;     // occupancy lists of the final state: [R][P], [R][P][cap]
    const int64_t *lcnt;            // [R][P][cap]
    int64_t P, H, cap;
    int64_t *key, *cnt;             // compartment tables
    int32_t *base, *len, *lcap, *arena;
    int32_t *tree, *tree_pop, *node_ev;
    int32_t *mut_node, *mut_AS, *mut_DS, *mut_site, *mut_ev;
    int32_t *mig_node, *mig_old, *mig_new, *mig_ev;
    int64_t *res;                   // [n][5] VgxGwResult
    uint64_t *rng_out;              // [n][4]
};
