// vgx_lineages.h — ancestral lineages of the sample per (population, variant class) of a DIRECT event chain at grid times the
// caller gives, written once for the host and the device: the observer that logs where the backward walk (vgx_gwalk.h) changes a
// lineage list, the signed cells a lineage record changes, the walk of a tile of consecutive records and the suffix sum.
// vgx_lineages.hip runs it over the device log (vgx_get_lineages) and vgx_genealogy.cpp, compiled for the host, behind
// vgx_test_lineages.  DESIGN.md §26.
//
// The walk is vgx_gw_walk: the same draws in the same order.  Whenever it changes a lineage list its observer appends one
// lineage record of six int32 words in the event log's layout: kind, hap, pop, newHap, newPop, ev (the event index).  Read
// FORWARD in time a record changes, with c(h) = variant_of[h] and a side of class -1 skipped,
//   TIP       (a SAMPLING pushes a lineage)                              -1 at (pop, c(hap))
//   SPLIT     (a BIRTH coalesces two lineages of (pop, hap))             +1 at (pop, c(hap))
//   SPLIT     (a MIGRATION coalesces; pop = the event's newPopulation)   +1 at (pop, c(hap))
//   MUTATION  (a MUTATION takes a lineage)                               -1 at (pop, c(hap)), +1 at (pop, c(newHap)); equal classes: nothing
//   MOVE      (a MIGRATION moves a lineage without coalescing)           -1 at (pop, c(hap)), +1 at (newPop, c(hap))
// The walk goes back in time, so a replicate's records lie in DESCENDING ev order.  The grid is prevalence's (vgx_prevalence.h):
// the T + 2 bounds of VgxPrevCutter, a record with event index ev in interval k when bound[k] <= ev < bound[k + 1].  No lineage
// is alive after the last event, so
//   values[j] = -(net change of the intervals j + 1 .. T),   root = -(net change of all intervals) = values[j] - net of 0 .. j
// which is prevalence's running sum with `root` as the start.  Everything after the cuts is integer work.
#pragma once
#include <stdint.h>
#include "vgx_gwalk.h"
#include "vgx_prevalence.h"

#define VGX_LN_TILE_DEFAULT 4096   // records of a tile unless VGX_LINEAGES_TILE_RECORDS says otherwise

enum { VGX_LN_TIP = 0, VGX_LN_SPLIT = 1, VGX_LN_MUTATION = 2, VGX_LN_MOVE = 3 };

// lineage records a chain can write: its nodes, its MUTATION events and its MIGRATION events (none below two samples)
VGX_HD int64_t vgx_ln_capacity(int64_t sCounter, int64_t n_mut, int64_t n_mig) {
    return sCounter >= 2 ? 2 * sCounter - 1 + n_mut + n_mig : 0;
}

// lineage records a TAU chain can write (vgx_tau_lineages.h): its nodes and, for every MUTATION or MIGRATION row, the lineages the
// row can take, min(num, sCounter), where a prefix event of direct type counts 1.  own_*: those sums over the replicate's raw rows
// (merging rows can only lower them), pre_*: over the prefix's rows, 0 for a replicate that restarted.  None below two samples.
VGX_HD int64_t vgx_ln_tau_capacity(int64_t sCounter, int64_t own_mut, int64_t own_mig, int64_t pre_mut, int64_t pre_mig) {
    return sCounter >= 2 ? 2 * sCounter - 1 + own_mut + pre_mut + own_mig + pre_mig : 0;
}

// one replicate's lineage log: `n` records written, `dropped` that found it full (a walk that ends with status 0 drops none)
struct VgxLnLog {
    int32_t *rec;   // [cap][6], 8-byte aligned
    int64_t cap, n, dropped;
};

// the observer of vgx_gw_walk that writes the lineage log; the walk keeps the parents alone (no tree populations, event indices,
// mutation or migration records).  A full log takes no record and never writes past its end.
struct VgxLnObserver {
    static constexpr bool records = false;
    VgxLnLog *lg;
    VGX_HD void put(int32_t kind, int64_t hap, int64_t pop, int64_t nh, int64_t np, int64_t e) {
        if (lg->n >= lg->cap) { lg->dropped += 1; return; }
        int32_t *r = lg->rec + lg->n * 6;
        r[0] = kind; r[1] = (int32_t)hap; r[2] = (int32_t)pop; r[3] = (int32_t)nh; r[4] = (int32_t)np; r[5] = (int32_t)e;
        lg->n += 1;
    }
    VGX_HD void tip(int64_t e, int64_t hap, int64_t pop) { put(VGX_LN_TIP, hap, pop, hap, pop, e); }
    VGX_HD void split(int64_t e, int64_t hap, int64_t pop) { put(VGX_LN_SPLIT, hap, pop, hap, pop, e); }
    VGX_HD void mutation(int64_t e, int64_t hap, int64_t pop, int64_t nh) { put(VGX_LN_MUTATION, hap, pop, nh, pop, e); }
    VGX_HD void move(int64_t e, int64_t hap, int64_t pop, int64_t np) { put(VGX_LN_MOVE, hap, pop, hap, np, e); }
};

// c = kind, hap, pop, newHap, newPop of one lineage record.  Writes the cells (pop * V + class) it changes forward in time with
// their signs and returns how many there are: 0, 1 or 2.  A population outside [0, P) or a haplotype outside [0, hapNum) counts
// nowhere.
VGX_HD int vgx_ln_deltas(const int32_t c[5], int32_t P, int32_t hapNum, int32_t V, const int32_t *variant_of, int32_t cell[2],
                         int32_t sign[2]) {
    const int32_t k = c[0], pop = c[2];
    if (k < VGX_LN_TIP || k > VGX_LN_MOVE || pop < 0 || pop >= P) return 0;
    const int32_t cls = vgx_prev_class(variant_of, hapNum, c[1]);
    int n = 0;
    if (k == VGX_LN_MUTATION) {
        const int32_t to = vgx_prev_class(variant_of, hapNum, c[3]);
        if (cls == to) return 0;
        if (cls >= 0) { cell[n] = pop * V + cls; sign[n++] = -1; }
        if (to >= 0) { cell[n] = pop * V + to; sign[n++] = 1; }
    } else if (cls >= 0) {
        cell[n] = pop * V + cls;
        sign[n++] = k == VGX_LN_SPLIT ? 1 : -1;
        if (k == VGX_LN_MOVE && c[4] >= 0 && c[4] < P) { cell[n] = c[4] * V + cls; sign[n++] = 1; }
    }
    return n;
}

// the interval of event index ev by a search in the bounds, kept inside 0 .. T whatever ev is
VGX_HD int32_t vgx_ln_interval(const int32_t *bound, int32_t T, int32_t ev) {
    const int32_t j = vgx_inc_bin(bound, T + 1, ev);
    return j < 0 ? 0 : (j > T ? T : j);
}

// records [pos, r1) of a log in descending ev order: the end of the run that starts at pos and stays at or above event index
// `lowest` (the first record after pos with ev < lowest, r1 if none).  Always past pos.
VGX_HD int64_t vgx_ln_run_end(const int32_t *rec, int64_t pos, int64_t r1, int32_t lowest) {
    int64_t lo = pos + 1, hi = r1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rec[mid * 6 + 5] >= lowest) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// host: the walk of one tile [r0, r1) of a lineage log as the workgroup does it: the interval of its first record by search, the
// signed cells of `hist` (P * V, zeroed, left zeroed), the nonzero ones added to the interval's net block (vgx_prev_net's layout)
// and cleared at every interval change and at the tile's end.
static inline void vgx_ln_tile_host(const int32_t *rec, const int32_t *bound, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                    const int32_t *variant_of, int64_t r0, int64_t r1, int32_t *hist, int32_t *val, int32_t *fin) {
    const int32_t cells = P * V;
    int64_t pos = r0;
    while (pos < r1) {
        const int32_t j = vgx_ln_interval(bound, T, rec[pos * 6 + 5]);
        const int64_t end = vgx_ln_run_end(rec, pos, r1, bound[j]);
        for (int64_t r = pos; r < end; r++) {
            int32_t cell[2], sign[2];
            const int n = vgx_ln_deltas(rec + r * 6, P, hapNum, V, variant_of, cell, sign);
            for (int k = 0; k < n; k++) hist[cell[k]] += sign[k];
        }
        int32_t *dst = vgx_prev_net(val, fin, 0, T, cells, j);
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// the suffix sum of one (row, cell) column in place: val[j] = -(net of the intervals j + 1 .. T), *fin = -(net of all) = the root.
// The sums wrap as unsigned integers do.
VGX_HD void vgx_ln_scan_column(int32_t *val, int32_t *fin, int32_t T, int64_t stride) {
    uint32_t run = 0u - (uint32_t)*fin;
    for (int32_t j = T - 1; j >= 0; j--) {
        const uint32_t net = (uint32_t)val[(int64_t)j * stride];
        val[(int64_t)j * stride] = (int32_t)run;
        run -= net;
    }
    *fin = (int32_t)run;
}

// ---- device plumbing (vgx_api.hip <-> vgx_lineages.hip) -----------------------------------------------------------------------
// one selected replicate of a walk pass: offsets into the pass's workspace (elements; rec_off in records)
struct VgxLnDesc {
    int64_t rep, n_ev, sCounter, tsize, tab_off, arena_off, arena_cap, node_off, rec_off, rec_cap;
    uint64_t rng[4];
};

struct VgxLnLaunch {
    int64_t m;                      // replicates of this pass
    const VgxLnDesc *desc;          // [m]
    const int32_t *log;             // [R][evcap][6] the device event log
    int64_t evcap;
    const int32_t *nocc, *lhap;     // occupancy lists of the final state: [R][P], [R][P][cap]
    const int64_t *lcnt;            // [R][P][cap]
    int64_t P, H, cap;
    int64_t *key, *cnt;             // compartment tables
    int32_t *base, *len, *lcap, *arena;
    int32_t *tree;                  // parents of the pass's nodes
    int32_t *rec;                   // lineage logs of the pass, [sum of rec_cap][6]
    int64_t *res;                   // [m][5] VgxGwResult
    uint64_t *rng_out;              // [m][4]
    int64_t *n_rec;                 // [m] records the binning reads: those written, 0 for a walk that failed
    // binning and scan
    const int32_t *bound;           // [m][T + 2]
    int32_t T, V;
    const int32_t *variant_of;      // [H]
    int32_t tile;                   // records per tile
    int64_t max_rec;                // largest rec_cap of the pass
    int32_t *val;                   // [m][T][P][V] net changes, zeroed by the caller; values after the scan
    int32_t *fin;                   // [m][P][V] net change of the tail; root after the scan
};
