// vgx_tree_events.h — the events of the sampled tree per interval of a grid, population, variant class and kind, written once for
// the host and the device: the cells a lineage record counts at and the walk of a tile of consecutive records.  The log is the
// lineage log of vgx_lineages.h (VgxLnObserver, six int32 words per record: kind, hap, pop, newHap, newPop, ev), written by the
// same walks; vgx_lineages.h collapses a record into a signed net change, this rule keeps the kinds apart.  vgx_tree_events.hip
// runs it over the device logs (vgx_get_tree_events, vgx_get_tau_tree_events) and the host hooks (vgx_test_tree_events,
// vgx_test_tau_tree_events) tile after tile.  DESIGN.md §28.
//
// Read FORWARD in time, with c(h) = variant_of[h] through vgx_prev_class, a record counts +1 at the cells (pop, class, channel)
//   0 samples           TIP                                                          (pop, c(hap))
//   1 coalescences      SPLIT (a BIRTH, or a MIGRATION that coalesces: pop is then   (pop, c(hap))
//                       the event's newPopulation, as the observer writes it)
//   2 mutations_within  MUTATION with c(hap) == c(newHap) >= 0                       (pop, c(hap))
//   3 mutations_out     MUTATION with c(hap) >= 0 and c(newHap) != c(hap)            (pop, c(hap))
//   4 mutations_in      MUTATION with c(newHap) >= 0 and c(newHap) != c(hap)         (pop, c(newHap))
//   5 departures        MOVE with c(hap) >= 0                                        (pop, c(hap))
//   6 arrivals          MOVE with c(hap) >= 0 and newPop inside [0, P)               (newPop, c(hap))
// so a record touches 0, 1 or 2 cells.  A class of -1, a population outside [0, P), a haplotype outside [0, hapNum) and a kind
// outside the four count nowhere, exactly where vgx_ln_deltas counts nothing, and by construction, for every cell (pop, class) and
// every interval,
//   coalescences - samples + mutations_in - mutations_out + arrivals - departures == the net change of vgx_ln_deltas
// so the block contains the block of vgx_get_lineages: values[j] = root + net of the intervals 0 .. j, root = -(net of all).
// The grid is that of vgx_lineages.h: the T + 2 bounds of VgxPrevCutter, a record with event index ev in interval i = 0 .. T when
// bound[i] <= ev < bound[i + 1]; interval T (the tail after the last grid time) is an ordinary row of the block
//   counts[T + 1][P][V][VGX_TE_K]
// whose cell order (pop * V + class) * VGX_TE_K + channel is also the order in LDS: 7 is odd, so the lanes of one atomic
// instruction (one channel for records of one kind) spread over the 64 banks as their (pop, class) cells do, as in vgxl_bin_kernel,
// and nothing is reordered on the flush.  Counts are int32 on both paths: a log holds at most vgx_ln_capacity or vgx_ln_tau_capacity records, which the calls
// bound below 2^31 (chains below 2^30 events and 2 sCounter at most 2^31), and no cell can count more than the log holds.
// Everything after the cuts is integer addition.
#pragma once
#include <stdint.h>
#include "vgx_lineages.h"

#define VGX_TE_K 7   // channels
enum { VGX_TE_SAMPLES = 0, VGX_TE_COALESCENCES = 1, VGX_TE_MUT_WITHIN = 2, VGX_TE_MUT_OUT = 3, VGX_TE_MUT_IN = 4, VGX_TE_DEPARTURES = 5,
       VGX_TE_ARRIVALS = 6 };

// LDS bytes of the P * V * VGX_TE_K int32 cells of a counting workgroup (the budget is VGX_PREV_LDS_MAX)
VGX_HD int64_t vgx_te_lds_bytes(int64_t P, int64_t V) { return 4 * VGX_TE_K * P * V; }

// is variant_of (hapNum int32) staged in LDS behind the cells?
VGX_HD bool vgx_te_stage_map(int64_t P, int64_t V, int64_t hapNum) { return vgx_te_lds_bytes(P, V) + 4 * hapNum <= VGX_PREV_LDS_MAX; }

// c = kind, hap, pop, newHap, newPop of one lineage record.  Writes the cells ((pop * V + class) * VGX_TE_K + channel) it counts at
// and returns how many there are: 0, 1 or 2.
VGX_HD int vgx_te_cells(const int32_t c[5], int32_t P, int32_t hapNum, int32_t V, const int32_t *variant_of, int32_t cell[2]) {
    const int32_t k = c[0], pop = c[2];
    if (k < VGX_LN_TIP || k > VGX_LN_MOVE || pop < 0 || pop >= P) return 0;
    const int32_t cls = vgx_prev_class(variant_of, hapNum, c[1]);
    int n = 0;
    if (k == VGX_LN_MUTATION) {
        const int32_t to = vgx_prev_class(variant_of, hapNum, c[3]);
        if (cls == to) {
            if (cls >= 0) cell[n++] = (pop * V + cls) * VGX_TE_K + VGX_TE_MUT_WITHIN;
        } else {
            if (cls >= 0) cell[n++] = (pop * V + cls) * VGX_TE_K + VGX_TE_MUT_OUT;
            if (to >= 0) cell[n++] = (pop * V + to) * VGX_TE_K + VGX_TE_MUT_IN;
        }
    } else if (cls >= 0) {
        if (k == VGX_LN_MOVE) {
            cell[n++] = (pop * V + cls) * VGX_TE_K + VGX_TE_DEPARTURES;
            if (c[4] >= 0 && c[4] < P) cell[n++] = (c[4] * V + cls) * VGX_TE_K + VGX_TE_ARRIVALS;
        } else {
            cell[n++] = (pop * V + cls) * VGX_TE_K + (k == VGX_LN_SPLIT ? VGX_TE_COALESCENCES : VGX_TE_SAMPLES);
        }
    }
    return n;
}

// host: the walk of one tile [r0, r1) of a lineage log as the workgroup does it (vgx_ln_tile_host with the kinds kept apart): the
// interval of its first record by search, the cells of `hist` (P * V * VGX_TE_K, zeroed, left zeroed), the nonzero ones added to
// the interval's row of counts [T + 1][P][V][VGX_TE_K] and cleared at every interval change and at the tile's end.
static inline void vgx_te_tile_host(const int32_t *rec, const int32_t *bound, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                    const int32_t *variant_of, int64_t r0, int64_t r1, int32_t *hist, int32_t *counts) {
    const int32_t cells = P * V * VGX_TE_K;
    int64_t pos = r0;
    while (pos < r1) {
        const int32_t j = vgx_ln_interval(bound, T, rec[pos * 6 + 5]);
        const int64_t end = vgx_ln_run_end(rec, pos, r1, bound[j]);
        for (int64_t r = pos; r < end; r++) {
            int32_t cell[2];
            const int n = vgx_te_cells(rec + r * 6, P, hapNum, V, variant_of, cell);
            for (int k = 0; k < n; k++) hist[cell[k]] += 1;
        }
        int32_t *dst = counts + (int64_t)j * cells;
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// ---- device plumbing (vgx_api.hip, vgx_tau_lineages.hip <-> vgx_tree_events.hip) ----------------------------------------------
// what the binning kernel reads of a walk pass (the walk's own launch is VgxLnLaunch or VgxTauLnLaunch)
struct VgxTeLaunch {
    int64_t m;                      // replicates of this pass
    const VgxLnDesc *desc;          // [m] where every replicate's log lies: rec_off, rec_cap
    const int32_t *rec;             // lineage logs of the pass, [sum of rec_cap][6]
    const int64_t *n_rec;           // [m] records to bin: those written, 0 for a walk that failed
    const int32_t *bound;           // [m][T + 2]
    int32_t T, P, H, V;
    const int32_t *variant_of;      // [H]
    int32_t tile;                   // records per tile
    int64_t max_rec;                // largest rec_cap of the pass
    int32_t *counts;                // [m][T + 1][P][V][VGX_TE_K], zeroed by the caller
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_te_bin(const VgxTeLaunch *a, hipStream_t s);
#pragma GCC visibility pop
#endif
