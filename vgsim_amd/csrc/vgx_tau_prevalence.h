// vgx_tau_prevalence.h — infectious hosts per (population, variant class) of a TAU chain at grid times the caller gives, written
// once for the host and the device: the weighted-row form of vgx_prevalence.h, which supplies the signed cells, the literal cut
// loop (VgxPrevCutter) and the T + 2 bounds.  vgx_tau_prevalence.hip runs it one workgroup per (chain, tile of rows) over the rows
// where they lie (vgx_get_tau_prevalence) and, compiled for the host, tile after tile behind vgx_test_tau_prevalence.
// DESIGN.md §19.
//
// ROWS.  The chain of vgx_tau_incidence.h: weighted rows of six int64 (num, type, haplotype, population, newHaplotype,
// newPopulation), the prefix flattened (vgx_tau_rows.h), then the replicate's own rows in its block of t_mev.  An EVENT is a direct
// event or a step; its time is that of its log record.
// CELLS.  A row changes the cells vgx_prev_deltas gives for its five fields with sign * num; VGX_TL_ROW_DIRECT is masked off the
// type, a field that is not a 32-bit index matches nothing (vgx_tau_inc_idx32), a row with num <= 0 changes nothing.
// BOUNDS, in ROW index space: cut[j] = first row of the first event i with grid[j] < t_i (the row count if none), by the literal
// loop of VgxPrevCutter over EVENTS fed with every event's first row; an event without rows still advances `point` and its cut is
// the first row after it.  Held as T + 2 bounds (bound[0] = 0, bound[j + 1] = cut[j], bound[T + 1] = rows): interval j = 0 .. T
// holds the rows bound[j] <= i < bound[j + 1], so all rows of a step share an interval and a grid point at exactly a step's time
// has the step applied.  OUTSIDE = (sum of num over the rows before cut[0], ... over the rows from cut[T - 1] on), num > 0 only.
// Cells and values are int64: an interval sums num over many steps, and 32 bits do not bound that.  The scan wraps as unsigned
// 64-bit integers do.
//
// PREFIX ONCE.  Net changes add, and with one grid the prefix part of the literal loop is the same for every chain that carries
// the prefix: it consumes the same point0 cuts at the same prefix rows.  So the prefix is a chain of its own with the bounds
// (0, those point0 cuts, then its row count), and a replicate's own rows are a chain relative to its block with the bounds
// (0, point0 zeros, then the loop continued from point0).  The net block of a replicate that did not restart STARTS from the
// prefix's net block (the T value intervals, the tail interval and `outside`), its own rows are added on top, and one running sum
// over the total gives the values: the sum of two net blocks is the net block of the whole chain, interval by interval.
#pragma once
#include <stdint.h>
#include "vgx_prevalence.h"
#include "vgx_tau_incidence.h"   // vgx_tau_inc_idx32

// LDS bytes of the P * V signed int64 cells of a counting workgroup (the budget is VGX_PREV_LDS_MAX)
VGX_HD int64_t vgx_tau_prev_lds_bytes(int64_t P, int64_t V) { return 8 * P * V; }

// is variant_of (hapNum int32) staged in LDS behind the cells?
VGX_HD bool vgx_tau_prev_stage_map(int64_t P, int64_t V, int64_t hapNum) { return 8 * P * V + 4 * hapNum <= VGX_PREV_LDS_MAX; }

// One row (num, type, haplotype, population, newHaplotype, newPopulation): the cells it changes (n = 0, 1 or 2) with their signs.
// Returns the weight num, or 0 when the row changes nothing.
VGX_HD int64_t vgx_tau_prev_row(int64_t num, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np, int32_t P, int32_t hapNum,
                                int32_t V, const int32_t *variant_of, int32_t cell[2], int32_t sign[2], int &n) {
    n = 0;
    if (num <= 0) return 0;
    const int32_t c[5] = {vgx_tau_inc_idx32(type & ~(int64_t)VGX_TL_ROW_DIRECT), vgx_tau_inc_idx32(hap), vgx_tau_inc_idx32(pop),
                          vgx_tau_inc_idx32(nh), vgx_tau_inc_idx32(np)};
    n = vgx_prev_deltas(c, P, hapNum, V, variant_of, cell, sign);
    return n > 0 ? num : 0;
}

// Where the net change of interval j of chain `row` lies: the intervals 0 .. T-1 in val[m][T][cells], the tail interval T in
// fin[m][cells] (vgx_prev_net for int64 cells)
VGX_HD int64_t *vgx_tau_prev_net(int64_t *val, int64_t *fin, int64_t row, int32_t T, int32_t cells, int32_t j) {
    return j < T ? val + (row * T + j) * cells : fin + row * cells;
}

// a + b wrapping as unsigned 64-bit integers do (what the device's atomics compute)
VGX_HD int64_t vgx_tau_prev_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// host: the walk of one tile [e0, e1) of a chain (rows = n records of 6 int64) as the workgroup does it: first interval by search,
// the signed cells of `hist` (P * V, zeroed, left zeroed), the nonzero ones added to the interval's net block and cleared at every
// interval change and at the tile's end.  Rows before bound[1] and from bound[T] on still count in their interval (0 or the tail)
// and add their positive num to outside[0 / 1].
static inline void vgx_tau_prev_tile_host(const int64_t *rows, const int32_t *bound, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                          const int32_t *variant_of, int32_t e0, int32_t e1, int64_t *hist, int64_t *val, int64_t *fin,
                                          int64_t *outside) {
    const int32_t cells = P * V;
    int32_t pos = e0;
    while (pos < e1) {
        const int32_t j = vgx_inc_bin(bound, T + 1, pos);
        const int32_t end = e1 < bound[j + 1] ? e1 : bound[j + 1];
        for (int32_t e = pos; e < end; e++) {
            const int64_t *v = rows + (int64_t)e * 6;
            if (v[0] > 0) {
                if (e < bound[1]) outside[0] = vgx_tau_prev_add(outside[0], v[0]);
                else if (e >= bound[T]) outside[1] = vgx_tau_prev_add(outside[1], v[0]);
            }
            int32_t cell[2], sign[2];
            int n;
            const int64_t w = vgx_tau_prev_row(v[0], v[1], v[2], v[3], v[4], v[5], P, hapNum, V, variant_of, cell, sign, n);
            for (int k = 0; k < n; k++) hist[cell[k]] = vgx_tau_prev_add(hist[cell[k]], sign[k] < 0 ? -w : w);
        }
        int64_t *dst = vgx_tau_prev_net(val, fin, 0, T, cells, j);
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] = vgx_tau_prev_add(dst[i], hist[i]); hist[i] = 0; }
        pos = end;
    }
}

// the running sum of one (chain, cell) column in 64 bits (vgx_prev_scan_column for int64 cells): val[j] = start + net of the
// intervals 0 .. j, fin = the same over all T + 1.  The sums wrap as unsigned 64-bit integers do.
VGX_HD void vgx_tau_prev_scan_column(int64_t *val, int64_t *fin, int64_t start, int32_t T, int64_t stride) {
    uint64_t run = (uint64_t)start;
    for (int32_t j = 0; j < T; j++) {
        run += (uint64_t)val[(int64_t)j * stride];
        val[(int64_t)j * stride] = (int64_t)run;
    }
    *fin = (int64_t)(run + (uint64_t)*fin);
}

// launch arguments of the counting and scan kernels (vgx_tau_prevalence.hip), filled by vgx_get_tau_prevalence
struct VgxTauPrevLaunch {
    int64_t m;               // chains of this launch
    const int64_t *rows;     // the prefix rows [n][6], or t_mev: [R][stride][6]
    int64_t stride;          // rows between the blocks of two replicates
    const int64_t *rep;      // [m] replicate of every chain; NULL: one chain at `rows`
    const int32_t *n_rows;   // [m] rows of the chain
    const int32_t *bound;    // [m][T + 2] relative to the chain's first row
    int32_t T, P, hapNum, V;
    const int32_t *variant_of;   // [hapNum]
    int32_t tile;            // rows per tile
    int64_t max_n;           // longest chain of the launch
    int64_t *val;            // [m][T][P][V] net changes; values after the scan
    int64_t *fin;            // [m][P][V] net change of the tail; final after the scan
    int64_t *outside;        // [m][2]
    const int64_t *start;    // [m][P][V] (scan only)
};
