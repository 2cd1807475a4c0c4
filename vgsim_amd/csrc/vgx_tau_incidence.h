// vgx_tau_incidence.h — incidence of a TAU chain on a grid of time bins the caller gives, written once for the host and the
// device: the weighted-row form of vgx_incidence.h, which supplies the cells, the channels, the bin search and the literal cut
// loop.  vgx_tau_incidence.hip runs it one workgroup per (chain, tile of rows) over the rows where they lie
// (vgx_get_tau_incidence) and, compiled for the host, tile after tile behind vgx_test_tau_incidence.  DESIGN.md §17.
//
// ROWS.  A tau replicate's chain is the list of weighted rows of vgx_tau_timelines.hip, six int64 (num, type, haplotype,
// population, newHaplotype, newPopulation): the model's chain before the call (the prefix) flattened (a direct event = a row with
// num 1, a MULTITYPE event of an earlier tau call = its multievent rows), then the replicate's own rows in its block of t_mev.
// An EVENT is a direct event or a step; its time is the f64 time of its log record, for a step that of its MULTITYPE record.
// CELLS.  A row counts `num` times in the cells vgx_inc_cells gives for its five fields; VGX_TL_ROW_DIRECT is masked off the
// type (incidence knows no direct / multievent difference), num <= 0 counts nothing, a field that is not a 32-bit index matches
// nothing.
// CUTS, in ROW index space: cut[k] = first row of the first event i with edges[k] <= t_i (the row count if none), by the literal
// loop of VgxIncCutter over EVENTS fed with every event's first row; an event without rows still advances `point` and its cut
// is the first row after it.  Row j lies in bin b when cut[b] <= j < cut[b + 1]: all rows of a step share a bin.
// OUTSIDE = (sum of num over the rows before cut[0], ... over the rows from cut[T] on), over num > 0 only, unfiltered.
// Counters are int64: a bin sums num over many steps, and population sizes below 2^31 do not bound that.
//
// PREFIX ONCE.  With one set of edges the prefix part of the literal loop is the same for every chain that carries the prefix:
// it consumes the same point0 cuts at the same prefix rows.  So the prefix is a chain of its own with the cuts
// (those point0, then the prefix's row count): a prefix row's bin depends on cuts inside the prefix only, and prefix rows from
// cut[T] on are after the window in every such chain.  A replicate's own rows are a chain relative to its own block with the cuts
// (point0 zeros, then the loop continued from point0 over its step times).  The whole chain's block is the sum of the two.
#pragma once
#include <stdint.h>
#include "vgx_incidence.h"

// LDS bytes of a counting workgroup: the histogram of P * 7 int64 cells (the budget is VGX_INC_LDS_MAX: P <= 1170)
VGX_HD int64_t vgx_tau_inc_lds_bytes(int64_t P) { return 8 * (int64_t)VGX_INC_CHANNELS * P; }

// a field of a row as a 32-bit index: anything that is not one (never written by the tau kernels) matches nothing
VGX_HD int32_t vgx_tau_inc_idx32(int64_t v) { return (uint64_t)v < 0x80000000ull ? (int32_t)v : -1; }

// One row (num, type, haplotype, population, newHaplotype, newPopulation): the cells it counts in (0, 1 or 2) and its weight.
// Returns the weight num, or 0 when the row counts nowhere.
VGX_HD int64_t vgx_tau_inc_row(int64_t num, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np, int32_t P, int32_t hapNum,
                               const uint32_t *mask, int32_t cell[2], int &n) {
    n = 0;
    if (num <= 0) return 0;
    const int32_t c[5] = {vgx_tau_inc_idx32(type & ~(int64_t)VGX_TL_ROW_DIRECT), vgx_tau_inc_idx32(hap), vgx_tau_inc_idx32(pop),
                          vgx_tau_inc_idx32(nh), vgx_tau_inc_idx32(np)};
    n = vgx_inc_cells(c, P, hapNum, mask, cell);
    return n > 0 ? num : 0;
}

// The parts of the tile [e0, e1) before the window, [e0, b1), and after it, [a0, e1) (either may be empty: b1 <= e0, e1 <= a0)
VGX_HD void vgx_tau_inc_outside(const int32_t *cut, int32_t T, int32_t e0, int32_t e1, int32_t &b1, int32_t &a0) {
    b1 = e1 < cut[0] ? e1 : cut[0];
    a0 = e0 > cut[T] ? e0 : cut[T];
}

// host: the walk of one tile [e0, e1) of a chain (rows = n records of 6 int64) as the workgroup does it: rows outside the window
// add their positive num to outside[0 / 1]; inside, first bin by search, a histogram of P * 7 cells, its nonzero cells added to
// counts[T][P][7] and cleared at every bin change and at the tile's end.  `hist` is P * 7 zeroed cells and is left zeroed.
static inline void vgx_tau_inc_tile_host(const int64_t *rows, const int32_t *cut, int32_t T, int32_t P, int32_t hapNum, const uint32_t *mask,
                                         int32_t e0, int32_t e1, int64_t *hist, int64_t *counts, int64_t *outside) {
    int32_t b1, a0;
    vgx_tau_inc_outside(cut, T, e0, e1, b1, a0);
    for (int32_t e = e0; e < b1; e++) if (rows[(int64_t)e * 6] > 0) outside[0] += rows[(int64_t)e * 6];
    for (int32_t e = a0; e < e1; e++) if (rows[(int64_t)e * 6] > 0) outside[1] += rows[(int64_t)e * 6];
    int32_t pos, hi;
    vgx_inc_clip(cut, T, e0, e1, pos, hi);
    const int32_t cells = P * VGX_INC_CHANNELS;
    while (pos < hi) {
        const int32_t b = vgx_inc_bin(cut, T, pos);
        const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
        for (int32_t e = pos; e < end; e++) {
            const int64_t *v = rows + (int64_t)e * 6;
            int32_t cell[2];
            int n;
            const int64_t w = vgx_tau_inc_row(v[0], v[1], v[2], v[3], v[4], v[5], P, hapNum, mask, cell, n);
            for (int k = 0; k < n; k++) hist[cell[k]] += w;
        }
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { counts[(int64_t)b * cells + i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// launch arguments of the counting kernel (vgx_tau_incidence.hip), filled by vgx_get_tau_incidence
struct VgxTauIncLaunch {
    int64_t m;               // chains of this launch
    const int64_t *rows;     // the prefix rows [n][6], or t_mev: [R][stride][6]
    int64_t stride;          // rows between the blocks of two replicates
    const int64_t *rep;      // [m] replicate of every chain; NULL: one chain at `rows`
    const int32_t *n_rows;   // [m] rows of the chain
    const int32_t *cut;      // [m][T + 1] relative to the chain's first row
    int32_t T, P, hapNum;
    const uint32_t *mask;    // NULL or ceil(hapNum / 32) words
    int32_t tile;            // rows per tile
    int64_t max_n;           // longest chain of the launch
    int64_t *counts;         // [m][T][P][7]
    int64_t *outside;        // [m][2]
};
