// vgx_tau_flows.h — who infects whom in a TAU chain: new infections per time bin, source population, destination population and
// variant class, written once for the host and the device: the weighted-row form of vgx_flows.h.  vgx_flows.h supplies the one
// cell a record counts in, the two forms and the cell indices; vgx_tau_incidence.h the rows, the cuts in row index space, the
// `outside` counters and the prefix-once construction.  This file adds only what weights change: int64 cells, so
// 8 bytes per cell in the LDS budget, and `num` in place of 1.  vgx_tau_flows.hip runs it one workgroup per (chain, tile of rows)
// over the rows where they lie (vgx_get_tau_flows) and, compiled for the host, tile after tile behind vgx_test_tau_flows.
// DESIGN.md §24.
//
// A row (num, type, haplotype, population, newHaplotype, newPopulation) counts `num` times in the one cell vgx_flow_cell gives for
// its five fields, each passed through vgx_tau_inc_idx32 and VGX_TL_ROW_DIRECT masked off the type; num <= 0 counts nothing.
// Both forms add the same numbers to the same cells: the block does not depend on the form.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "vgx_flows.h"
#include "vgx_tau_incidence.h"

// LDS bytes of the int64 cells of a counting workgroup in either form
VGX_HD int64_t vgx_tau_flow_lds_bytes(int form, int64_t P, int64_t V) { return form == VGX_FLOW_DENSE ? 8 * P * P * V : 8 * P * V; }

// The form that runs when `asked` is asked for: dense where it fits, else split; 0 when the form asked for, or
// under AUTO the split form, does not fit.
VGX_HD int vgx_tau_flow_form(int asked, int64_t P, int64_t V) {
    if (asked == VGX_FLOW_DENSE || asked == VGX_FLOW_SPLIT) return vgx_tau_flow_lds_bytes(asked, P, V) <= VGX_FLOW_LDS_MAX ? asked : 0;
    if (vgx_tau_flow_lds_bytes(VGX_FLOW_DENSE, P, V) <= VGX_FLOW_LDS_MAX) return VGX_FLOW_DENSE;
    return vgx_tau_flow_lds_bytes(VGX_FLOW_SPLIT, P, V) <= VGX_FLOW_LDS_MAX ? VGX_FLOW_SPLIT : 0;
}

// host: the words of the refusal when vgx_tau_flow_form gives 0, behind the caller's prefix
static inline void vgx_tau_flow_refusal(int asked, int64_t P, int64_t V, char *buf, size_t cap) {
    const int form = asked == VGX_FLOW_DENSE ? VGX_FLOW_DENSE : VGX_FLOW_SPLIT;
    snprintf(buf, cap, "%lld populations x %lld classes need %lld bytes of 8-byte cells in the %s form, above the %lld bytes of LDS a counting workgroup may use",
             (long long)P, (long long)V, (long long)vgx_tau_flow_lds_bytes(form, P, V),
             form == VGX_FLOW_DENSE ? "dense" : "split", (long long)VGX_FLOW_LDS_MAX);
}

// is variant_of (hapNum int32) staged in LDS behind the cells?
VGX_HD bool vgx_tau_flow_stage_map(int form, int64_t P, int64_t V, int64_t hapNum) {
    return vgx_tau_flow_lds_bytes(form, P, V) + 4 * hapNum <= VGX_FLOW_LDS_MAX;
}

// One row: its weight num and the (src, dst, class) it counts at, or 0 when it counts nowhere
VGX_HD int64_t vgx_tau_flow_row(int64_t num, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np, int32_t P, int32_t hapNum,
                                const int32_t *variant_of, int32_t within, int32_t &src, int32_t &dst, int32_t &cls) {
    if (num <= 0) return 0;
    const int32_t c[5] = {vgx_tau_inc_idx32(type & ~(int64_t)VGX_TL_ROW_DIRECT), vgx_tau_inc_idx32(hap), vgx_tau_inc_idx32(pop),
                          vgx_tau_inc_idx32(nh), vgx_tau_inc_idx32(np)};
    return vgx_flow_cell(c, P, hapNum, variant_of, within, src, dst, cls) ? num : 0;
}

// host: the walk of one tile [e0, e1) of a chain (rows = n records of 6 int64) as the workgroup does it in `form`: rows outside the
// window add their positive num to outside[0 / 1]; inside, first bin by search, the cells of `hist` (dense: P * P * V, split:
// P * V; zeroed, left zeroed), the nonzero ones added to counts[T][P][P][V] and cleared at every bin change and at the tile's end;
// in the split form a row off the diagonal goes to counts at once.
static inline void vgx_tau_flow_tile_host(int form, const int64_t *rows, const int32_t *cut, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                          const int32_t *variant_of, int32_t within, int32_t e0, int32_t e1, int64_t *hist, int64_t *counts,
                                          int64_t *outside) {
    int32_t b1, a0;
    vgx_tau_inc_outside(cut, T, e0, e1, b1, a0);
    for (int32_t e = e0; e < b1; e++) if (rows[(int64_t)e * 6] > 0) outside[0] += rows[(int64_t)e * 6];
    for (int32_t e = a0; e < e1; e++) if (rows[(int64_t)e * 6] > 0) outside[1] += rows[(int64_t)e * 6];
    int32_t pos, hi;
    vgx_inc_clip(cut, T, e0, e1, pos, hi);
    const int64_t cells = (int64_t)P * P * V;
    const int32_t kept = form == VGX_FLOW_DENSE ? (int32_t)cells : P * V;
    while (pos < hi) {
        const int32_t b = vgx_inc_bin(cut, T, pos);
        const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
        int64_t *out = counts + (int64_t)b * cells;
        for (int32_t e = pos; e < end; e++) {
            const int64_t *v = rows + (int64_t)e * 6;
            int32_t src, dst, cls;
            const int64_t w = vgx_tau_flow_row(v[0], v[1], v[2], v[3], v[4], v[5], P, hapNum, variant_of, within, src, dst, cls);
            if (!w) continue;
            if (form == VGX_FLOW_DENSE) hist[vgx_flow_index(P, V, src, dst, cls)] += w;
            else if (src == dst) hist[src * V + cls] += w;
            else out[vgx_flow_index(P, V, src, dst, cls)] += w;
        }
        for (int32_t i = 0; i < kept; i++)
            if (hist[i]) { out[form == VGX_FLOW_DENSE ? i : vgx_flow_diag_index(P, V, i)] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// launch arguments of the counting kernel (vgx_tau_flows.hip), filled by vgx_get_tau_flows
struct VgxTauFlowLaunch {
    int64_t m;               // chains of this launch
    const int64_t *rows;     // the prefix rows [n][6], or t_mev: [R][stride][6]
    int64_t stride;          // rows between the blocks of two replicates
    const int64_t *rep;      // [m] replicate of every chain; NULL: one chain at `rows`
    const int32_t *n_rows;   // [m] rows of the chain
    const int32_t *cut;      // [m][T + 1] relative to the chain's first row
    int32_t T, P, hapNum, V;
    const int32_t *variant_of;   // [hapNum]
    int32_t within;          // 0: births are not counted
    int32_t form;            // VGX_FLOW_DENSE or VGX_FLOW_SPLIT
    int32_t tile;            // rows per tile
    int64_t max_n;           // longest chain of the launch
    int64_t *counts;         // [m][T][P][P][V]
    int64_t *outside;        // [m][2]
};
