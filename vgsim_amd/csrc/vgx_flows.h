// vgx_flows.h — who infects whom: new infections of a DIRECT event chain per time bin, source population, destination population
// and variant class, written once for the host and the device: the one cell a log record counts in, the two forms of the table a
// counting workgroup keeps, and the walk of a tile of consecutive events.  vgx_flows.hip runs it one workgroup per
// (replicate, tile) over the device log (vgx_get_flows) and, compiled for the host, tile after tile behind vgx_test_flows.
// DESIGN.md §23.
//
// Every new infection in this log names its source: a BIRTH in p is a transmission within p, a MIGRATION
// (population -> newPopulation) one across.  The bins are vgx_incidence.h's, unchanged (edges[0 .. T], VgxIncCutter, vgx_inc_bin,
// vgx_inc_clip), the class lookup is vgx_prevalence.h's vgx_prev_class.  The margins of the block are vgx_incidence.h's channels:
// the sum over src is 0 + 5, the off-diagonal sum over dst is 6, the diagonal is 0 (when no MIGRATION has equal keys).
//
// The table of a bin, P * P * V int32 cells in (src, dst, class) order, does not always fit the LDS of a counting workgroup, and
// it is unevenly hit: births touch the diagonal only, migrations are few and scattered.  Two forms of the same walk:
//   dense   all P * P * V cells in LDS, the nonzero ones added to the bin's block at every bin change and at the tile's end;
//   split   the P * V diagonal cells in LDS, flushed the same way; a record off the diagonal adds 1 to its cell of the bin's
//           block in device memory at once.
// Both add the same ones to the same cells: the block does not depend on the form.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "vgx_incidence.h"
#include "vgx_prevalence.h"

#define VGX_FLOW_TILE_DEFAULT 4096            // events of a tile unless VGX_FLOWS_TILE_EVENTS says otherwise
#define VGX_FLOW_LDS_MAX (64 * 1024)          // LDS budget of a counting workgroup's cells
#define VGX_FLOW_MAX_BINS VGX_INC_MAX_BINS
#define VGX_FLOW_MAX_EVENTS VGX_INC_MAX_EVENTS
enum { VGX_FLOW_AUTO = 0, VGX_FLOW_DENSE = 1, VGX_FLOW_SPLIT = 2 };   // `form` asked for; the form that ran is DENSE or SPLIT

// LDS bytes of the cells of a counting workgroup in either form
VGX_HD int64_t vgx_flow_lds_bytes(int form, int64_t P, int64_t V) { return form == VGX_FLOW_DENSE ? 4 * P * P * V : 4 * P * V; }

// The form that runs when `asked` is asked for: dense where it fits, else split (DESIGN.md §23 for why not the other way round);
// 0 when the form asked for, or under AUTO the split form, does not fit.
VGX_HD int vgx_flow_form(int asked, int64_t P, int64_t V) {
    if (asked == VGX_FLOW_DENSE || asked == VGX_FLOW_SPLIT) return vgx_flow_lds_bytes(asked, P, V) <= VGX_FLOW_LDS_MAX ? asked : 0;
    if (vgx_flow_lds_bytes(VGX_FLOW_DENSE, P, V) <= VGX_FLOW_LDS_MAX) return VGX_FLOW_DENSE;
    return vgx_flow_lds_bytes(VGX_FLOW_SPLIT, P, V) <= VGX_FLOW_LDS_MAX ? VGX_FLOW_SPLIT : 0;
}

// host: the words of the refusal when vgx_flow_form gives 0, behind the caller's prefix
static inline void vgx_flow_refusal(int asked, int64_t P, int64_t V, char *buf, size_t cap) {
    const int form = asked == VGX_FLOW_DENSE ? VGX_FLOW_DENSE : VGX_FLOW_SPLIT;
    snprintf(buf, cap, "%lld populations x %lld classes need %lld bytes of cells in the %s form, above the %lld bytes of LDS a counting workgroup may use",
             (long long)P, (long long)V, (long long)vgx_flow_lds_bytes(form, P, V),
             form == VGX_FLOW_DENSE ? "dense" : "split", (long long)VGX_FLOW_LDS_MAX);
}

// is variant_of (hapNum int32) staged in LDS behind the cells?  (vgx_prev_stage_map with this table's bytes)
VGX_HD bool vgx_flow_stage_map(int form, int64_t P, int64_t V, int64_t hapNum) {
    return vgx_flow_lds_bytes(form, P, V) + 4 * hapNum <= VGX_FLOW_LDS_MAX;
}

// c = type, haplotype, population, newHaplotype, newPopulation of one log record; `within` = 0 leaves the births out.  Does the
// record count, and if so at which (src, dst, class)?  A BIRTH counts at (population, population), a MIGRATION at
// (population, newPopulation) literally (equal keys land on the diagonal); every other type, a type outside 0 .. 5, a key outside
// [0, P), a haplotype outside [0, hapNum) and a haplotype that is not tracked count nowhere.
VGX_HD bool vgx_flow_cell(const int32_t c[5], int32_t P, int32_t hapNum, const int32_t *variant_of, int32_t within, int32_t &src,
                          int32_t &dst, int32_t &cls) {
    const int32_t t = c[0];
    if (t == VGX_TL_BIRTH) {
        if (!within) return false;
        dst = c[2];
    } else if (t == VGX_TL_MIGRATION) {
        dst = c[4];
    } else {
        return false;
    }
    src = c[2];
    if (src < 0 || src >= P || dst < 0 || dst >= P) return false;
    cls = vgx_prev_class(variant_of, hapNum, c[1]);
    return cls >= 0;
}

// the cell of (src, dst, class) in a bin's table of P * P * V
VGX_HD int32_t vgx_flow_index(int32_t P, int32_t V, int32_t src, int32_t dst, int32_t cls) { return (src * P + dst) * V + cls; }

// split form: the cell of a bin's table that diagonal cell i = p * V + class stands for
VGX_HD int32_t vgx_flow_diag_index(int32_t P, int32_t V, int32_t i) { return (i / V) * (P + 1) * V + i % V; }

// host: the walk of one tile [e0, e1) of a chain (log = n_ev records of 5 int32) as the workgroup does it in `form`: first bin by
// search, the cells of `hist` (dense: P * P * V, split: P * V; zeroed, left zeroed), the nonzero ones added to counts[T][P][P][V]
// and cleared at every bin change and at the tile's end; in the split form a record off the diagonal goes to counts at once.
static inline void vgx_flow_tile_host(int form, const int32_t *log, const int32_t *cut, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                      const int32_t *variant_of, int32_t within, int32_t e0, int32_t e1, int32_t *hist, int32_t *counts) {
    int32_t pos, hi;
    vgx_inc_clip(cut, T, e0, e1, pos, hi);
    const int64_t cells = (int64_t)P * P * V;
    const int32_t kept = form == VGX_FLOW_DENSE ? (int32_t)cells : P * V;
    while (pos < hi) {
        const int32_t b = vgx_inc_bin(cut, T, pos);
        const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
        int32_t *out = counts + (int64_t)b * cells;
        for (int32_t e = pos; e < end; e++) {
            int32_t src, dst, cls;
            if (!vgx_flow_cell(log + (int64_t)e * 5, P, hapNum, variant_of, within, src, dst, cls)) continue;
            if (form == VGX_FLOW_DENSE) hist[vgx_flow_index(P, V, src, dst, cls)] += 1;
            else if (src == dst) hist[src * V + cls] += 1;
            else out[vgx_flow_index(P, V, src, dst, cls)] += 1;
        }
        for (int32_t i = 0; i < kept; i++)
            if (hist[i]) { out[form == VGX_FLOW_DENSE ? i : vgx_flow_diag_index(P, V, i)] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// launch arguments of the counting kernel (vgx_flows.hip), filled by vgx_get_flows (vgx_api.hip)
struct VgxFlowLaunch {
    int64_t m;               // replicates of this launch
    const int32_t *log;      // r_evcols: [R][evcap][6]
    int64_t evcap;
    const int64_t *rep;      // [m] replicate of every row
    const int32_t *n_ev;     // [m] events of its chain
    const int32_t *cut;      // [m][T + 1]
    int32_t T, P, hapNum, V;
    const int32_t *variant_of;   // [hapNum]
    int32_t within;          // 0: births are not counted
    int32_t form;            // VGX_FLOW_DENSE or VGX_FLOW_SPLIT
    int32_t tile;            // events per tile
    int64_t max_n;           // longest chain of the launch
    int32_t *counts;         // [m][T][P][P][V], zeroed by the caller
};
