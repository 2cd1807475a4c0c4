// vgx_tau_susceptible.h — susceptible hosts per (population, class of immunity groups) of a TAU chain at grid times the caller
// gives: vgx_tau_prevalence.h over the rule of vgx_susceptible.h, written once for the host and the device.
// vgx_tau_susceptible.hip runs it one workgroup per (chain, tile of rows) over the rows where they lie (vgx_get_tau_susceptibles)
// and, compiled for the host, tile after tile behind vgx_test_tau_susceptibles.  DESIGN.md §20.
//
// Rows, bounds, `outside`, the prefix counted once, the int64 cells, the net block (vgx_tau_prev_net), the wrapping sum
// (vgx_tau_prev_add), the running sum (vgx_tau_prev_scan_column) and the launch arguments (VgxTauPrevLaunch with hapNum := susNum,
// V := G, variant_of := class_of) are §19's.  A MIGRATION row's group is its newHaplotype field, as for a direct record: keyed by
// the row's haplotype field (the reference's own replay) the sum does not end in the final state.
#pragma once
#include <stdint.h>
#include "vgx_susceptible.h"
#include "vgx_tau_prevalence.h"

// One row (num, type, haplotype, population, newHaplotype, newPopulation): the cells it changes (n = 0, 1 or 2) with their signs.
// Returns the weight num, or 0 when the row changes nothing.
VGX_HD int64_t vgx_tau_sus_row(int64_t num, int64_t type, int64_t hap, int64_t pop, int64_t nh, int64_t np, int32_t P, int32_t susNum,
                               int32_t G, const int32_t *class_of, int32_t cell[2], int32_t sign[2], int &n) {
    n = 0;
    if (num <= 0) return 0;
    const int32_t c[5] = {vgx_tau_inc_idx32(type & ~(int64_t)VGX_TL_ROW_DIRECT), vgx_tau_inc_idx32(hap), vgx_tau_inc_idx32(pop),
                          vgx_tau_inc_idx32(nh), vgx_tau_inc_idx32(np)};
    n = vgx_sus_deltas(c, P, susNum, G, class_of, cell, sign);
    return n > 0 ? num : 0;
}

// host: the walk of one tile [e0, e1) of a chain (rows = n records of 6 int64) as the workgroup does it (vgx_tau_prev_tile_host
// over this rule)
static inline void vgx_tau_sus_tile_host(const int64_t *rows, const int32_t *bound, int32_t T, int32_t P, int32_t susNum, int32_t G,
                                         const int32_t *class_of, int32_t e0, int32_t e1, int64_t *hist, int64_t *val, int64_t *fin,
                                         int64_t *outside) {
    const int32_t cells = P * G;
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
            const int64_t w = vgx_tau_sus_row(v[0], v[1], v[2], v[3], v[4], v[5], P, susNum, G, class_of, cell, sign, n);
            for (int k = 0; k < n; k++) hist[cell[k]] = vgx_tau_prev_add(hist[cell[k]], sign[k] < 0 ? -w : w);
        }
        int64_t *dst = vgx_tau_prev_net(val, fin, 0, T, cells, j);
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] = vgx_tau_prev_add(dst[i], hist[i]); hist[i] = 0; }
        pos = end;
    }
}
