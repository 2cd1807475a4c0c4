// vgx_susceptible.h — susceptible hosts per (population, class of immunity groups) of a DIRECT event chain at grid times the caller
// gives: the sibling of vgx_prev_deltas for the other half of the state, written once for the host and the device.
// vgx_susceptible.hip runs it one workgroup per (replicate, tile) over the device log (vgx_get_susceptibles) and, compiled for the
// host, tile after tile behind vgx_test_susceptibles.  DESIGN.md §20.
//
// Everything but the cells a record changes is vgx_prevalence.h's: the strict cut rule and the T + 2 bounds (VgxPrevCutter,
// vgx_inc_bin), the layout of the net block (vgx_prev_net), the running sum (vgx_prev_scan_column), the limits and the LDS budget
// (VGX_PREV_LDS_MAX over 4 * P * G bytes), and the launch arguments (VgxPrevLaunch with hapNum := susNum, V := G,
// variant_of := class_of).
#pragma once
#include <stdint.h>
#include "vgx_prevalence.h"

// c = type, haplotype, population, newHaplotype, newPopulation of one log record.  Writes the cells (key * G + class) the record
// changes with their signs and returns how many there are: 0, 1 or 2.  The susceptible side of the 'compartment' semantics of
// vgx_tline.h folded through class_of: the group of the host that leaves or joins the susceptibles is in newHaplotype (a BIRTH
// takes one, a DEATH or SAMPLING returns one, a MIGRATION takes one in newPopulation), a SUSCCHANGE moves one from group
// `haplotype` to group `newHaplotype` of `population`; each side only if tracked, and within one class nothing changes.
VGX_HD int vgx_sus_deltas(const int32_t c[5], int32_t P, int32_t susNum, int32_t G, const int32_t *class_of, int32_t cell[2],
                          int32_t sign[2]) {
    const int32_t t = c[0];
    if (t < VGX_TL_BIRTH || t > VGX_TL_MIGRATION || t == VGX_TL_MUTATION) return 0;
    const int32_t key = t == VGX_TL_MIGRATION ? c[4] : c[2];
    if (key < 0 || key >= P) return 0;
    const int32_t to = vgx_prev_class(class_of, susNum, c[3]);
    int n = 0;
    if (t == VGX_TL_SUSCCHANGE) {
        const int32_t from = vgx_prev_class(class_of, susNum, c[1]);
        if (from == to) return 0;
        if (to >= 0) { cell[n] = key * G + to; sign[n++] = 1; }
        if (from >= 0) { cell[n] = key * G + from; sign[n++] = -1; }
    } else if (to >= 0) {
        cell[n] = key * G + to;
        sign[n++] = t == VGX_TL_DEATH || t == VGX_TL_SAMPLING ? 1 : -1;
    }
    return n;
}

// host: the walk of one tile [e0, e1) of a chain (log = n_ev records of 5 int32) as the workgroup does it (vgx_prev_tile_host
// over this rule): first interval by search, the signed cells of `hist` (P * G, zeroed, left zeroed), the nonzero ones added to
// the interval's net block and cleared at every interval change and at the tile's end.
static inline void vgx_sus_tile_host(const int32_t *log, const int32_t *bound, int32_t T, int32_t P, int32_t susNum, int32_t G,
                                     const int32_t *class_of, int32_t e0, int32_t e1, int32_t *hist, int32_t *val, int32_t *fin) {
    const int32_t cells = P * G;
    int32_t pos = e0;
    while (pos < e1) {
        const int32_t j = vgx_inc_bin(bound, T + 1, pos);
        const int32_t end = e1 < bound[j + 1] ? e1 : bound[j + 1];
        for (int32_t e = pos; e < end; e++) {
            int32_t cell[2], sign[2];
            const int n = vgx_sus_deltas(log + (int64_t)e * 5, P, susNum, G, class_of, cell, sign);
            for (int k = 0; k < n; k++) hist[cell[k]] += sign[k];
        }
        int32_t *dst = vgx_prev_net(val, fin, 0, T, cells, j);
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}
