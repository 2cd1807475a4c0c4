// vgx_prevalence.h — infectious hosts per (population, variant class) of a DIRECT event chain at grid times the caller gives,
// written once for the host and the device: the signed cells a log record changes, the rule that turns event times into
// intervals, the walk of a tile of consecutive events and the running sum.  vgx_prevalence.hip runs it one workgroup per
// (replicate, tile) over the device log (vgx_get_prevalence) and, compiled for the host, tile after tile behind
// vgx_test_prevalence.  DESIGN.md §18.
//
// As in vgx_incidence.h the chain depends on time for one thing only: at which event the interval index advances.  With the grid
// grid[0 .. T-1] the whole time dependence of a chain is T event indices
//     cut[j] = first event index i with grid[j] < t_i   (n_ev if none)
// formed by a literal loop whose `point` never goes back (VgxPrevCutter, host only).  The comparison is strict: it is the
// trajectories' `tg < t_new` (traj_emit), so a grid point gets the state before the event that takes the time past it and an
// event at exactly grid[j] is applied before point j.  Held as T + 2 bounds
//     bound[0] = 0,  bound[j + 1] = cut[j],  bound[T + 1] = n_ev
// interval j = 0 .. T holds the events bound[j] <= i < bound[j + 1] (interval T is the tail after the last grid point), which is
// the bin search of vgx_incidence.h over T + 1 bins that cover the whole chain.  value[j] is the start block plus the net change
// of the intervals 0 .. j, final the same over all T + 1.  Everything after the cuts is integer work.
#pragma once
#include <stdint.h>
#include "vgx_incidence.h"

#define VGX_PREV_TILE_DEFAULT 4096            // events of a tile unless VGX_PREVALENCE_TILE_EVENTS says otherwise
#define VGX_PREV_LDS_MAX (64 * 1024)          // LDS budget of a counting workgroup's cells
#define VGX_PREV_MAX_POINTS ((int64_t)1 << 24)   // T below this
#define VGX_PREV_MAX_EVENTS ((int64_t)1 << 30)

// LDS bytes of the P * V signed int32 cells of a counting workgroup
VGX_HD int64_t vgx_prev_lds_bytes(int64_t P, int64_t V) { return 4 * P * V; }

// is variant_of (hapNum int32) staged in LDS behind the cells?
VGX_HD bool vgx_prev_stage_map(int64_t P, int64_t V, int64_t hapNum) { return 4 * P * V + 4 * hapNum <= VGX_PREV_LDS_MAX; }

// the class of haplotype h: -1 (not tracked) for an h outside [0, hapNum)
VGX_HD int32_t vgx_prev_class(const int32_t *variant_of, int32_t hapNum, int32_t h) {
    return h >= 0 && h < hapNum ? variant_of[h] : -1;
}

// c = type, haplotype, population, newHaplotype, newPopulation of one log record.  Writes the cells (key * V + class) the record
// changes with their signs and returns how many there are: 0, 1 or 2.  The 'compartment' semantics of vgx_tline.h folded through
// variant_of: a MIGRATION adds a host in newPopulation (its source stays), a MUTATION moves one between classes of `population`,
// each side only if tracked, and within one class changes nothing.
VGX_HD int vgx_prev_deltas(const int32_t c[5], int32_t P, int32_t hapNum, int32_t V, const int32_t *variant_of, int32_t cell[2],
                           int32_t sign[2]) {
    const int32_t t = c[0];
    if (t < VGX_TL_BIRTH || t > VGX_TL_MIGRATION || t == VGX_TL_SUSCCHANGE) return 0;
    const int32_t key = t == VGX_TL_MIGRATION ? c[4] : c[2];
    if (key < 0 || key >= P) return 0;
    const int32_t cls = vgx_prev_class(variant_of, hapNum, c[1]);
    int n = 0;
    if (t == VGX_TL_MUTATION) {
        const int32_t to = vgx_prev_class(variant_of, hapNum, c[3]);
        if (cls == to) return 0;
        if (cls >= 0) { cell[n] = key * V + cls; sign[n++] = -1; }
        if (to >= 0) { cell[n] = key * V + to; sign[n++] = 1; }
    } else if (cls >= 0) {
        cell[n] = key * V + cls;
        sign[n++] = t == VGX_TL_BIRTH || t == VGX_TL_MIGRATION ? 1 : -1;
    }
    return n;
}

// host: the bounds of a chain from its event times by the literal loop: `grid[point] < t` is strict, `point` stops at T and never
// goes back, whatever the times do
struct VgxPrevCutter {
    const double *grid;
    int64_t T;
    int32_t *bound;      // [T + 2]
    int64_t point = 0;
    void event(int64_t i, double t) {
        while (point < T && grid[point] < t) bound[++point] = (int32_t)i;
    }
    void finish(int64_t n_ev) {
        bound[0] = 0;
        for (int64_t p = point + 1; p <= T + 1; p++) bound[p] = (int32_t)n_ev;
    }
};

// Where the net change of interval j of row `row` lies: the intervals 0 .. T-1 in val[m][T][cells], which the scan turns into the
// values and the column summary reads as a matrix [m][T * cells]; the tail interval T in fin[m][cells], which becomes `final`.
VGX_HD int32_t *vgx_prev_net(int32_t *val, int32_t *fin, int64_t row, int32_t T, int32_t cells, int32_t j) {
    return j < T ? val + (row * T + j) * cells : fin + row * cells;
}

// host: the walk of one tile [e0, e1) of a chain (log = n_ev records of 5 int32) as the workgroup does it: first interval by
// search, the signed cells of `hist` (P * V, zeroed, left zeroed), the nonzero ones added to the interval's net block and cleared
// at every interval change and at the tile's end.
static inline void vgx_prev_tile_host(const int32_t *log, const int32_t *bound, int32_t T, int32_t P, int32_t hapNum, int32_t V,
                                      const int32_t *variant_of, int32_t e0, int32_t e1, int32_t *hist, int32_t *val, int32_t *fin) {
    const int32_t cells = P * V;
    int32_t pos = e0;
    while (pos < e1) {
        const int32_t j = vgx_inc_bin(bound, T + 1, pos);
        const int32_t end = e1 < bound[j + 1] ? e1 : bound[j + 1];
        for (int32_t e = pos; e < end; e++) {
            int32_t cell[2], sign[2];
            const int n = vgx_prev_deltas(log + (int64_t)e * 5, P, hapNum, V, variant_of, cell, sign);
            for (int k = 0; k < n; k++) hist[cell[k]] += sign[k];
        }
        int32_t *dst = vgx_prev_net(val, fin, 0, T, cells, j);
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { dst[i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// the running sum of one (row, cell) column: val[j] = start + net of the intervals 0 .. j, fin = the same over all T + 1.  The sums
// wrap as unsigned integers do (a log with records outside the model can take a cell below zero; nothing is undefined).
VGX_HD void vgx_prev_scan_column(int32_t *val, int32_t *fin, int32_t start, int32_t T, int64_t stride) {
    uint32_t run = (uint32_t)start;
    for (int32_t j = 0; j < T; j++) {
        run += (uint32_t)val[(int64_t)j * stride];
        val[(int64_t)j * stride] = (int32_t)run;
    }
    *fin = (int32_t)(run + (uint32_t)*fin);
}

// launch arguments of the counting and scan kernels (vgx_prevalence.hip), filled by vgx_get_prevalence (vgx_api.hip)
struct VgxPrevLaunch {
    int64_t m;               // replicates of this launch
    const int32_t *log;      // r_evcols: [R][evcap][6]
    int64_t evcap;
    const int64_t *rep;      // [m] replicate of every row
    const int32_t *n_ev;     // [m] events of its chain
    const int32_t *bound;    // [m][T + 2]
    int32_t T, P, hapNum, V;
    const int32_t *variant_of;   // [hapNum]
    int32_t tile;            // events per tile
    int64_t max_n;           // longest chain of the launch
    int32_t *val;            // [m][T][P][V] net changes, zeroed by the caller; values after the scan
    int32_t *fin;            // [m][P][V] net change of the tail; final after the scan
    const int32_t *start;    // [m][P][V] (scan only)
};
