// vgx_incidence.h — incidence of a DIRECT event chain on a grid of time bins the caller gives, written once for the host and
// the device: which (channel, population) cells a log record counts in, the rule that turns event times into bins, and the
// walk of a tile of consecutive events.  vgx_incidence.hip runs it one workgroup per (replicate, tile) over the device log
// (vgx_get_incidence) and, compiled for the host, tile after tile behind vgx_test_incidence.
//
// As in vgx_tline.h the chain depends on time for one thing only: at which event the bin index advances.  With the edges
// edges[0 .. T] the whole time dependence of a chain is T + 1 event indices:
//     cut[k] = first event index i with edges[k] <= t_i   (n_ev if none),   k = 0 .. T
// formed by a literal loop whose `point` never goes back (VgxIncCutter, host only).  Event i lies in bin b when
// cut[b] <= i < cut[b + 1]; events before cut[0] or from cut[T] on are outside the window.  Everything after the cuts is
// integer work: a bin is a contiguous range of event indices.
#pragma once
#include <stdint.h>
#include "vgx_rng.h"
#include "vgx_tline.h"

#define VGX_INC_CHANNELS 7
enum { VGX_INC_BIRTH = 0, VGX_INC_DEATH = 1, VGX_INC_SAMPLING = 2, VGX_INC_MUTATION = 3, VGX_INC_SUSCCHANGE = 4, VGX_INC_ARRIVAL = 5,
       VGX_INC_DEPARTURE = 6 };

#define VGX_INC_TILE_DEFAULT 4096            // events of a tile unless VGX_INCIDENCE_TILE_EVENTS says otherwise
#define VGX_INC_LDS_MAX (64 * 1024)          // LDS budget of a counting workgroup
#define VGX_INC_MAX_BINS ((int64_t)1 << 24)  // T below this
#define VGX_INC_MAX_EVENTS ((int64_t)1 << 30)

// LDS bytes of a counting workgroup: the histogram of P * 7 int32 cells is all it keeps there (cuts are read where they lie)
VGX_HD int64_t vgx_inc_lds_bytes(int64_t P) { return 4 * (int64_t)VGX_INC_CHANNELS * P; }

// is haplotype h in the filter?  mask = NULL: no filter.  An h outside [0, hapNum) is in no filter.
VGX_HD bool vgx_inc_in_mask(const uint32_t *mask, int32_t hapNum, int32_t h) {
    return h >= 0 && h < hapNum && ((mask[h >> 5] >> (h & 31)) & 1u) != 0;
}

// c = type, haplotype, population, newHaplotype, newPopulation of one log record.  Writes the histogram cells
// (key * 7 + channel) the record counts in and returns how many there are: 0, 1 or 2 (a MIGRATION counts as an arrival in
// newPopulation and as a departure in population, each only if that key is a population).
VGX_HD int vgx_inc_cells(const int32_t c[5], int32_t P, int32_t hapNum, const uint32_t *mask, int32_t cell[2]) {
    const int32_t t = c[0];
    if (t < VGX_TL_BIRTH || t > VGX_TL_MIGRATION) return 0;
    if (mask) {   // the judged haplotype: the variant that arises for a MUTATION; a SUSCCHANGE carries none
        if (t == VGX_TL_SUSCCHANGE) return 0;
        if (!vgx_inc_in_mask(mask, hapNum, t == VGX_TL_MUTATION ? c[3] : c[1])) return 0;
    }
    int n = 0;
    if (t == VGX_TL_MIGRATION) {
        if (c[4] >= 0 && c[4] < P) cell[n++] = c[4] * VGX_INC_CHANNELS + VGX_INC_ARRIVAL;
        if (c[2] >= 0 && c[2] < P) cell[n++] = c[2] * VGX_INC_CHANNELS + VGX_INC_DEPARTURE;
    } else if (c[2] >= 0 && c[2] < P) {
        cell[n++] = c[2] * VGX_INC_CHANNELS + t;   // channels 0 .. 4 are the types 0 .. 4
    }
    return n;
}

// The bin of event e: (number of cuts <= e) - 1, by a search in the non-decreasing cut[0 .. T].  -1: before the window, T: after.
VGX_HD int32_t vgx_inc_bin(const int32_t *cut, int32_t T, int32_t e) {
    int32_t lo = 0, hi = T + 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cut[mid] <= e) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The part of the tile [e0, e1) inside the window: [lo, hi), empty when hi <= lo.
VGX_HD void vgx_inc_clip(const int32_t *cut, int32_t T, int32_t e0, int32_t e1, int32_t &lo, int32_t &hi) {
    lo = e0 > cut[0] ? e0 : cut[0];
    hi = e1 < cut[T] ? e1 : cut[T];
}

// host: the cuts of a chain from its event times by the literal loop: `edges[point] <= t` is inclusive, `point` stops at T + 1
// and never goes back, whatever the times do
struct VgxIncCutter {
    const double *edges;
    int64_t T;
    int32_t *cut;        // [T + 1]
    int64_t point = 0;
    void event(int64_t i, double t) {
        while (point <= T && edges[point] <= t) cut[point++] = (int32_t)i;
    }
    void finish(int64_t n_ev) {
        for (int64_t p = point; p <= T; p++) cut[p] = (int32_t)n_ev;
    }
};

// host: the walk of one tile [e0, e1) of a chain (log = n_ev records of 5 int32) as the workgroup does it: first bin by search,
// a histogram of P * 7 cells, its nonzero cells added to counts[T][P][7] and cleared at every bin change and at the tile's end.
// `hist` is P * 7 zeroed cells and is left zeroed.
static inline void vgx_inc_tile_host(const int32_t *log, const int32_t *cut, int32_t T, int32_t P, int32_t hapNum, const uint32_t *mask,
                                     int32_t e0, int32_t e1, int32_t *hist, int32_t *counts) {
    int32_t pos, hi;
    vgx_inc_clip(cut, T, e0, e1, pos, hi);
    const int32_t cells = P * VGX_INC_CHANNELS;
    while (pos < hi) {
        const int32_t b = vgx_inc_bin(cut, T, pos);
        const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
        for (int32_t e = pos; e < end; e++) {
            int32_t cell[2];
            const int n = vgx_inc_cells(log + (int64_t)e * 5, P, hapNum, mask, cell);
            for (int k = 0; k < n; k++) hist[cell[k]] += 1;
        }
        for (int32_t i = 0; i < cells; i++)
            if (hist[i]) { counts[(int64_t)b * cells + i] += hist[i]; hist[i] = 0; }
        pos = end;
    }
}

// launch arguments of the counting kernel (vgx_incidence.hip), filled by vgx_get_incidence (vgx_api.hip)
struct VgxIncLaunch {
    int64_t m;               // replicates of this launch
    const int32_t *log;      // r_evcols: [R][evcap][6]
    int64_t evcap;
    const int64_t *rep;      // [m] replicate of every row
    const int32_t *n_ev;     // [m] events of its chain
    const int32_t *cut;      // [m][T + 1]
    int32_t T, P, hapNum;
    const uint32_t *mask;    // NULL or ceil(hapNum / 32) words
    int32_t tile;            // events per tile
    int64_t max_n;           // longest chain of the launch
    int32_t *counts;         // [m][T][P][7], zeroed by the caller
};
