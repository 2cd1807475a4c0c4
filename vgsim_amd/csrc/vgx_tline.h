// vgx_tline.h — the log replays get_data_infectious / get_data_susceptible (reference src/_BirthDeath.pyx:1967-2045) of a
// DIRECT event chain, written once for the host and the device: which counters an event moves, the rule that turns event
// times into bins, and the query table.  vgx_timelines.hip runs it one workgroup per replicate over the device log
// (vgx_get_timelines) and, compiled for the host, behind vgx_test_timelines.
// vgx_tau_timelines.hip runs the same rule on weighted rows (a tau replicate's chain: the model's events before the call, then
// its multievent rows) behind vgx_get_tau_timelines / vgx_test_tau_timelines.
//
// The replay depends on time for one thing only: at which event the grid index `point` advances (pyx:1978-1981).  `point`
// never decreases, so the whole time dependence of a chain is step_num event indices:
//     cut[p - 1] = first event index whose bin is >= p   (n_ev if none),   p = 1 .. step_num
// and the bin of event e is the number of cuts <= e.  The cuts come from the clock (VgxTlCutter, host only); everything
// after them is integer work.
#pragma once
#include <stdint.h>
#include "vgx_rng.h"

enum { VGX_TL_REFERENCE = 0, VGX_TL_COMPARTMENT = 1 };
enum { VGX_TL_BIRTH = 0, VGX_TL_DEATH = 1, VGX_TL_SAMPLING = 2, VGX_TL_MUTATION = 3, VGX_TL_SUSCCHANGE = 4, VGX_TL_MIGRATION = 5,
       VGX_TL_MULTITYPE = 6 };

// One counter an event moves: a series keyed (population, haplotype) [side 0] or (population, group) [side 1].
struct VgxTlOp {
    int32_t side;      // -1 = none
    int32_t major, minor;
    int32_t delta;
    int32_t sample;    // side 0: the series' Sample counts this event too
};
// Everything one event does: at most two keyed counters, and in the reference semantics the two query-independent rows
// (pyx:1982 reads `A or B or C and D`: a DEATH or SAMPLING of ANY compartment decrements every infectious series, and every
// SAMPLING counts in every Sample).
struct VgxTlMoves {
    VgxTlOp op[2];
    int32_t all_ds, all_s;
};

// c = type, haplotype, population, newHaplotype, newPopulation of one log record
VGX_HD void vgx_tl_classify(int semantics, const int32_t c[5], VgxTlMoves &m) {
    const int32_t t = c[0], hap = c[1], pop = c[2], nh = c[3], np = c[4];
    m.op[0].side = m.op[1].side = -1;
    m.op[0].sample = m.op[1].sample = 0;
    m.all_ds = m.all_s = 0;
    if (t == VGX_TL_BIRTH) {                                  // pyx:1980 / pyx:2017
        m.op[0] = VgxTlOp{0, pop, hap, 1, 0};
        m.op[1] = VgxTlOp{1, pop, nh, -1, 0};
    } else if (t == VGX_TL_DEATH || t == VGX_TL_SAMPLING) {   // pyx:1982 / pyx:2019
        if (semantics == VGX_TL_REFERENCE) {
            m.all_ds = 1;
            m.all_s = t == VGX_TL_SAMPLING;
        } else {
            m.op[0] = VgxTlOp{0, pop, hap, -1, t == VGX_TL_SAMPLING};
        }
        m.op[1] = VgxTlOp{1, pop, nh, 1, 0};
    } else if (t == VGX_TL_MUTATION) {                        // pyx:1982 (its last clause), pyx:1986
        m.op[0] = VgxTlOp{0, pop, hap, -1, 0};
        // the reference's elif chain stops at the first clause that holds: a record with newHaplotype == haplotype only decrements
        if (semantics != VGX_TL_REFERENCE || nh != hap) m.op[1] = VgxTlOp{0, pop, nh, 1, 0};
    } else if (t == VGX_TL_SUSCCHANGE) {                      // pyx:2019, pyx:2021
        m.op[0] = VgxTlOp{1, pop, nh, 1, 0};
        if (nh != hap) m.op[1] = VgxTlOp{1, pop, hap, -1, 0};
    } else if (t == VGX_TL_MIGRATION) {                       // pyx:1988 / pyx:2023
        m.op[0] = VgxTlOp{0, np, hap, 1, 0};
        m.op[1] = VgxTlOp{1, np, nh, -1, 0};
    }
}

// ---- weighted rows (vgx_tau_timelines.hip): the chain of a tau replicate as ONE list of rows (num, type, haplotype, population,
// newHaplotype, newPopulation).  A direct event is a row with num = 1 under the DIRECT rule (vgx_tl_classify as it stands); a
// multievent row moves the same counters num times under the MULTIEVENT rule, the MULTITYPE branch of the reference's replays
// (pyx:1993-2003, 2030-2040), which differs from the direct rule in one place: its susceptible MIGRATION clause tests the row's
// `haplotypes` field against the group (pyx:2037) where the direct one tests `newHaplotypes` (pyx:2023).  The tau kernels write
// the migrant's group into newHaplotypes (as direct MIGRATION events carry it), so the `compartment` semantics key it there under
// both rules.  Returns the weight of the row's moves (0: the row moves nothing).
enum { VGX_TL_RULE_DIRECT = 0, VGX_TL_RULE_MULTIEVENT = 1 };
#define VGX_TL_ROW_DIRECT 0x100   // set in the type field of a flattened row that takes the direct rule
VGX_HD int64_t vgx_tl_classify_row(int semantics, int rule, int64_t num, const int32_t c[5], VgxTlMoves &m) {
    vgx_tl_classify(semantics, c, m);
    if (rule == VGX_TL_RULE_MULTIEVENT && semantics == VGX_TL_REFERENCE && c[0] == VGX_TL_MIGRATION) m.op[1].minor = c[1];
    return num > 0 ? num : 0;
}

// ---- the query table: open addressing over (major, minor'), minor' = haplotype for an infectious query and ~group for a
// susceptible one, so that one table and one probe sequence serve both sides.  tab = [3][tsize]: major, minor', row (-1 = empty).
VGX_HD int32_t vgx_tl_minor(int side, int32_t minor) { return side ? ~minor : minor; }
VGX_HD uint32_t vgx_tl_hash(int32_t major, int32_t minorx) {
    uint32_t h = (uint32_t)major * 0x9E3779B1u ^ (uint32_t)minorx * 0x85EBCA6Bu;
    return h ^ (h >> 15);
}
VGX_HD int vgx_tl_table_size(int queries) {   // power of two, load factor <= 1/2
    int s = 8;
    while (s < 2 * queries) s *= 2;
    return s;
}
// row of the query (side, major, minor), -1 if nobody asked for it (or the record's fields are not indices)
VGX_HD int32_t vgx_tl_find(const int32_t *tab, int tsize, int side, int32_t major, int32_t minor) {
    if (major < 0 || minor < 0) return -1;
    const int32_t mx = vgx_tl_minor(side, minor);
    uint32_t s = vgx_tl_hash(major, mx) & (uint32_t)(tsize - 1);
    for (int k = 0; k < tsize; k++) {
        const int32_t row = tab[2 * tsize + s];
        if (row < 0) return -1;
        if (tab[s] == major && tab[tsize + s] == mx) return row;
        s = (s + 1) & (uint32_t)(tsize - 1);
    }
    return -1;
}
// host: enters a query; false when it is already there
static inline bool vgx_tl_insert(int32_t *tab, int tsize, int side, int32_t major, int32_t minor, int32_t row) {
    const int32_t mx = vgx_tl_minor(side, minor);
    uint32_t s = vgx_tl_hash(major, mx) & (uint32_t)(tsize - 1);
    while (tab[2 * tsize + s] >= 0) {
        if (tab[s] == major && tab[tsize + s] == mx) return false;
        s = (s + 1) & (uint32_t)(tsize - 1);
    }
    tab[s] = major; tab[tsize + s] = mx; tab[2 * tsize + s] = row;
    return true;
}

// ---- bins
// The bin of event e = number of cuts <= e; `hint` is the bin of an earlier event of the same chain (bins never decrease), so
// the usual case is one comparison and the search runs only when a cut was passed.
VGX_HD int vgx_tl_bin(const int32_t *cut, int step, int32_t e, int hint) {
    int b = hint;
    if (b < step && cut[b] <= e) {
        int lo = b + 1, hi = step;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cut[mid] <= e) lo = mid + 1; else hi = mid;
        }
        b = lo;
    }
    return b;
}

// host: time_points as the Python expression `i * currentTime / step_num` forms them (product, then quotient)
static inline void vgx_tl_time_points(double current_time, int64_t step, double *tp) {
    for (int64_t i = 0; i <= step; i++) {
        const double prod = (double)i * current_time;
        tp[i] = prod / (double)step;
    }
}

// host: the cuts of a chain from its event times, by the reference's own loop (pyx:1978-1981; `time_points[point] < t` is strict,
// `point` stops at step_num and never goes back, whatever the times do)
struct VgxTlCutter {
    const double *tp;
    int64_t step;
    int32_t *cut;        // [step]
    int64_t point = 0;
    void event(int64_t i, double t) {
        while (point != step && tp[point] < t) cut[point++] = (int32_t)i;
    }
    int64_t finish(int64_t n_ev) {   // returns last_point
        for (int64_t p = point; p < step; p++) cut[p] = (int32_t)n_ev;
        return point;
    }
};

// Counter rows of one launch: ni infectious queries, ns susceptible ones: Data rows [0, ni), Sample rows [ni, 2 ni),
// susceptible rows [2 ni, 2 ni + ns), each T = step + 1 int32 bins; the table's row of an infectious query is its Data row.
// LDS words of a launch: cuts, table, the two query-independent rows, the counters.
VGX_HD int64_t vgx_tl_lds_bytes(int64_t step, int64_t ni, int64_t ns) {
    const int64_t T = step + 1;
    return 4 * (step + 3 * (int64_t)vgx_tl_table_size((int)(ni + ns)) + 2 * T + (2 * ni + ns) * T);
}
// ... of the weighted-row replay (vgx_tau_timelines.hip): the same rows with int64 counters (a bin sums `num` over many steps), the
// counters first so that they are 8-byte aligned, then the cuts and the table.
VGX_HD int64_t vgx_ttl_lds_bytes(int64_t step, int64_t ni, int64_t ns) {
    const int64_t T = step + 1;
    return 8 * (2 * T + (2 * ni + ns) * T) + 4 * (step + 3 * (int64_t)vgx_tl_table_size((int)(ni + ns)));
}

// host: the cuts of a chain made of a PREFIX of events shared by many chains and the chain's OWN events, as ROW indices of the
// flattened list (prefix rows, then own rows).  The event loop is VgxTlCutter's; the prefix part does not walk the prefix:
// time_points never decrease, so the first prefix event with `time_points[p] < t` is the first one whose RUNNING MAXIMUM of the
// times exceeds time_points[p] — a binary search in pre_max per grid point, equal to the literal loop whatever the times do.
// pre_row[i] = first row of prefix event i (pre_row[n_pre] = prefix rows); own event k starts at row own_row0 + own_m0(k); an
// event without rows still advances `point`, and its cut is the first row after it.  Returns last_point.
template <class OwnTime, class OwnRow>
static inline int64_t vgx_tl_row_cuts(const double *tp, int64_t step, int64_t n_pre, const double *pre_max, const int64_t *pre_row,
                                      int64_t n_own, OwnTime own_time, OwnRow own_m0, int64_t own_row0, int64_t n_rows, int32_t *cut) {
    int64_t point = 0, lo = 0;
    while (point != step && lo < n_pre) {
        int64_t a = lo, b = n_pre;                       // first i in [lo, n_pre) with pre_max[i] > tp[point]
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (tp[point] < pre_max[mid]) b = mid; else a = mid + 1;
        }
        if (a == n_pre) break;
        cut[point++] = (int32_t)pre_row[a];
        lo = a;
    }
    for (int64_t k = 0; k < n_own; k++) {
        const double t = own_time(k);
        while (point != step && tp[point] < t) cut[point++] = (int32_t)(own_row0 + own_m0(k));
    }
    for (int64_t p = point; p < step; p++) cut[p] = (int32_t)n_rows;
    return point;
}

#define VGX_TL_LDS_DEFAULT (64 * 1024)    // a workgroup's LDS budget unless VGX_TIMELINES_LDS_BYTES says otherwise
#define VGX_TL_LDS_MAX (160 * 1024)        // what one workgroup may declare on gfx950
