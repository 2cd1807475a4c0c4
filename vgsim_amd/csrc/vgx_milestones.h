// vgx_milestones.h — peaks, first passages and last positive events of the cells of a DIRECT event chain, written once for the host
// and the device: the cells a log record changes (vgx_prev_deltas plus the row of all populations), the records a tile keeps, the
// ordered walk of 64 consecutive events with ballots and population counts (one lane settles one cell), the initial block, the merge of a tile and the end
// of a chain.  vgx_milestones.hip runs it one wavefront per (replicate, tile) over the device log (vgx_get_milestones) and,
// compiled for the host with a loop over 64 emulated lanes in place of the wave intrinsics, tile after tile behind
// vgx_test_milestones.  DESIGN.md §21.
//
// Cells: key * V + class with key 0 .. P-1 the populations and key P all populations together, cells = (P + 1) * V.  x[-1] is the
// start, x[i] the value after event i; every step of a cell is +1, 0 or -1.  Per cell
//     final          x[n_ev - 1]
//     peak           max x[i] over [-1, n_ev), peak_event the smallest i that attains it
//     first_event[k] the smallest i >= -1 with x[i] >= theta[k], VGX_MS_NEVER if none
//     last_positive  the largest i in [-1, n_ev) with x[i] > 0, -2 if none
// Every one of them is an extremum over CANDIDATES (value, event) that hold whatever tile they come from: any i with
// x[i] >= theta[k] may be offered to a minimum, any i with x[i] > 0 to a maximum, any (x[i], i) to the peak's ordered maximum.  A
// tile therefore offers what it sees of the cells its events touch, starting from the tile's base (the values at its first event,
// which pass A forms as running sums of tile nets), and the merge takes extrema with integer atomics: no result depends on the
// tile size, the launch geometry, the chunking or the order in which workgroups finish.  What no tile sees is offered elsewhere:
// the start (event -1) by the initial block, and the run of a value up to the end of the chain by vgx_ms_finish (a cell that ends
// positive is positive at event n_ev - 1).  A run of equal values inside the chain begins at a changing event, which its tile
// sees, and the event before a change to zero is offered by the round that holds the change (its lane, or `cur` at e0 - 1).
#pragma once
#include <stdint.h>
#include "../../include/vgx.h"                // VGX_MS_NEVER: first_event of a threshold no value reaches
#include "vgx_prevalence.h"

#define VGX_MS_NONE (-2)                      // last_positive of a cell that is never positive; peak_event of an empty tile record
#define VGX_MS_TILE_DEFAULT 4096              // events of a tile unless VGX_MILESTONES_TILE_EVENTS says otherwise
#define VGX_MS_LDS_MAX (64 * 1024)            // LDS budget of a walking workgroup's records
#define VGX_MS_MAX_K 16                       // thresholds of one call
#define VGX_MS_MAX_EVENTS ((int64_t)1 << 30)
#define VGX_MS_LANES 64                       // events of a round: one per lane of a wavefront

// LDS bytes of the records of a walking workgroup: value, peak, peak event, last positive event and K first events per cell
VGX_HD int64_t vgx_ms_lds_bytes(int64_t P, int64_t V, int64_t K) { return (P + 1) * V * 4 * (4 + K); }

// the peak as one ordered 64-bit key: the value biased to unsigned above, 0xFFFFFFFF - (event + 1) below, so that the largest key
// is the largest value and, among equals, the earliest event (event >= -1)
VGX_HD uint64_t vgx_ms_pack_peak(int32_t value, int32_t event) {
    return ((uint64_t)((uint32_t)value ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(event + 1));
}
VGX_HD int32_t vgx_ms_peak_value(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
VGX_HD int32_t vgx_ms_peak_event(uint64_t key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key) - 1; }

// the lanes 0 .. l of a 64-lane mask
VGX_HD uint64_t vgx_ms_le(int l) { return ((uint64_t)2 << l) - 1; }

VGX_HD int vgx_ms_popc(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(m);
#else
    return __builtin_popcountll(m);
#endif
}
VGX_HD int vgx_ms_ctz(uint64_t m) {      // m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)m) - 1;
#else
    return __builtin_ctzll(m);
#endif
}
VGX_HD int vgx_ms_top(uint64_t m) {      // m != 0: its highest set bit
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)m);
#else
    return 63 - __builtin_clzll(m);
#endif
}

// The records of the cells a tile has touched, one array per field ([cells] each, first [K][cells]): in LDS on the device.
struct VgxMsRecords {
    int32_t *cur;          // the value after the events walked so far (the tile's base before the first)
    int32_t *peak;         // the largest value seen, the tile's base before any is
    int32_t *peak_event;   // its first event, VGX_MS_NONE: nothing above the base seen
    int32_t *last_pos;     // the last event seen with a positive value, VGX_MS_NONE: none
    int32_t *first;        // [K][cells] the first event seen at or above theta[k], VGX_MS_NEVER: none
};
VGX_HD VgxMsRecords vgx_ms_records(int32_t *base, int32_t cells) {
    return VgxMsRecords{base, base + cells, base + 2 * (int64_t)cells, base + 3 * (int64_t)cells, base + 4 * (int64_t)cells};
}
// the record of cell i when a tile begins: the value is the tile's base, nothing seen yet
VGX_HD void vgx_ms_record_init(const VgxMsRecords &rec, int32_t i, int32_t cells, int32_t K, int32_t base) {
    rec.cur[i] = base;
    rec.peak[i] = base;
    rec.peak_event[i] = VGX_MS_NONE;
    rec.last_pos[i] = VGX_MS_NONE;
    for (int32_t k = 0; k < K; k++) rec.first[(int64_t)k * cells + i] = VGX_MS_NEVER;
}

// What lane l's event changes: up to two cells of population rows by vgx_prev_deltas, each also in the row of all populations.
// LANES is 1 on the device (a lane holds its own event in registers) and 64 on the host (slot l is lane l).
template <int LANES>
struct VgxMsEvents {
    int32_t n[LANES];            // 0, 2 or 4 changes
    int32_t cell[4][LANES];
    int32_t sign[4][LANES];
    uint32_t todo[LANES];        // bit k: change k has not been applied yet
};

// c: the record of lane slot `s`, or nullptr for a lane past the tile's end
template <int LANES>
VGX_HD void vgx_ms_load(VgxMsEvents<LANES> &ev, int s, const int32_t *c, int32_t P, int32_t hapNum, int32_t V, const int32_t *variant_of) {
    int32_t cell[2], sign[2];
    const int n = c ? vgx_prev_deltas(c, P, hapNum, V, variant_of, cell, sign) : 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {      // (constant indices: the arrays stay in registers on the device)
        const bool on = k < n;
        ev.cell[2 * k][s] = on ? cell[k] : -1;                  ev.sign[2 * k][s] = on ? sign[k] : 0;
        ev.cell[2 * k + 1][s] = on ? P * V + cell[k] % V : -1;  ev.sign[2 * k + 1][s] = on ? sign[k] : 0;
    }
    ev.n[s] = 2 * n;
    ev.todo[s] = (1u << (2 * n)) - 1;
}

// What one lane settles: one cell of a round from the masks of the lanes that add to it (`pos`) and take from it (`neg`), which
// hold no lane at or past nl.  The value after lane l's event is
//     cur + popcount(pos & le(l)) - popcount(neg & le(l)),
// and all values of the round lie in [cur - popcount(neg), cur + popcount(pos)], which settles most questions at once: a cell
// positive throughout, a peak the range cannot beat, a threshold above the range.  Otherwise a value rises only where a lane adds,
// so the peak and the first passages are looked for at the lanes of `pos` in ascending order, and the last positive event from the
// last change downwards (a value holds from its change up to the next one; before the first it is `cur`, the value at e0 - 1).
// The record's peak starts as the tile's base, which an earlier tile or the initial block has offered: only a larger value is news.
VGX_HD void vgx_ms_settle(int32_t cell, uint64_t pos, uint64_t neg, int32_t e0, int32_t nl, const int32_t *theta, int32_t K, int32_t cells,
                          const VgxMsRecords &rec) {
    const int32_t cur = rec.cur[cell];
    auto value = [&](int l) { return (int32_t)((uint32_t)cur + (uint32_t)vgx_ms_popc(pos & vgx_ms_le(l)) - (uint32_t)vgx_ms_popc(neg & vgx_ms_le(l))); };
    const int64_t hi = (int64_t)cur + vgx_ms_popc(pos), lo = (int64_t)cur - vgx_ms_popc(neg);
    int32_t last = VGX_MS_NONE;
    if (lo > 0) {
        last = e0 + nl - 1;
    } else if (hi > 0) {
        int32_t next = nl;                // the lane of the change after the one looked at (nl: none)
        bool found = false;
        for (uint64_t ch = pos | neg; ch && !found;) {
            const int l = vgx_ms_top(ch);
            ch &= ~((uint64_t)1 << l);
            if (value(l) > 0) found = true;
            else next = l;
        }
        if (found || cur > 0) last = e0 + next - 1;
    }
    if (last > rec.last_pos[cell]) rec.last_pos[cell] = last;
    uint32_t pending = 0;                 // thresholds not met so far that the range reaches
    for (int32_t k = 0; k < K; k++)
        if (hi >= theta[k] && rec.first[(int64_t)k * cells + cell] == VGX_MS_NEVER) pending |= 1u << k;
    int32_t peak = rec.peak[cell];
    if (hi > peak || pending) {
        int32_t peak_event = rec.peak_event[cell];
        for (uint64_t up = pos; up; up &= up - 1) {
            const int l = vgx_ms_ctz(up);
            const int32_t v = value(l);
            if (v > peak) { peak = v; peak_event = e0 + l; }
            for (int32_t k = 0; pending >> k; k++)
                if (((pending >> k) & 1) && v >= theta[k]) {
                    rec.first[(int64_t)k * cells + cell] = e0 + l;
                    pending &= ~(1u << k);
                }
        }
        rec.peak[cell] = peak;
        rec.peak_event[cell] = peak_event;
    }
    rec.cur[cell] = (int32_t)((uint32_t)cur + (uint32_t)vgx_ms_popc(pos) - (uint32_t)vgx_ms_popc(neg));
}

// The distinct cells of a round with their masks, lane j holding the j-th one (LANES as in VgxMsEvents)
template <int LANES>
struct VgxMsCells {
    int32_t cell[LANES];
    uint64_t pos[LANES], neg[LANES];
};

// One round: the events e0 .. e0 + nl - 1 (nl <= 64) of a tile, lane l holding event e0 + l, applied to the records in log order.
// The wave W gives
//     slot(l)            where lane l's data lie in `ev` (0 on the device, l on the host)
//     ballot(f)          the mask of the lanes l with f(l) true
//     at(l, f)           f(l) of one lane, known to all
//     each(f)            f(l) for every lane
//     sync()             the records written are visible to all lanes
// with f(l) evaluated by lane l on the device and in a loop over l = 0 .. 63 on the host.  The loop visits the distinct cells of
// the round (a wave has no match instruction): the lowest lane with a change left names a cell, `pos` / `neg` are the ballots of
// the lanes that add to / take from it (a lane changes a cell at most once), and lane j keeps the j-th cell with its masks.  Then
// every lane settles its own cell from the masks alone (vgx_ms_settle), all cells of the round at once: the cells are distinct,
// so no two lanes touch one record.  A round of more than 64 distinct cells (it can hold 256) settles 64 at a time.
template <class W, int LANES>
VGX_HD void vgx_ms_round(const W &w, VgxMsEvents<LANES> &ev, int32_t e0, int32_t nl, const int32_t *theta, int32_t K, int32_t cells,
                         const VgxMsRecords &rec) {
    VgxMsCells<LANES> mine;
    int count = 0;
    auto settle = [&]() {
        w.each([&](int l) {
            const int s = w.slot(l);
            if (l < count) vgx_ms_settle(mine.cell[s], mine.pos[s], mine.neg[s], e0, nl, theta, K, cells, rec);
        });
        count = 0;
    };
    for (;;) {
        const uint64_t left = w.ballot([&](int l) { return ev.todo[w.slot(l)] != 0; });
        if (!left) break;
        const int lead = vgx_ms_ctz(left);
        const int32_t cell = w.at(lead, [&](int l) {      // (the lead lane's lowest change left; >= 0)
            const int s = w.slot(l);
            const uint32_t low = ev.todo[s] & (0u - ev.todo[s]);
            int32_t c = -1;
#pragma unroll
            for (int k = 0; k < 4; k++) c = low == (1u << k) ? ev.cell[k][s] : c;      // (selects of values: no indexed access)
            return c;
        });
        // the sign of lane l's change to `cell`, 0 without one (unused changes hold cell -1)
        auto sign_of = [&](int l) {
            const int s = w.slot(l);
            int32_t sg = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (ev.cell[k][s] == cell) sg = ev.sign[k][s];
            return sg;
        };
        const uint64_t pos = w.ballot([&](int l) { return sign_of(l) > 0; });
        const uint64_t neg = w.ballot([&](int l) { return sign_of(l) < 0; });
        w.each([&](int l) {
            const int s = w.slot(l);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (ev.cell[k][s] == cell) ev.todo[s] &= ~(1u << k);
            if (l == count) { mine.cell[s] = cell; mine.pos[s] = pos; mine.neg[s] = neg; }
        });
        if (++count == VGX_MS_LANES) settle();
    }
    if (count) settle();
    w.sync();      // (once per round: the cells of one round are distinct)
}

// The result block of one replicate in device memory, one array per field as the records
struct VgxMsBlock {
    uint64_t *peak;        // [cells] vgx_ms_pack_peak
    int32_t *last_pos;     // [cells]
    int32_t *first;        // [K][cells]
};

// the block of a chain before any tile: the start offers itself at event -1.  start [P + 1][V], the row of all populations included
VGX_HD void vgx_ms_init_cell(const VgxMsBlock &b, int32_t cell, int32_t cells, int32_t start, const int32_t *theta, int32_t K) {
    b.peak[cell] = vgx_ms_pack_peak(start, -1);
    b.last_pos[cell] = start > 0 ? -1 : VGX_MS_NONE;
    for (int32_t k = 0; k < K; k++) b.first[(int64_t)k * cells + cell] = start >= theta[k] ? -1 : VGX_MS_NEVER;
}

// the end of a chain of n_ev events for one cell whose final value is `final`: a cell that ends positive is positive at n_ev - 1
VGX_HD int32_t vgx_ms_finish_last(int32_t last_pos, int32_t final, int32_t n_ev) { return final > 0 ? n_ev - 1 : last_pos; }

// host: the merge of a tile's records into the block, as the device does it with atomicMax / atomicMin
static inline void vgx_ms_merge_host(const VgxMsRecords &rec, const VgxMsBlock &b, int32_t cells, int32_t K) {
    for (int32_t i = 0; i < cells; i++) {
        if (rec.peak_event[i] != VGX_MS_NONE) {
            const uint64_t key = vgx_ms_pack_peak(rec.peak[i], rec.peak_event[i]);
            if (key > b.peak[i]) b.peak[i] = key;
        }
        if (rec.last_pos[i] > b.last_pos[i]) b.last_pos[i] = rec.last_pos[i];
        for (int32_t k = 0; k < K; k++)
            if (rec.first[(int64_t)k * cells + i] < b.first[(int64_t)k * cells + i]) b.first[(int64_t)k * cells + i] = rec.first[(int64_t)k * cells + i];
    }
}

// host: the time of an event index: the chain's start for -1, NaN for VGX_MS_NEVER and VGX_MS_NONE
static inline double vgx_ms_time(const double *times, int64_t n_ev, double t_start, int64_t ev) {
    return ev == -1 ? t_start : ev >= 0 && ev < n_ev ? times[ev] : __builtin_nan("");
}

// host: where the results of one replicate go ([P + 1][V] each, first_* [K][P + 1][V]); a null pointer is not written
struct VgxMsOut {
    int32_t *final, *peak, *peak_event, *last_pos, *first;
    double *peak_time, *ext_time, *first_time;
};

// host: the results of one chain from its merged block and the final values of its population rows (fin [P][V], pass A's scan):
// the row of all populations is their sum, a cell that ends positive is positive at n_ev - 1, and every event index gets its time
static inline void vgx_ms_outputs(const VgxMsBlock &b, const int32_t *fin, int32_t P, int32_t V, int32_t K, int64_t n_ev, const double *times,
                                  double t_start, const VgxMsOut &o) {
    const int32_t pv = P * V, cells = pv + V;
    for (int32_t i = 0; i < cells; i++) {
        uint32_t f = 0;
        if (i < pv) f = (uint32_t)fin[i];
        else for (int32_t p = 0; p < P; p++) f += (uint32_t)fin[p * V + (i - pv)];
        const int32_t final = (int32_t)f, last = vgx_ms_finish_last(b.last_pos[i], final, (int32_t)n_ev);
        const int32_t pe = vgx_ms_peak_event(b.peak[i]);
        if (o.final) o.final[i] = final;
        if (o.peak) o.peak[i] = vgx_ms_peak_value(b.peak[i]);
        if (o.peak_event) o.peak_event[i] = pe;
        if (o.last_pos) o.last_pos[i] = last;
        if (o.peak_time) o.peak_time[i] = vgx_ms_time(times, n_ev, t_start, pe);
        if (o.ext_time) o.ext_time[i] = last >= -1 && final == 0 ? vgx_ms_time(times, n_ev, t_start, (int64_t)last + 1) : __builtin_nan("");
        for (int32_t k = 0; k < K; k++) {
            const int32_t fe = b.first[(int64_t)k * cells + i];
            if (o.first) o.first[(int64_t)k * cells + i] = fe;
            if (o.first_time) o.first_time[(int64_t)k * cells + i] = vgx_ms_time(times, n_ev, t_start, fe);
        }
    }
}

// host: a wave of 64 emulated lanes
struct VgxMsHostWave {
    int slot(int l) const { return l; }
    template <class F> uint64_t ballot(F f) const {
        uint64_t m = 0;
        for (int l = 0; l < 64; l++)
            if (f(l)) m |= (uint64_t)1 << l;
        return m;
    }
    template <class F> int32_t at(int l, F f) const { return f(l); }
    template <class F> void each(F f) const { for (int l = 0; l < 64; l++) f(l); }
    void sync() const {}
};

// the base of tile t of row `row`: the start for the first tile, the running sum after tile t - 1 (pass A) for the others
VGX_HD int32_t vgx_ms_base(const int32_t *start, const int32_t *val, int64_t row, int32_t T, int32_t pv, int64_t t, int32_t cell) {
    return t == 0 ? start[row * pv + cell] : val[(row * T + (t - 1)) * pv + cell];
}

// launch arguments of the walk (vgx_milestones.hip), filled by vgx_get_milestones (vgx_api.hip): pass A's launch and what the
// walk adds
struct VgxMsLaunch {
    VgxPrevLaunch a;         // T = tiles of the longest chain, bound[j] = min(j * tile, n_ev), val the running sums after the scan
    int32_t K;
    int32_t theta[VGX_MS_MAX_K];
    uint64_t *peak;          // [m][cells]
    int32_t *last_pos;       // [m][cells]
    int32_t *first;          // [m][K][cells]
};
