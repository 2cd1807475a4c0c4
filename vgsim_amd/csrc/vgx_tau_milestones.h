// vgx_tau_milestones.h — peaks, first passages and last positive events of the cells of a TAU event chain, written once for the host
// and the device: the records a tile keeps, the settle of one cell at one event, the initial block, the merge of a tile, the end of
// a chain and the outputs.  vgx_tau_milestones.hip runs it one workgroup per (chain, tile of whole events) over the rows where they
// lie (vgx_get_tau_milestones) and, compiled for the host, tile after tile behind vgx_test_tau_milestones.  DESIGN.md §22.
//
// CHAIN.  The chain of vgx_tau_prevalence.h: weighted rows of six int64, the prefix flattened (vgx_tau_rows.h), then the replicate's
// own rows.  An EVENT is a direct event of the prefix or one step; events are numbered from 0 along the chain.
// CELLS.  key * V + class with key 0 .. P-1 the populations and key P all populations together, cells = (P + 1) * V.  A row changes
// the population cells as vgx_tau_prev_row says (sign * num), and every change to (p, c) is also made to (P, c).
// VALUES.  x[-1] is the start, x[i] the value after ALL rows of event i: the state inside a step is not a value.  int64, compared
// signed, summed wrapping as unsigned 64-bit integers do (vgx_tau_prev_add).  Per cell
//     final          x[n_ev - 1]
//     peak           max x[i] over [-1, n_ev), peak_event the smallest i that attains it
//     first_event[k] the smallest i >= -1 with x[i] >= theta[k] (int64), VGX_MS_NEVER if none
//     last_positive  the largest i in [-1, n_ev) with x[i] > 0, -2 if none
// Every one of them is an extremum over CANDIDATES that hold whatever tile offers them: any i with x[i] >= theta[k] to a minimum,
// any (x[i], i) to the peak's ordered maximum, any i with x[i] > 0 to a maximum; an event that takes a cell from above zero to zero
// or below offers i - 1.  A cell's value changes only at events that touch it, so a tile settles the touched (event, cell) pairs
// alone (vgx_tau_ms_settle), starting from the tile's base (the values at its first event, pass A's running sums); events without
// rows are not visited.  What no tile sees is offered elsewhere: the start by the initial block, the run of a value up to the end
// of the chain by vgx_tau_ms_finish_last.  The PREFIX is walked once as a chain of its own from the initial state; its block and
// its final values are what every replicate that carries it starts from, which is legitimate because extrema of candidates do not
// care who offered them.
#pragma once
#include <stdint.h>
#include "../../include/vgx.h"
#include "vgx_milestones.h"        // VGX_MS_NONE, VGX_MS_MAX_K, VGX_MS_MAX_EVENTS, VGX_MS_LDS_MAX
#include "vgx_tau_prevalence.h"    // vgx_tau_prev_row, vgx_tau_prev_add, VgxTauPrevLaunch

#define VGX_TAU_MS_TILE_DEFAULT 4096     // rows of a tile unless VGX_TAU_MILESTONES_TILE_ROWS says otherwise

// LDS bytes of a walking workgroup: per cell the value, the event's net change and the peak (int64), the peak's event, the last
// positive event, K first events, an entry of the touched list and its mark (int32); two list lengths behind them
VGX_HD int64_t vgx_tau_ms_lds_bytes(int64_t P, int64_t V, int64_t K) { return (P + 1) * V * (40 + 4 * K) + 16; }

// The records of a tile, one array per field ([cells] each, first [K][cells]): in LDS on the device.  list[0 .. pv) holds the
// population cells the running event has touched, list[pv .. cells) the cells of row P; count[0 / 1] their numbers.
struct VgxTauMsRecords {
    int64_t *cur;          // the value after the events walked so far (the tile's base before the first)
    int64_t *delta;        // the net change of the running event, zero between events
    int64_t *peak;         // the largest value seen, the tile's base before any is
    int32_t *peak_event;   // its first event, VGX_MS_NONE: nothing above the base seen
    int32_t *last_pos;     // the last event seen with a positive value, VGX_MS_NONE: none
    int32_t *first;        // [K][cells] the first event seen at or above theta[k], VGX_MS_NEVER: none
    int32_t *list;         // [cells]
    int32_t *mark;         // [cells] 1: the cell is on the list
    int32_t *count;        // [2]
};
// base: 8-byte aligned, vgx_tau_ms_lds_bytes long
VGX_HD VgxTauMsRecords vgx_tau_ms_records(void *base, int32_t cells, int32_t K) {
    int64_t *q = (int64_t *)base;
    int32_t *d = (int32_t *)(q + 3 * (int64_t)cells);
    return VgxTauMsRecords{q, q + cells, q + 2 * (int64_t)cells, d, d + cells, d + 2 * (int64_t)cells, d + (2 + (int64_t)K) * cells,
                           d + (3 + (int64_t)K) * cells, d + (4 + (int64_t)K) * cells};
}
// the record of cell i when a tile begins: the value is the tile's base, nothing seen, nothing touched
VGX_HD void vgx_tau_ms_record_init(const VgxTauMsRecords &rec, int32_t i, int32_t cells, int32_t K, int64_t base) {
    rec.cur[i] = base;
    rec.delta[i] = 0;
    rec.peak[i] = base;
    rec.peak_event[i] = VGX_MS_NONE;
    rec.last_pos[i] = VGX_MS_NONE;
    rec.mark[i] = 0;
    for (int32_t k = 0; k < K; k++) rec.first[(int64_t)k * cells + i] = VGX_MS_NEVER;
}

// The settle of one cell at event `ev`, whose rows change it by `delta` in all: the new value and what it offers.  The events of
// a tile are settled in ascending order, so the first event at a threshold is kept and the last positive event overwritten.  A
// net change of zero offers nothing: the value was offered when it arose.  The record's peak starts as the tile's base, which an
// earlier tile or the initial block has offered: only a larger value is news.
VGX_HD void vgx_tau_ms_settle(const VgxTauMsRecords &rec, int32_t cell, int32_t cells, int64_t delta, int32_t ev, const int64_t *theta, int32_t K) {
    if (delta == 0) return;
    const int64_t v0 = rec.cur[cell], v1 = vgx_tau_prev_add(v0, delta);
    rec.cur[cell] = v1;
    if (v1 > rec.peak[cell]) { rec.peak[cell] = v1; rec.peak_event[cell] = ev; }
    for (int32_t k = 0; k < K; k++)
        if (v1 >= theta[k] && rec.first[(int64_t)k * cells + cell] == VGX_MS_NEVER) rec.first[(int64_t)k * cells + cell] = ev;
    if (v1 > 0) rec.last_pos[cell] = ev;
    else if (v0 > 0) rec.last_pos[cell] = ev - 1;      // (positive up to the event before this one)
}

// The result block of one chain, one array per field
struct VgxTauMsBlock {
    int64_t *peak;         // [cells]
    int32_t *peak_event;   // [cells]
    int32_t *last_pos;     // [cells]
    int32_t *first;        // [K][cells]
};

// the block of a chain before any tile: the start offers itself at event -1.  start: the cell's x[-1]
VGX_HD void vgx_tau_ms_init_cell(const VgxTauMsBlock &b, int32_t cell, int32_t cells, int64_t start, const int64_t *theta, int32_t K) {
    b.peak[cell] = start;
    b.peak_event[cell] = -1;
    b.last_pos[cell] = start > 0 ? -1 : VGX_MS_NONE;
    for (int32_t k = 0; k < K; k++) b.first[(int64_t)k * cells + cell] = start >= theta[k] ? -1 : VGX_MS_NEVER;
}

// the peak of a tile (value, event; VGX_MS_NONE: none) offered to the block's: tiles are offered in chain order and only a
// strictly greater value wins, so among equals the earliest event stays
VGX_HD void vgx_tau_ms_offer_peak(int64_t &peak, int32_t &peak_event, int64_t value, int32_t event) {
    if (event != VGX_MS_NONE && value > peak) { peak = value; peak_event = event; }
}

// the end of a chain of n_ev events for one cell whose final value is `final`: a cell that ends positive is positive at n_ev - 1
VGX_HD int32_t vgx_tau_ms_finish_last(int32_t last_pos, int64_t final, int32_t n_ev) { return final > 0 ? n_ev - 1 : last_pos; }

// the base of tile t of chain `row` for a population cell: the chain's start for the first tile, the running sum after tile t - 1
// (pass A) for the others
VGX_HD int64_t vgx_tau_ms_base(const int64_t *start, const int64_t *val, int64_t row, int32_t T, int32_t pv, int64_t t, int32_t cell) {
    return t == 0 ? start[row * pv + cell] : val[(row * T + (t - 1)) * pv + cell];
}

// host: one event of a tile as the workgroup does it: (i) every row's signed num into the net change of its cells, a cell noted
// the first time it is hit; (ii) every touched population cell settled, its net change passed on to row P and cleared; then the
// touched cells of row P settled.  rows: the event's rows [n][6].
static inline void vgx_tau_ms_event_host(const VgxTauMsRecords &rec, const int64_t *rows, int64_t n, int32_t ev, int32_t P, int32_t hapNum, int32_t V,
                                         const int32_t *variant_of, const int64_t *theta, int32_t K) {
    const int32_t pv = P * V, cells = pv + V;
    auto note = [&](int32_t cell, int64_t w, int32_t at, int which) {
        rec.delta[cell] = vgx_tau_prev_add(rec.delta[cell], w);
        if (!rec.mark[cell]) { rec.mark[cell] = 1; rec.list[at + rec.count[which]++] = cell; }
    };
    for (int64_t r = 0; r < n; r++) {
        const int64_t *v = rows + r * 6;
        int32_t cell[2], sign[2];
        int k;
        const int64_t w = vgx_tau_prev_row(v[0], v[1], v[2], v[3], v[4], v[5], P, hapNum, V, variant_of, cell, sign, k);
        for (int j = 0; j < k; j++) note(cell[j], sign[j] < 0 ? -w : w, 0, 0);
    }
    for (int32_t i = 0; i < rec.count[0]; i++) {
        const int32_t cell = rec.list[i];
        const int64_t d = rec.delta[cell];
        rec.delta[cell] = 0;
        rec.mark[cell] = 0;
        if (!d) continue;
        vgx_tau_ms_settle(rec, cell, cells, d, ev, theta, K);
        note(pv + cell % V, d, pv, 1);
    }
    for (int32_t i = 0; i < rec.count[1]; i++) {
        const int32_t cell = rec.list[pv + i];
        const int64_t d = rec.delta[cell];
        rec.delta[cell] = 0;
        rec.mark[cell] = 0;
        vgx_tau_ms_settle(rec, cell, cells, d, ev, theta, K);
    }
    rec.count[0] = rec.count[1] = 0;
}

// host: the merge of a tile's records into the block, tiles in chain order (the device: 32-bit atomic extrema, and the peaks
// through a slot per tile that a small kernel reduces in tile order)
static inline void vgx_tau_ms_merge_host(const VgxTauMsRecords &rec, const VgxTauMsBlock &b, int32_t cells, int32_t K) {
    for (int32_t i = 0; i < cells; i++) {
        vgx_tau_ms_offer_peak(b.peak[i], b.peak_event[i], rec.peak[i], rec.peak_event[i]);
        if (rec.last_pos[i] > b.last_pos[i]) b.last_pos[i] = rec.last_pos[i];
        for (int32_t k = 0; k < K; k++)
            if (rec.first[(int64_t)k * cells + i] < b.first[(int64_t)k * cells + i]) b.first[(int64_t)k * cells + i] = rec.first[(int64_t)k * cells + i];
    }
}

// host: the tiles of a chain of n_ev events whose first rows are ev_row[0 .. n_ev]: runs of whole events of about `tile` rows (a
// tile closes before the event that would take it past `tile` rows, and after `tile` events; a step with more rows is a tile of
// its own).  Appends the first event of every tile and, last, n_ev: tiles + 1 entries, one entry (0) for a chain without events.
template <class Row, class Vec>
static inline void vgx_tau_ms_tiles(Row ev_row, int64_t n_ev, int64_t tile, Vec &edges) {
    edges.push_back(0);
    int64_t first = 0;
    for (int64_t e = 1; e < n_ev; e++)
        if (e - first >= tile || (int64_t)ev_row(e + 1) - (int64_t)ev_row(first) > tile) {
            edges.push_back((int32_t)e);
            first = e;
        }
    if (n_ev > 0) edges.push_back((int32_t)n_ev);
}

// host: where the results of one chain go ([P + 1][V] each, first_* [K][P + 1][V]); a null pointer is not written
struct VgxTauMsOut {
    int64_t *final, *peak;
    int32_t *peak_event, *last_pos, *first;
    double *peak_time, *ext_time, *first_time;
};

// host: the results of one chain from its merged block and the final values of its population rows (fin [P][V], pass A's scan):
// the row of all populations is their sum, a cell that ends positive is positive at n_ev - 1, and every event index gets its time
// (time_of(i) for 0 <= i < n_ev, t_start for -1, NaN for VGX_MS_NEVER and VGX_MS_NONE)
template <class TimeOf>
static inline void vgx_tau_ms_outputs(const VgxTauMsBlock &b, const int64_t *fin, int32_t P, int32_t V, int32_t K, int64_t n_ev, TimeOf time_of,
                                      double t_start, const VgxTauMsOut &o) {
    const int32_t pv = P * V, cells = pv + V;
    auto when = [&](int64_t ev) { return ev == -1 ? t_start : ev >= 0 && ev < n_ev ? (double)time_of(ev) : __builtin_nan(""); };
    for (int32_t i = 0; i < cells; i++) {
        int64_t final = 0;
        if (i < pv) final = fin[i];
        else for (int32_t p = 0; p < P; p++) final = vgx_tau_prev_add(final, fin[p * V + (i - pv)]);
        const int32_t last = vgx_tau_ms_finish_last(b.last_pos[i], final, (int32_t)n_ev), pe = b.peak_event[i];
        if (o.final) o.final[i] = final;
        if (o.peak) o.peak[i] = b.peak[i];
        if (o.peak_event) o.peak_event[i] = pe;
        if (o.last_pos) o.last_pos[i] = last;
        if (o.peak_time) o.peak_time[i] = when(pe);
        if (o.ext_time) o.ext_time[i] = last >= -1 && final == 0 ? when((int64_t)last + 1) : __builtin_nan("");
        for (int32_t k = 0; k < K; k++) {
            const int32_t fe = b.first[(int64_t)k * cells + i];
            if (o.first) o.first[(int64_t)k * cells + i] = fe;
            if (o.first_time) o.first_time[(int64_t)k * cells + i] = when(fe);
        }
    }
}

// launch arguments of the walk and of the peak reduction (vgx_tau_milestones.hip), filled by vgx_get_tau_milestones: pass A's
// launch and what the walk adds
struct VgxTauMsLaunch {
    VgxTauPrevLaunch a;        // T = tiles of the launch's longest chain, bound[j] = first row of tile min(j, tiles), val the running sums after the scan
    int32_t K;
    int64_t theta[VGX_MS_MAX_K];
    const int32_t *ev_row;     // first row of every event of every chain, events + 1 entries per chain, relative to the chain's first row
    const int64_t *ev_off;     // [m] where the chain's entries begin in ev_row
    const int32_t *tile_ev;    // [m][T + 1] first event of every tile, the chain's event count from its last tile on
    const int32_t *n_tiles;    // [m]
    const int32_t *ev0;        // [m] the index of the chain's first event along the whole chain (the prefix's events come before)
    int64_t max_tiles;         // most tiles of a chain of the launch
    int64_t *peak;             // [m][cells] the block: in, and out after the reduction
    int32_t *peak_event;       // [m][cells]
    int32_t *last_pos;         // [m][cells]
    int32_t *first;            // [m][K][cells]
    int64_t *slot_peak;        // [m][T][cells] every tile's peak ...
    int32_t *slot_event;       // [m][T][cells] ... and its event, VGX_MS_NONE: none
};
