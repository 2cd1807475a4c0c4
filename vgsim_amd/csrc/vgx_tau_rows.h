// vgx_tau_rows.h — host: the flattened list of a chain's events as weighted rows in the 48-byte layout of the multievent log (the
// prefix of a tau call, or a whole chain in a test hook).  Host-only; the frame of the tau replays (vgx_tau_replay.h) builds on
// it, and through the frame the six units that read tau chains as rows: vgx_tau_timelines.hip, vgx_tau_incidence.hip,
// vgx_tau_flows.hip, vgx_tau_prevalence.hip, vgx_tau_susceptible.hip and vgx_tau_milestones.hip.  `flatten` is inline: one
// definition for all of them.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>
#include "vgx_tline.h"

#pragma GCC visibility push(hidden)   // nothing here is part of the exported C ABI

// ---- host: the flattened list of a chain's events (the prefix of a call, or a whole chain in the test hook)
struct EventCols {
    int64_t n;
    const double *times;
    const int64_t *types, *hap, *pop, *nh, *np;
};
struct RowCols {
    int64_t n;
    const int64_t *num, *types, *hap, *pop, *nh, *np;
};
struct FlatChain {
    std::vector<int64_t> rows;       // [n][6]
    std::vector<int64_t> ev_row;     // [events + 1] first row of every event
    std::vector<double> ev_max;      // [events] running maximum of the event times
    int64_t n_rows() const { return (int64_t)rows.size() / 6; }
};

// events [0, n_ev) of `ev` as rows; "" or why not
inline std::string flatten(const EventCols &ev, int64_t n_ev, const RowCols &mv, FlatChain &f) {
    f.rows.clear();
    f.ev_row.assign((size_t)n_ev + 1, 0);
    f.ev_max.resize((size_t)n_ev);
    double mx = 0.0;
    auto ok32 = [](int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; };
    for (int64_t i = 0; i < n_ev; i++) {
        f.ev_row[(size_t)i] = f.n_rows();
        mx = i == 0 ? ev.times[0] : std::max(mx, ev.times[i]);
        f.ev_max[(size_t)i] = mx;
        const int64_t t = ev.types[i];
        if (t == VGX_TL_MULTITYPE) {
            const int64_t j0 = ev.hap[i], j1 = ev.pop[i];
            if (j1 <= j0) continue;                      // a step without rows is still an event
            if (j0 < 0 || j1 > mv.n || !mv.num) return "event " + std::to_string(i) + ": MULTITYPE row range outside the multievent log";
            for (int64_t j = j0; j < j1; j++) {
                const int64_t v[6] = {mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]};
                if (v[0] < 0 || v[1] < 0 || v[1] >= VGX_TL_ROW_DIRECT || !ok32(v[2]) || !ok32(v[3]) || !ok32(v[4]) || !ok32(v[5]))
                    return "multievent row " + std::to_string(j) + ": value out of range";
                f.rows.insert(f.rows.end(), v, v + 6);
            }
        } else {
            const int64_t v[6] = {1, t | VGX_TL_ROW_DIRECT, ev.hap[i], ev.pop[i], ev.nh[i], ev.np[i]};
            if (t < 0 || t >= VGX_TL_ROW_DIRECT || !ok32(v[2]) || !ok32(v[3]) || !ok32(v[4]) || !ok32(v[5]))
                return "event " + std::to_string(i) + ": log value outside 32 bits";
            f.rows.insert(f.rows.end(), v, v + 6);
        }
        if (f.n_rows() >= ((int64_t)1 << 31)) return "the chain has 2^31 rows or more";
    }
    f.ev_row[(size_t)n_ev] = f.n_rows();
    return "";
}

#pragma GCC visibility pop
