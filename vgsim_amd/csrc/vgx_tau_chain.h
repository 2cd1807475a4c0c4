// vgx_tau_chain.h — a tau chain's events as the 32-byte rows of vgx_gwalk_tau.h, on the host: what the host sides of
// vgx_get_tau_genealogies and vgx_get_tau_lineages and their test hooks share.  The prefix (the model's chain before the tau call)
// flattened into rows, the capacities its rows can add to a replicate's workspace, and the chain of a test hook (prefix plus the
// trailing MULTITYPE events as own steps, brought into canonical rows by the device's key and merge rule).  Host only.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_gwalk_tau.h"

namespace vgxtc {

struct EventCols {
    int64_t n;
    const double *times;
    const int64_t *types, *hap, *pop, *nh, *np;
};
struct RowCols {
    int64_t n;
    const int64_t *num;
    const double *times;
    const int64_t *types, *hap, *pop, *nh, *np;
};
struct FlatChain {
    std::vector<VgxGtRow> rows;
    std::vector<int32_t> off;        // [events + 1]
    std::vector<double> time;        // [events] what the host pass writes for a node or record of the event
};

// sum of min(v, cap) over a list of values, for many caps
struct CappedSum {
    std::vector<int64_t> v, pre;     // sorted, prefix sums
    void add(int64_t x) { v.push_back(x); }
    void close() {
        std::sort(v.begin(), v.end());
        pre.assign(v.size() + 1, 0);
        for (size_t i = 0; i < v.size(); i++) pre[i + 1] = pre[i] + v[i];
    }
    int64_t operator()(int64_t cap) const {
        const size_t k = (size_t)(std::upper_bound(v.begin(), v.end(), cap) - v.begin());
        return pre[k] + (int64_t)(v.size() - k) * cap;
    }
};

// events [0, n_ev) of `ev` as rows; "" or why not
inline std::string flatten(const EventCols &ev, int64_t n_ev, const RowCols &mv, int64_t P, int64_t H, FlatChain &f) {
    f.rows.clear();
    f.off.assign((size_t)n_ev + 1, 0);
    f.time.assign((size_t)n_ev, 0.0);
    auto ok32 = [](int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; };
    for (int64_t i = 0; i < n_ev; i++) {
        f.off[(size_t)i] = (int32_t)f.rows.size();
        f.time[(size_t)i] = ev.times[i];
        const int64_t t = ev.types[i];
        if (t == VGX_GW_MULTITYPE_EV) {
            const int64_t j0 = ev.hap[i], j1 = ev.pop[i];
            if (j1 <= j0) continue;
            if (j0 < 0 || j1 > mv.n || !mv.num) return "event " + std::to_string(i) + ": MULTITYPE row range outside the multievent log";
            if (mv.times) f.time[(size_t)i] = mv.times[j0];
            for (int64_t j = j0; j < j1; j++) {
                if (mv.types[j] < 0 || mv.types[j] >= VGX_GT_ROW_DIRECT || !ok32(mv.hap[j]) || !ok32(mv.pop[j]) || !ok32(mv.nh[j]) || !ok32(mv.np[j]) ||
                    !vgx_gt_row_ok(P, H, mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]))
                    return "multievent row " + std::to_string(j) + ": value out of range";
                f.rows.push_back({mv.num[j], (int32_t)mv.types[j], (int32_t)mv.hap[j], (int32_t)mv.pop[j], (int32_t)mv.nh[j], (int32_t)mv.np[j], 0});
            }
        } else {
            if (t < 0 || t >= VGX_GT_ROW_DIRECT || !ok32(ev.hap[i]) || !ok32(ev.pop[i]) || !ok32(ev.nh[i]) || !ok32(ev.np[i]) ||
                !vgx_gt_row_ok(P, H, 1, t, ev.hap[i], ev.pop[i], ev.nh[i], ev.np[i]))
                return "event " + std::to_string(i) + ": value out of range";
            f.rows.push_back({1, (int32_t)(t | VGX_GT_ROW_DIRECT), (int32_t)ev.hap[i], (int32_t)ev.pop[i], (int32_t)ev.nh[i], (int32_t)ev.np[i], 0});
        }
        if (f.rows.size() >= ((size_t)1 << 30)) return "the chain has 2^30 rows or more";
    }
    f.off[(size_t)n_ev] = (int32_t)f.rows.size();
    return "";
}

// what the rows of a flattened chain can add to the record and lineage capacities
struct FlatCaps {
    CappedSum mut, mig, push;
    int64_t direct_mut = 0, direct_mig = 0, direct_push = 0;
    void of(const FlatChain &f) {
        for (const VgxGtRow &r : f.rows) {
            const int32_t t = r.type & ~(int32_t)VGX_GT_ROW_DIRECT;
            if (r.type & VGX_GT_ROW_DIRECT) {
                direct_mut += t == VGX_GW_MUTATION;
                direct_mig += t == VGX_GW_MIGRATION;
                direct_push += t == VGX_GW_SAMPLING || t == VGX_GW_MUTATION || t == VGX_GW_MIGRATION;
            } else {
                if (t == VGX_GW_MUTATION) mut.add(r.num);
                if (t == VGX_GW_MIGRATION) mig.add(r.num);
                if (t == VGX_GW_BIRTH || t == VGX_GW_SAMPLING || t == VGX_GW_MUTATION || t == VGX_GW_MIGRATION) push.add(r.num);
            }
        }
        mut.close(); mig.close(); push.close();
    }
};

// The chain of a test hook's vgx_genealogy_io: the trailing MULTITYPE events play the replicate's own steps (their rows in any
// order and granularity, brought into canonical rows by the device's key and merge rule), everything before them the prefix,
// whose rows are taken as they are.  With the sizes of the walk's workspace.
struct HostChain {
    FlatChain pre;
    int64_t n_pre = 0;
    std::vector<VgxGtRow> can;
    std::vector<int32_t> can_off;
    std::vector<double> step_time;
    FlatCaps caps;
    int64_t tsize = 0, arena_cap = 0;
    VgxGtChain chain(int64_t n) const { return VgxGtChain{pre.rows.data(), pre.off.data(), n_pre, can.data(), can_off.data(), n - n_pre}; }
    double time_of(int32_t e) const { return e < 0 ? 0.0 : (e < n_pre ? pre.time[(size_t)e] : step_time[(size_t)(e - n_pre)]); }
};

// "" or why not (`me` goes before the hook's own refusals; the text of a status comes from `message`)
template <class Message>
inline std::string host_chain(const vgx_genealogy_io *io, int64_t sites, const std::string &me, Message message, HostChain &hc) {
    const int64_t n = io->ev_ptr, P = io->popNum, H = io->hapNum, PH = P * H, sC = io->sCounter;
    int64_t n_pre = n;
    while (n_pre > 0 && io->ev_types[n_pre - 1] == VGX_GW_MULTITYPE_EV) n_pre--;
    hc.n_pre = n_pre;
    const EventCols ev{n, io->ev_times, io->ev_types, io->ev_haplotypes, io->ev_populations, io->ev_newHaplotypes, io->ev_newPopulations};
    const RowCols mv{io->mev_num ? io->mev_rows : 0, io->mev_num, io->mev_times, io->mev_types, io->mev_haplotypes, io->mev_populations,
                     io->mev_newHaplotypes, io->mev_newPopulations};
    std::string why = flatten(ev, n_pre, mv, P, H, hc.pre);
    if (!why.empty()) return me + why;
    // the own steps: canonical rows by the device's key and merge rule
    std::vector<VgxGtRow> &can = hc.can;
    can.clear();
    hc.can_off.assign((size_t)(n - n_pre) + 1, 0);
    hc.step_time.assign((size_t)(n - n_pre), 0.0);
    struct Keyed { uint64_t hi, lo; int64_t j; };
    std::vector<Keyed> keys;
    for (int64_t k = 0; k < n - n_pre; k++) {
        const int64_t e = n_pre + k, j0 = io->ev_haplotypes[e], j1 = io->ev_populations[e];
        hc.can_off[(size_t)k] = (int32_t)can.size();
        hc.step_time[(size_t)k] = io->ev_times[e];
        if (j1 <= j0) continue;
        if (j0 < 0 || j1 > mv.n) return me + "event " + std::to_string(e) + ": MULTITYPE row range outside the multievent log";
        if (j1 - j0 > VGX_GT_STEP_ROWS_MAX) return message(VGX_GW_STEP_ROWS, k);
        if (mv.times) hc.step_time[(size_t)k] = mv.times[j0];
        keys.clear();
        for (int64_t j = j0; j < j1; j++) {
            if (mv.types[j] < 0 || mv.types[j] >= VGX_GT_ROW_DIRECT || !vgx_gt_row_ok(P, H, mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]))
                return message(VGX_GW_BAD_ROW, k);
            Keyed q{0, 0, j};
            vgx_gt_row_key(sites, mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j], q.hi, q.lo);
            keys.push_back(q);
        }
        std::sort(keys.begin(), keys.end(), [](const Keyed &x, const Keyed &y) { return x.hi != y.hi ? x.hi < y.hi : (x.lo != y.lo ? x.lo < y.lo : x.j < y.j); });
        for (size_t i = 0; i < keys.size(); i++) {
            const int64_t j = keys[i].j;
            if (i == 0 || keys[i].hi != keys[i - 1].hi || keys[i].lo != keys[i - 1].lo)
                can.push_back({0, (int32_t)mv.types[j], (int32_t)mv.hap[j], (int32_t)mv.pop[j], (int32_t)mv.nh[j], (int32_t)mv.np[j], 0});
            can.back().num += mv.num[j];
        }
    }
    hc.can_off[(size_t)(n - n_pre)] = (int32_t)can.size();
    hc.caps.of(hc.pre);
    int64_t pushes = hc.caps.direct_push + hc.caps.push(sC);
    for (const VgxGtRow &r : can) pushes += vgx_gt_row_pushes(r.type, r.num, sC);
    hc.tsize = vgx_gw_table_size((int64_t)(hc.pre.rows.size() + can.size()), PH);
    hc.arena_cap = std::min(pushes, (hc.tsize / 2) * sC);
    return "";
}

}  // namespace vgxtc
