// vgx_tau_replay.h — the frame the replays of TAU chains share: vgx_tau_incidence.hip, vgx_tau_flows.hip,
// vgx_tau_prevalence.hip, vgx_tau_susceptible.hip, vgx_tau_milestones.hip and vgx_tau_timelines.hip.  A unit keeps what is its
// own (rule header, counting or walk kernel, launcher, check_request / check_grid, entry points) and reads as: check the request,
// select, lay out, prefix pass, chunks, copy out, summary.  Everything around that is here, once:
//   tau_select                       the engine-state check, the replicate selection, the prefix flattened
//   tau_prefix_marks, tau_own_marks  a chain's cuts (VgxIncCutter, first slot 0) or bounds (VgxPrevCutter, first slot 1)
//   tau_hook_split, _marks, _count   the chain of a CPU test hook split into prefix and own rows, and counted like the device's
//   DevLayout, DevHold, dev_alloc    256-byte aligned offsets into one device allocation, held until the call returns
//   tau_timed                        event, launches, event, sync, elapsed time added to ms[0]
//   tau_prefix_pass, tau_chunks      the device frame of the four binned replays
//   tau_summary                      an int64 block narrowed, refused at 2^31, summarised by column
//   wave_sum, add64, flat_grid       what their kernels and flat launches share
// The templates are inline here; what needs no template, and the init kernel, is compiled once in vgx_tau_replay.hip.
#pragma once
#include "vgx_engine.h"
#include "vgx_tau_rows.h"   // EventCols, RowCols, FlatChain, flatten

#pragma GCC visibility push(hidden)   // nothing here is part of the exported C ABI

// ---- device helpers
static __device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

static __device__ __forceinline__ void add64(long long *p, long long v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);   // two's complement: the sum is the signed one
}

// workgroups of 256 threads that stride over `total` items
inline unsigned flat_grid(int64_t total) { return (unsigned)std::min<int64_t>(std::max<int64_t>((total + 255) / 256, 1), 1 << 16); }

// The net blocks (tc value cells and `cells` tail cells per chain; cells = 0: no tail blocks) and `outside` counters of m chains
// start from the prefix's (with[i] != 0) or from zero.  vgx_tau_replay.hip
extern "C" hipError_t vgxi_tau_block_init(int64_t m, int64_t tc, int64_t cells, const int32_t *with, const int64_t *pre_val, const int64_t *pre_fin,
                                          const int64_t *pre_out, int64_t *val, int64_t *fin, int64_t *outside, hipStream_t s);

// ---- selection
struct TauSel {
    int64_t pre_ev = 0, pre_loc = 0, pre_rows = 0;   // the prefix: its events, its lockdown records, its flattened rows
    bool any_prefix = false;
    std::vector<int32_t> n_own, with_prefix;         // [n] own rows of a replicate; whether its chain starts with the prefix
    FlatChain pre;
};
// Checks that the engine holds a tau call with its rows (`verb`: what the caller does with tau chains only), then `request`
// ("" or why the caller refuses), the prefix columns (`lockdown`: the lockdown columns too), every selected replicate (last of its
// checks each(i, r, with_prefix): "" or why replicate r at place i is refused; tau_every: nothing more), flattens the prefix if a
// chain carries it and checks the 2^31 row limit.
template <class Request, class Each>
int tau_select(vgx_engine *e, const std::string &me, const char *verb, Request request, int64_t n, const int64_t *replicates,
               const vgx_timelines_prefix *prefix, bool lockdown, Each each, TauSel &s) {
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (" + verb + " tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    {
        const std::string why = request();
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + why);
    }
    // the prefix: what the model held when the call started
    const int64_t pre_ev = s.pre_ev = prefix ? prefix->ev_ptr : 0, mev_cap = e->tau_mev_cap;
    s.pre_loc = prefix ? std::max<int64_t>(prefix->loc_n, 0) : 0;
    if (pre_ev < 0 || (pre_ev > 0 && (!prefix->ev_times || !prefix->ev_types || !prefix->ev_haplotypes || !prefix->ev_populations ||
                                      !prefix->ev_newHaplotypes || !prefix->ev_newPopulations)))
        return fail(e, VGX_ERR_ARG, me + "null prefix column");
    if (lockdown && s.pre_loc > 0 && (!prefix->loc_state || !prefix->loc_pop || !prefix->loc_time)) return fail(e, VGX_ERR_ARG, me + "null prefix lockdown column");
    s.n_own.assign((size_t)n, 0);
    s.with_prefix.assign((size_t)n, 0);
    s.any_prefix = false;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &sc = e->sc_host[(size_t)r];
            const int64_t first = sc.restarts > 0 ? 0 : e->ev_ptr0;   // vgx_counters.ev_first_new
            if (sc.restarts == 0 && first != pre_ev)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain continues a log of " + std::to_string(first) +
                                                " events, the prefix holds " + std::to_string(pre_ev));
            s.with_prefix[(size_t)i] = sc.restarts == 0 && pre_ev > 0;
            s.any_prefix = s.any_prefix || s.with_prefix[(size_t)i];
            const auto &lg = e->tau_log[(size_t)r];
            for (size_t k = 0; k < lg.size(); k++)   // the steps' row ranges tile the replicate's block
                if (lg[k].m0 != (k ? lg[k - 1].m1 : 0) || lg[k].m1 < lg[k].m0)
                    return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": row ranges of its steps are not contiguous");
            if (!lg.empty() && lg.back().m1 > mev_cap) return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " logged more rows than its block holds");
            const std::string why = each(i, r, s.with_prefix[(size_t)i] != 0);
            if (!why.empty()) return fail(e, VGX_ERR_ARG, me + why);
        }
    }
    s.pre = FlatChain();
    s.pre.ev_row.assign(1, 0);
    if (s.any_prefix) {
        const EventCols ev{pre_ev, prefix->ev_times, prefix->ev_types, prefix->ev_haplotypes, prefix->ev_populations, prefix->ev_newHaplotypes, prefix->ev_newPopulations};
        const RowCols mv{prefix->mev_rows, prefix->mev_num, prefix->mev_types, prefix->mev_haplotypes, prefix->mev_populations, prefix->mev_newHaplotypes,
                         prefix->mev_newPopulations};
        if (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np)) return fail(e, VGX_ERR_ARG, me + "null prefix multievent column");
        const std::string why = flatten(ev, pre_ev, mv, s.pre);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + "prefix: " + why);
    }
    s.pre_rows = s.pre.n_rows();
    for (int64_t i = 0; i < n; i++) {
        const auto &lg = e->tau_log[(size_t)replicates[i]];
        const int64_t own = lg.empty() ? 0 : lg.back().m1, total = (s.with_prefix[(size_t)i] ? s.pre_rows : 0) + own;
        if (total >= ((int64_t)1 << 31))
            return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(replicates[i]) + ": prefix and own rows reach 2^31 (" + std::to_string(total) + ")");
        s.n_own[(size_t)i] = (int32_t)own;
    }
    return VGX_OK;
}
// a selection with nothing of its own to check per replicate
inline std::string tau_every(int64_t, int64_t, bool) { return ""; }

// ---- cuts.  Cutter: VgxIncCutter (marks: T + 1 cuts, FIRST = 0) or VgxPrevCutter (marks: T + 2 bounds, FIRST = 1)
// The prefix as a chain of its own: its marks (the literal loop over its events, then its row count) and where the loop stands
// after it
template <class Cutter, int FIRST>
int64_t tau_prefix_marks(const FlatChain &f, int64_t n_ev, const double *times, const double *grid, int64_t T, int32_t *mark) {
    Cutter ct{grid, T, mark};
    for (int64_t i = 0; i < n_ev; i++) ct.event(f.ev_row[(size_t)i], times[i]);
    const int64_t point0 = ct.point;
    ct.finish(f.ev_row[(size_t)n_ev]);
    return point0;
}

// A chain's own events after a prefix that left the loop at point0: marks relative to the chain's first own row
template <class Cutter, int FIRST, class OwnTime, class OwnRow>
void tau_own_marks(const double *grid, int64_t T, int64_t point0, int64_t n_own, OwnTime own_time, OwnRow own_m0, int64_t n_rows, int32_t *mark) {
    for (int64_t k = 0; k < point0; k++) mark[FIRST + k] = 0;   // these cuts lie inside the prefix: before the first own row
    Cutter ct{grid, T, mark};
    ct.point = point0;
    for (int64_t k = 0; k < n_own; k++) ct.event(own_m0(k), own_time(k));
    ct.finish(n_rows);
}

// ---- the CPU test hooks: the last n_own_ev events of a chain given as arrays play the replicate's own steps (their rows are
// taken as they are, as the device reads t_mev), everything before them the prefix, which is flattened
struct TauHookChain {
    int64_t n_pre_ev = 0, n_own_ev = 0, tile = 0;
    FlatChain pre;
    std::vector<int64_t> own, own_m0;   // [own rows][6]; [n_own_ev + 1] first own row of every own event, then the own rows
    int64_t pre_rows() const { return pre.n_rows(); }
    int64_t own_rows() const { return (int64_t)own.size() / 6; }
};
// block: cells of the hook's [T] block (refused at 2^40), or 0.  "" or why not
std::string tau_hook_split(const EventCols &ev, const RowCols &mv, int64_t tile, int64_t tile_default, int64_t block, int64_t n_own_events, TauHookChain &c);
template <class Io>
std::string tau_hook_split(const Io *io, int64_t tile_default, int64_t block, TauHookChain &c) {
    return tau_hook_split(EventCols{io->ev_ptr, io->ev_times, io->ev_types, io->ev_haplotypes, io->ev_populations, io->ev_newHaplotypes, io->ev_newPopulations},
                          RowCols{io->mev_rows, io->mev_num, io->mev_types, io->mev_haplotypes, io->mev_populations, io->mev_newHaplotypes, io->mev_newPopulations},
                          io->tile, tile_default, block, io->n_own_events, c);
}

// the marks of the prefix and of the own rows
template <class Cutter, int FIRST>
void tau_hook_marks(const TauHookChain &c, const double *times, const double *grid, int64_t T, std::vector<int32_t> &pmark, std::vector<int32_t> &omark) {
    pmark.assign((size_t)(T + 1 + FIRST), 0);
    omark.assign((size_t)(T + 1 + FIRST), 0);
    const int64_t point0 = tau_prefix_marks<Cutter, FIRST>(c.pre, c.n_pre_ev, times, grid, T, pmark.data());
    tau_own_marks<Cutter, FIRST>(grid, T, point0, c.n_own_ev, [&](int64_t k) { return times[c.n_pre_ev + k]; }, [&](int64_t k) { return c.own_m0[(size_t)k]; },
                                 c.own_rows(), omark.data());
}

// The prefix tiles counted once into blocks of their own; the chain's blocks dst[k] (len[k] cells) start from them and the own
// tiles are counted on top.  tile_host(rows, marks, t0, t1, blocks): the unit's *_tile_host on rows [t0, t1)
template <int NB, class TileHost>
void tau_hook_count(const TauHookChain &c, const int32_t *pmark, const int32_t *omark, int64_t *const (&dst)[NB], const int64_t (&len)[NB], TileHost tile_host) {
    std::vector<int64_t> pre[NB];
    int64_t *pblock[NB];
    for (int k = 0; k < NB; k++) {
        pre[k].assign((size_t)len[k], 0);
        pblock[k] = pre[k].data();
    }
    for (int64_t t0 = 0; t0 < c.pre_rows(); t0 += c.tile)
        tile_host(c.pre.rows.data(), pmark, (int32_t)t0, (int32_t)std::min<int64_t>(t0 + c.tile, c.pre_rows()), pblock);
    for (int k = 0; k < NB; k++) std::copy(pre[k].begin(), pre[k].end(), dst[k]);
    for (int64_t t0 = 0; t0 < c.own_rows(); t0 += c.tile)
        tile_host(c.own.data(), omark, (int32_t)t0, (int32_t)std::min<int64_t>(t0 + c.tile, c.own_rows()), dst);
}

// a state [P][H] folded through variant_of: [P][V]
std::vector<int64_t> tau_fold_state(const std::vector<int64_t> &src, int64_t P, int64_t H, int64_t V, const int32_t *variant_of);

// ---- device workspace
struct DevLayout {   // regions of one allocation in the order they are taken, each from a 256-byte aligned offset
    int64_t total = 0;
    static int64_t up(int64_t bytes) { return (bytes + 255) / 256 * 256; }
    int64_t take(int64_t bytes) {
        const int64_t at = total;
        total += up(bytes);
        return at;
    }
};
struct DevFree {
    void operator()(char *p) const { (void)hipFree(p); }
};
typedef std::unique_ptr<char, DevFree> DevHold;
int dev_alloc(vgx_engine *e, const std::string &me, int64_t bytes, DevHold &hold);

// bytes of device memory the chunks of a call may take: `room`, at most 2^30, at most VGX_TIMELINES_CHUNK_BYTES
int64_t tau_chunk_share(int64_t room);

// ---- timed section: what `body` puts on the stream between the engine's two events, `after` behind them; their time is added to
// ms[0].  failed: the caller's text for a kernel that failed, ": " included
template <class Body, class After>
int tau_timed(vgx_engine *e, double *ms, const std::string &failed, Body body, After after) {
    HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
    if (const int rc = body()) return rc;
    HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
    if (const int rc = after()) return rc;
    const hipError_t er = hipStreamSynchronize(e->stream);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, failed + hipGetErrorString(er));
    float kms = 0.f;
    HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
    ms[0] += kms;
    return VGX_OK;
}
template <class Body>
int tau_timed(vgx_engine *e, double *ms, const std::string &failed, Body body) {
    return tau_timed(e, ms, failed, body, []() { return (int)VGX_OK; });
}

// ---- the device frame of the binned replays (incidence, flows, prevalence, susceptibles)
// The prefix, once, if a selected chain carries it: its marks (host time to ms[1]), its rows, marks and row count uploaded to
// d_rows, d_marks, d_n, then `count` (the unit's launch over this one chain) as a timed section.  point0: where the loop stands
// after the prefix
template <class Cutter, int FIRST, class Count>
int tau_prefix_pass(vgx_engine *e, const std::string &me, double *ms, const TauSel &s, const double *times, const double *grid, int64_t T, char *d_rows,
                    char *d_marks, char *d_n, int64_t &point0, Count count) {
    point0 = 0;
    if (!s.any_prefix) return VGX_OK;
    std::vector<int32_t> marks((size_t)(T + 1 + FIRST), 0);
    const int32_t pn = (int32_t)s.pre_rows;
    const auto t_cuts = std::chrono::steady_clock::now();
    point0 = tau_prefix_marks<Cutter, FIRST>(s.pre, s.pre_ev, times, grid, T, marks.data());
    ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_cuts).count();
    if (s.pre_rows > 0) HIPCHECK(e, hipMemcpyAsync(d_rows, s.pre.rows.data(), (size_t)s.pre_rows * 48, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(d_marks, marks.data(), marks.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(d_n, &pn, 4, hipMemcpyHostToDevice, e->stream));
    return tau_timed(e, ms, me + "counting kernel failed on the prefix: ", count);
}

// Chunks of replicates: the marks of a chunk fit the share of `room` (bytes of device memory the call leaves free of its half).
// Per chunk: every replicate's marks in the row index space of its own block (the loop continued where the prefix left it; host
// time to ms[1]), uploaded, then enqueue(i0, m, max_n, marks on the device) as a timed section.  failed: as tau_timed takes it
template <class Cutter, int FIRST, class Enqueue>
int tau_chunks(vgx_engine *e, const std::string &me, const std::string &failed, double *ms, const TauSel &s, int64_t n, const int64_t *replicates,
               const double *grid, int64_t T, int64_t point0, int64_t room, Enqueue enqueue) {
    const int64_t per_chain = T + 1 + FIRST, per_rep = per_chain * 4 + 64;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(tau_chunk_share(room + 4096) / per_rep, (int64_t)1 << 20));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t m = std::min(n, i0 + chunk) - i0;
        DevHold hold;
        if (const int rc = dev_alloc(e, me, DevLayout::up(m * per_chain * 4), hold)) return rc;
        const auto t_cuts = std::chrono::steady_clock::now();
        std::vector<int32_t> marks((size_t)(m * per_chain));
        int64_t steps_all = 0, max_n = 0;
        for (int64_t j = 0; j < m; j++) {
            steps_all += (int64_t)e->tau_log[(size_t)replicates[i0 + j]].size();
            max_n = std::max<int64_t>(max_n, s.n_own[(size_t)(i0 + j)]);
        }
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j;
                const auto &lg = e->tau_log[(size_t)replicates[gi]];
                tau_own_marks<Cutter, FIRST>(grid, T, s.with_prefix[(size_t)gi] ? point0 : 0, (int64_t)lg.size(), [&](int64_t k) { return lg[(size_t)k].time; },
                                             [&](int64_t k) { return lg[(size_t)k].m0; }, s.n_own[(size_t)gi], marks.data() + j * per_chain);
            }
        }, std::max<int64_t>(steps_all / std::max<int64_t>(m, 1), 1) + T);
        ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_cuts).count();
        HIPCHECK(e, hipMemcpyAsync(hold.get(), marks.data(), marks.size() * 4, hipMemcpyHostToDevice, e->stream));
        if (const int rc = tau_timed(e, ms, failed, [&]() -> int { return enqueue(i0, m, max_n, (const int32_t *)hold.get()); })) return rc;
    }
    return VGX_OK;
}

// ---- summary tail: the int64 block [n][tc] narrowed to int32 at `narrow` with its extremes at mm[2] (both on the device), refused
// where the column summary cannot take it, then summarised by column.  counts: the block holds counts (never negative), else
// values; the two refusals word it so
int tau_summary(vgx_engine *e, const std::string &me, bool counts, const int64_t *block, int64_t n, int64_t tc, int32_t *narrow, uint64_t *mm,
                vgx_traj_summary_io *summary, double *ms);

#pragma GCC visibility pop
