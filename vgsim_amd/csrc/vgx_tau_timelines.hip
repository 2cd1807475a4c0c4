// vgx_tau_timelines.hip — the log replays (get_data_infectious / get_data_susceptible, reference pyx:1967-2045) of every replicate
// of a TAU ensemble on the device (vgx_get_tau_timelines), the host side of that call, and the same replay compiled for the host
// (vgx_test_tau_timelines).
//
// The chain of a replicate is one list of weighted rows (vgx_tline.h): the model's chain before the call, flattened once per call
// into the 48-byte row layout of the multievent log and shared by all replicates, then the replicate's own rows where the tau
// kernels left them (its block of t_mev, blocks mev_cap rows apart).  Nothing is copied or compacted: a row index below the
// prefix length reads the prefix buffer, any other the replicate's block.  Times stay on the host, where they already are
// (prefix event times, the step times of tau_log): per replicate they become step_num cuts in ROW index space
// (vgx_tl_row_cuts), and everything after that is integer work.
//
// REPLAY kernel: one workgroup of 256 threads per replicate, consecutive lanes consecutive rows (three 16-byte loads per lane:
// every byte of a fetched line is used), two tiles of 256 rows in flight.  Per row: its bin from the cuts in LDS (one comparison
// unless a cut was passed), the at most two compartments it moves looked up in the LDS query table, `num` added to 64-bit per-bin
// counters in LDS (a bin sums num over many steps, and the all-DEATH+SAMPLING row of the reference semantics sums over every
// compartment: population sizes below 2^31 do not bound these sums).  The two query-independent rows are reduced per wavefront
// (a wave sum of num, one LDS add) when the wavefront's rows share a bin.  The finish is the int64 prefix sum over the bins of
// every series by wavefront scans, start + sum stored as f64 with coalesced stores.
// EXACTNESS: integer arithmetic up to the final conversion; every stored value is exact while its magnitude is below 2^53 (the
// reference accumulates the same sums in float64 and is exact in the same range).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_tau_replay.h"   // the frame: selection, workspace, timed sections, wave_sum; FlatChain and flatten of vgx_tau_rows.h

namespace {

struct VgxTtlLaunch {
    int64_t m;               // replicates of this pass = workgroups
    const int64_t *pre;      // [prefix rows][6] the flattened prefix (type | VGX_TL_ROW_DIRECT on rows of the direct rule)
    const int64_t *mev;      // t_mev: [R][mev_cap][6]
    int64_t mev_cap;
    const int64_t *rep;      // [m] replicate of every workgroup
    const int32_t *n_pre;    // [m] prefix rows of its chain (0 for a replicate that restarted)
    const int32_t *n_rows;   // [m] prefix + own rows
    const int32_t *last;     // [m] last_point
    const int32_t *cut;      // [m][step] row indices
    int step, semantics;
    int ni, ns;              // queries of this launch
    int i0, s0;              // ... their first index among all queries of the call
    int n_inf, n_sus;        // all queries of the call (row strides of the outputs)
    int tsize;               // slots of the query table
    const int32_t *tab;      // [3][tsize] major, minor', row
    const int64_t *start;    // [ni + ns] initial_infectious / initial_susceptible of the queried compartments
    double *inf, *smp, *sus; // [m][n_inf][T], [m][n_inf][T], [m][n_sus][T]
};

struct Row { longlong2 a, b, c; };   // num, type | haplotype, population | newHaplotype, newPopulation

// a field of a row as a 32-bit index: anything that is not one (never written by the tau kernels) matches no query
__device__ __forceinline__ int32_t idx32(long long v) { return (unsigned long long)v < 0x80000000ull ? (int32_t)v : -1; }

__device__ __forceinline__ void lds_add(long long *p, long long v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);   // two's complement: the sum is the signed one
}

__global__ void __launch_bounds__(256) vgxtt_replay_kernel(VgxTtlLaunch a) {
    extern __shared__ __attribute__((aligned(16))) long long lds64[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int step = a.step, T = step + 1, ni = a.ni, ns = a.ns, rows = 2 * ni + ns, ts = a.tsize;
    long long *g_ds = lds64, *g_s = g_ds + T, *cnt = g_s + T;
    int32_t *cut = (int32_t *)(cnt + (int64_t)rows * T), *tab = cut + step;
    for (int i = tid; i < step; i += 256) cut[i] = a.cut[b * step + i];
    for (int i = tid; i < 3 * ts; i += 256) tab[i] = a.tab[i];
    for (int i = tid; i < (2 + rows) * T; i += 256) g_ds[i] = 0;
    __syncthreads();
    const int32_t n = a.n_rows[b], npre = a.n_pre[b];
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *pre = (const longlong2 *)a.pre;
    const longlong2 *own = (const longlong2 *)(a.mev + a.rep[b] * a.mev_cap * 6);
    const bool reference = a.semantics == VGX_TL_REFERENCE;
    int bin = 0;

    auto load = [&](int32_t e, Row &r) {
        if (e < n) {
            const longlong2 *p = e < npre ? pre + (int64_t)e * 3 : own + (int64_t)(e - npre) * 3;
            r.a = p[0]; r.b = p[1]; r.c = p[2];
        } else {
            r.a = r.b = r.c = make_longlong2(0, -1);   // num 0, no type
        }
    };
    auto apply = [&](int32_t e, const Row &r) {
        const bool act = e < n;
        if (act) bin = vgx_tl_bin(cut, step, e, bin);
        const long long ty = r.a.y;
        const int rule = (ty & VGX_TL_ROW_DIRECT) ? VGX_TL_RULE_DIRECT : VGX_TL_RULE_MULTIEVENT;
        const int32_t c[5] = {idx32(ty & ~(long long)VGX_TL_ROW_DIRECT), idx32(r.b.x), idx32(r.b.y), idx32(r.c.x), idx32(r.c.y)};
        VgxTlMoves m;
        const long long w = vgx_tl_classify_row(a.semantics, rule, r.a.x, c, m);   // (a row past the end: weight 0, type -1)
        if (reference) {
            // the rows every row of a type moves are the contended ones: one add per wavefront when its rows share a bin
            const long long wds = m.all_ds ? w : 0, wsm = m.all_s ? w : 0;
            if (__any(wds != 0)) {
                const int b0 = __shfl(bin, 0);
                if (__all(!act || bin == b0)) {
                    const long long sds = wave_sum(wds), ssm = wave_sum(wsm);
                    if (lane == 0) {
                        lds_add(&g_ds[b0], sds);
                        if (ssm) lds_add(&g_s[b0], ssm);
                    }
                } else {
                    if (wds) lds_add(&g_ds[bin], wds);
                    if (wsm) lds_add(&g_s[bin], wsm);
                }
            }
        }
        if (w == 0) return;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const VgxTlOp &o = m.op[k];
            if (o.side < 0) continue;
            const int32_t row = vgx_tl_find(tab, ts, o.side, o.major, o.minor);
            if (row < 0) continue;
            lds_add(&cnt[row * T + bin], o.delta < 0 ? -w : w);
            if (o.sample) lds_add(&cnt[(row + ni) * T + bin], w);
        }
    };
    // two tiles of 256 rows in flight per workgroup
    for (int64_t base = 0; base < n; base += 512) {
        Row r0, r1;
        // (an index past the end becomes n: no 32-bit overflow for chains near 2^31 rows)
        const int32_t e0 = base + tid < n ? (int32_t)(base + tid) : n;
        const int32_t e1 = base + 256 + tid < n ? (int32_t)(base + 256 + tid) : n;
        load(e0, r0);
        load(e1, r1);
        apply(e0, r0);
        apply(e1, r1);
    }
    __syncthreads();
    if (reference) {   // every infectious series takes the query-independent rows
        for (int i = tid; i < ni * T; i += 256) {
            const int c = i % T;
            cnt[i] -= g_ds[c];
            cnt[ni * T + i] += g_s[c];
        }
        __syncthreads();
    }
    // finish: prefix sums over the bins, a series per wavefront at a time
    const int last = a.last[b];
    for (int r = wave; r < rows; r += 4) {
        long long carry;
        double *dst;
        if (r < ni) { carry = a.start[r]; dst = a.inf + ((b * a.n_inf + a.i0 + r) * (int64_t)T); }
        else if (r < 2 * ni) { carry = 0; dst = a.smp + ((b * a.n_inf + a.i0 + (r - ni)) * (int64_t)T); }
        else { carry = a.start[r - ni]; dst = a.sus + ((b * a.n_sus + a.s0 + (r - 2 * ni)) * (int64_t)T); }
        double held = 0.0;
        for (int c0 = 0; c0 < T; c0 += 64) {
            const int c = c0 + lane;
            long long v = c < T ? cnt[r * T + c] : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long u = __shfl_up(v, d);
                if (lane >= d) v += u;
            }
            v += carry;
            carry = __shfl(v, 63);
            if (last >= c0 && last < c0 + 64) held = (double)__shfl(v, last - c0);
            if (c < T) dst[c] = c <= last ? (double)v : (reference ? 0.0 : held);   // after last_point: upstream's zeros / the value kept
        }
    }
}

hipError_t launch_replay(const VgxTtlLaunch *a, hipStream_t s) {
    if (a->m <= 0) return hipSuccess;
    const int64_t lds = vgx_ttl_lds_bytes(a->step, a->ni, a->ns);
    if (lds > VGX_TL_LDS_MAX) return hipErrorInvalidValue;
    hipError_t err = hipFuncSetAttribute((const void *)vgxtt_replay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtt_replay_kernel, dim3((unsigned)a->m), dim3(256), (size_t)lds, s, *a);
    return hipGetLastError();
}

// the queries of every launch: as many as the LDS budget holds, infectious ones first (the scheme of vgx_get_timelines with the
// byte formula of the 64-bit counters)
struct Group { int64_t i0, ni, s0, ns, tab_off, start_off; };

}  // namespace

extern "C" int vgx_get_tau_timelines(vgx_engine *e, vgx_timelines_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && !io->replicates) || io->n_inf < 0 || io->n_sus < 0) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_timelines: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, S = e->d.susNum, step = io->step_num, T = step + 1;
    const int64_t n_inf = io->n_inf, n_sus = io->n_sus, mev_cap = e->tau_mev_cap;
    auto request = [&]() -> std::string {
        if (step < 1) return "step_num must be at least 1";
        if (io->semantics != VGX_TL_REFERENCE && io->semantics != VGX_TL_COMPARTMENT) return "semantics must be 0 (reference) or 1 (compartment)";
        if ((n_inf > 0 && (!io->inf_pop || !io->inf_hap)) || (n_sus > 0 && (!io->sus_pop || !io->sus_grp)) || n_inf + n_sus >= ((int64_t)1 << 20))
            return "bad query list";
        std::vector<std::pair<int64_t, int64_t>> qi, qs;
        for (int64_t k = 0; k < n_inf; k++) {
            if (io->inf_pop[k] < 0 || io->inf_pop[k] >= P) return "population index out of range";
            if (io->inf_hap[k] < 0 || io->inf_hap[k] >= H) return "haplotype index out of range";
            qi.emplace_back(io->inf_pop[k], io->inf_hap[k]);
        }
        for (int64_t k = 0; k < n_sus; k++) {
            if (io->sus_pop[k] < 0 || io->sus_pop[k] >= P) return "population index out of range";
            if (io->sus_grp[k] < 0 || io->sus_grp[k] >= S) return "susceptibility group index out of range";
            qs.emplace_back(io->sus_pop[k], io->sus_grp[k]);
        }
        std::sort(qi.begin(), qi.end());
        std::sort(qs.begin(), qs.end());
        if (std::adjacent_find(qi.begin(), qi.end()) != qi.end() || std::adjacent_find(qs.begin(), qs.end()) != qs.end()) return "a query is given twice";
        return "";
    };
    TauSel sel;
    int64_t loc_need = 1;
    if (const int rc = tau_select(e, me, "replays", request, n, io->replicates, prefix, true, [&](int64_t, int64_t r, bool) -> std::string {
            loc_need = std::max<int64_t>(loc_need, (e->sc_host[(size_t)r].restarts == 0 ? sel.pre_loc : 0) + (int64_t)e->tau_loc_time[(size_t)r].size());
            return "";
        }, sel))
        return rc;
    const FlatChain &pre = sel.pre;
    const std::vector<int32_t> &with_prefix = sel.with_prefix;
    const int64_t pre_ev = sel.pre_ev, pre_loc = sel.pre_loc;
    std::vector<int32_t> n_pre((size_t)n), n_rows((size_t)n);   // prefix rows of a chain; prefix + own rows
    for (int64_t i = 0; i < n; i++) {
        n_pre[(size_t)i] = with_prefix[(size_t)i] ? (int32_t)sel.pre_rows : 0;
        n_rows[(size_t)i] = n_pre[(size_t)i] + sel.n_own[(size_t)i];
    }
    if (!io->time_points) {   // sizing
        io->loc_cap = loc_need;
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    if (!io->last_point || !io->loc_n || !io->loc_state || !io->loc_pop || !io->loc_time || (n_inf > 0 && (!io->inf_data || !io->inf_sample)) ||
        (n_sus > 0 && !io->sus_data))
        return fail(e, VGX_ERR_ARG, me + "null output");
    if (io->loc_cap < loc_need) return fail(e, VGX_ERR_ARG, me + "loc_cap smaller than the sizing call gave");
    const int64_t loc_cap = io->loc_cap;

    int64_t budget = VGX_TL_LDS_DEFAULT;
    if (const char *lb = getenv("VGX_TIMELINES_LDS_BYTES")) budget = std::min<int64_t>(std::max<int64_t>(atoll(lb), 1), VGX_TL_LDS_MAX);
    const int64_t need1 = std::max(n_inf > 0 ? vgx_ttl_lds_bytes(step, 1, 0) : 0, n_sus > 0 ? vgx_ttl_lds_bytes(step, 0, 1) : vgx_ttl_lds_bytes(step, 0, 0));
    if (need1 > VGX_TL_LDS_MAX)
        return fail(e, VGX_ERR_ARG, me + "step_num " + std::to_string(step) + " is too large: the counters of one query exceed a workgroup's LDS");
    budget = std::max(budget, need1);
    std::vector<Group> groups;
    std::vector<int32_t> h_tab;
    std::vector<int64_t> h_start;
    for (int64_t i = 0, s = 0; i < n_inf || s < n_sus;) {
        Group g{i, 0, s, 0, (int64_t)h_tab.size(), (int64_t)h_start.size()};
        while (i + g.ni < n_inf && vgx_ttl_lds_bytes(step, g.ni + 1, g.ns) <= budget) g.ni++;
        while (s + g.ns < n_sus && vgx_ttl_lds_bytes(step, g.ni, g.ns + 1) <= budget) g.ns++;
        const int ts = vgx_tl_table_size((int)(g.ni + g.ns));
        h_tab.resize(h_tab.size() + (size_t)(3 * ts), -1);
        int32_t *tab = h_tab.data() + g.tab_off;
        for (int64_t k = 0; k < g.ni; k++) {
            vgx_tl_insert(tab, ts, 0, (int32_t)io->inf_pop[i + k], (int32_t)io->inf_hap[i + k], (int32_t)k);
            h_start.push_back(e->hs.initial_infectious[(size_t)(io->inf_pop[i + k] * H + io->inf_hap[i + k])]);
        }
        for (int64_t k = 0; k < g.ns; k++) {
            vgx_tl_insert(tab, ts, 1, (int32_t)io->sus_pop[s + k], (int32_t)io->sus_grp[s + k], (int32_t)(2 * g.ni + k));
            h_start.push_back(e->hs.initial_susceptible[(size_t)(io->sus_pop[s + k] * S + io->sus_grp[s + k])]);
        }
        groups.push_back(g);
        i += g.ni;
        s += g.ns;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    // one allocation for what every chunk shares: [table | start | prefix rows], uploaded ONCE per call
    DevLayout ql;
    const int64_t q_tab = ql.take((int64_t)h_tab.size() * 4 + 8), q_start = ql.take((int64_t)h_start.size() * 8 + 8), q_pre = ql.take((int64_t)pre.rows.size() * 8 + 8);
    DevHold qhold;
    if (const int rc = dev_alloc(e, me, ql.total, qhold)) return rc;
    char *const qws = qhold.get();
    if (!h_tab.empty()) HIPCHECK(e, hipMemcpy(qws + q_tab, h_tab.data(), h_tab.size() * 4, hipMemcpyHostToDevice));
    if (!h_start.empty()) HIPCHECK(e, hipMemcpy(qws + q_start, h_start.data(), h_start.size() * 8, hipMemcpyHostToDevice));
    if (!pre.rows.empty()) HIPCHECK(e, hipMemcpy(qws + q_pre, pre.rows.data(), pre.rows.size() * 8, hipMemcpyHostToDevice));

    // chunks of replicates: cuts and outputs of a chunk fit `share` bytes of device memory
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    const int64_t share = tau_chunk_share((int64_t)(free_b / 2));
    const int64_t per_rep = step * 4 + (2 * n_inf + n_sus) * T * 8 + 64;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(share / per_rep, (int64_t)1 << 20));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t i1 = std::min(n, i0 + chunk), m = i1 - i0;
        // one allocation: [rep | n_pre | n_rows | last | cut | inf | smp | sus]
        DevLayout lay;
        const int64_t o_rep = lay.take(m * 8), o_npre = lay.take(m * 4), o_nrows = lay.take(m * 4), o_last = lay.take(m * 4), o_cut = lay.take(m * step * 4),
                      o_inf = lay.take(m * n_inf * T * 8), o_smp = lay.take(m * n_inf * T * 8), o_sus = lay.take(m * n_sus * T * 8);
        DevHold hold;
        if (const int rc = dev_alloc(e, me, lay.total, hold)) return rc;
        char *const ws = hold.get();
        // host: time_points, cuts in row index space, last_point, lockdown records
        const auto t_cuts = std::chrono::steady_clock::now();
        std::vector<int32_t> cuts((size_t)(m * step)), last((size_t)m);
        int64_t steps_all = 0;
        for (int64_t j = 0; j < m; j++) steps_all += (int64_t)e->tau_log[(size_t)io->replicates[i0 + j]].size();
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j, r = io->replicates[gi];
                const auto &lg = e->tau_log[(size_t)r];
                const bool wp = with_prefix[(size_t)gi];
                double *tp = io->time_points + gi * T;
                vgx_tl_time_points(e->sc_host[(size_t)r].currentTime, step, tp);
                const int64_t lp = vgx_tl_row_cuts(tp, step, wp ? pre_ev : 0, pre.ev_max.data(), pre.ev_row.data(), (int64_t)lg.size(),
                                                   [&](int64_t k) { return lg[(size_t)k].time; }, [&](int64_t k) { return lg[(size_t)k].m0; },
                                                   n_pre[(size_t)gi], n_rows[(size_t)gi], cuts.data() + j * step);
                last[(size_t)j] = (int32_t)lp;
                io->last_point[gi] = lp;
                int64_t nl = 0;
                auto put = [&](int64_t st, int64_t pp, double tt) {
                    io->loc_state[gi * loc_cap + nl] = st; io->loc_pop[gi * loc_cap + nl] = pp; io->loc_time[gi * loc_cap + nl] = tt;
                    nl++;
                };
                if (e->sc_host[(size_t)r].restarts == 0)
                    for (int64_t k = 0; k < pre_loc; k++) put(prefix->loc_state[k], prefix->loc_pop[k], prefix->loc_time[k]);
                const auto &lt = e->tau_loc_time[(size_t)r];
                for (size_t k = 0; k < lt.size(); k++) put(e->tau_loc_state[(size_t)r][k], e->tau_loc_pop[(size_t)r][k], lt[k]);
                io->loc_n[gi] = nl;
            }
        }, std::max<int64_t>(steps_all / std::max<int64_t>(m, 1), 1) + step * 8);
        io->ms[1] += since(t_cuts);
        std::vector<int64_t> reps(io->replicates + i0, io->replicates + i1);
        HIPCHECK(e, hipMemcpyAsync(ws + o_rep, reps.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_npre, n_pre.data() + i0, (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_nrows, n_rows.data() + i0, (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_cut, cuts.data(), (size_t)(m * step) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_last, last.data(), (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        const int rc = tau_timed(e, io->ms, me + "replay kernel failed: ", [&]() -> int {
            for (const Group &g : groups) {
                VgxTtlLaunch a{};
                a.m = m;
                a.pre = (const int64_t *)(qws + q_pre);
                a.mev = (const int64_t *)e->t_mev.p; a.mev_cap = mev_cap;
                a.rep = (const int64_t *)(ws + o_rep); a.n_pre = (const int32_t *)(ws + o_npre); a.n_rows = (const int32_t *)(ws + o_nrows);
                a.last = (const int32_t *)(ws + o_last); a.cut = (const int32_t *)(ws + o_cut);
                a.step = (int)step; a.semantics = (int)io->semantics;
                a.ni = (int)g.ni; a.ns = (int)g.ns; a.i0 = (int)g.i0; a.s0 = (int)g.s0; a.n_inf = (int)n_inf; a.n_sus = (int)n_sus;
                a.tsize = vgx_tl_table_size((int)(g.ni + g.ns));
                a.tab = (const int32_t *)(qws + q_tab) + g.tab_off;
                a.start = (const int64_t *)(qws + q_start) + g.start_off;
                a.inf = (double *)(ws + o_inf); a.smp = (double *)(ws + o_smp); a.sus = (double *)(ws + o_sus);
                HIPCHECK(e, launch_replay(&a, e->stream));
                io->passes += 1;
            }
            return VGX_OK;
        });
        if (rc) return rc;
        if (n_inf > 0) {
            HIPCHECK(e, hipMemcpy(io->inf_data + i0 * n_inf * T, ws + o_inf, (size_t)(m * n_inf * T) * 8, hipMemcpyDeviceToHost));
            HIPCHECK(e, hipMemcpy(io->inf_sample + i0 * n_inf * T, ws + o_smp, (size_t)(m * n_inf * T) * 8, hipMemcpyDeviceToHost));
        }
        if (n_sus > 0) HIPCHECK(e, hipMemcpy(io->sus_data + i0 * n_sus * T, ws + o_sus, (size_t)(m * n_sus * T) * 8, hipMemcpyDeviceToHost));
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, cut search, classification, bins and table on a chain given as arrays (no device,
// no engine).  The chain's trailing MULTITYPE events play the replicate's own steps, everything before them the prefix.
extern "C" int vgx_test_tau_timelines(vgx_tau_timelines_chain *tio, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_timelines: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!tio || !tio->chain.time_points) return fail_("null argument");
    vgx_timelines_chain *io = &tio->chain;
    const int64_t n = io->ev_ptr, step = io->step_num, ni = io->n_inf, ns = io->n_sus, T = step + 1;
    if (step < 1 || step >= ((int64_t)1 << 24)) return fail_("step_num must be at least 1");
    if (io->semantics != VGX_TL_REFERENCE && io->semantics != VGX_TL_COMPARTMENT) return fail_("unknown semantics");
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail_("chain too long");
    if (ni < 0 || ns < 0 || ni + ns >= ((int64_t)1 << 20)) return fail_("bad query count");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail_("null event column");
    if ((ni > 0 && (!io->inf_pop || !io->inf_hap || !io->inf_start || !io->inf_data || !io->inf_sample)) ||
        (ns > 0 && (!io->sus_pop || !io->sus_grp || !io->sus_start || !io->sus_data)))
        return fail_("null query or output array");
    if (tio->mev_rows < 0 || (tio->mev_rows > 0 && (!tio->mev_num || !tio->mev_types || !tio->mev_haplotypes || !tio->mev_populations ||
                                                    !tio->mev_newHaplotypes || !tio->mev_newPopulations)))
        return fail_("null multievent column");
    const int ts = vgx_tl_table_size((int)(ni + ns));
    std::vector<int32_t> tab((size_t)(3 * ts), -1);
    for (int64_t k = 0; k < ni; k++) {
        if (io->inf_pop[k] < 0 || io->inf_pop[k] >= io->popNum) return fail_("population index out of range");
        if (io->inf_hap[k] < 0 || io->inf_hap[k] >= io->hapNum) return fail_("haplotype index out of range");
        if (!vgx_tl_insert(tab.data(), ts, 0, (int32_t)io->inf_pop[k], (int32_t)io->inf_hap[k], (int32_t)k)) return fail_("an infectious query is given twice");
    }
    for (int64_t k = 0; k < ns; k++) {
        if (io->sus_pop[k] < 0 || io->sus_pop[k] >= io->popNum) return fail_("population index out of range");
        if (io->sus_grp[k] < 0 || io->sus_grp[k] >= io->susNum) return fail_("susceptibility group index out of range");
        if (!vgx_tl_insert(tab.data(), ts, 1, (int32_t)io->sus_pop[k], (int32_t)io->sus_grp[k], (int32_t)(2 * ni + k))) return fail_("a susceptible query is given twice");
    }
    const EventCols ev{n, io->ev_times, io->ev_types, io->ev_haplotypes, io->ev_populations, io->ev_newHaplotypes, io->ev_newPopulations};
    const RowCols mv{tio->mev_rows, tio->mev_num, tio->mev_types, tio->mev_haplotypes, tio->mev_populations, tio->mev_newHaplotypes, tio->mev_newPopulations};
    FlatChain f;
    const std::string why = flatten(ev, n, mv, f);
    if (!why.empty()) return fail_(why);
    int64_t n_pre_ev = n;
    while (n_pre_ev > 0 && io->ev_types[n_pre_ev - 1] == VGX_TL_MULTITYPE) n_pre_ev--;
    const int64_t n_rows = f.n_rows(), pre_rows = f.ev_row[(size_t)n_pre_ev];
    vgx_tl_time_points(io->currentTime, step, io->time_points);
    std::vector<int32_t> cut((size_t)step);
    const int64_t last = vgx_tl_row_cuts(io->time_points, step, n_pre_ev, f.ev_max.data(), f.ev_row.data(), n - n_pre_ev,
                                         [&](int64_t k) { return io->ev_times[n_pre_ev + k]; },
                                         [&](int64_t k) { return f.ev_row[(size_t)(n_pre_ev + k)] - pre_rows; }, pre_rows, n_rows, cut.data());
    io->last_point = last;
    const int64_t rows = 2 * ni + ns;
    std::vector<int64_t> cnt((size_t)((2 + rows) * T), 0);
    int64_t *g_ds = cnt.data(), *g_s = g_ds + T, *cn = g_s + T;
    int bin = 0;
    for (int64_t e = 0; e < n_rows; e++) {
        bin = vgx_tl_bin(cut.data(), (int)step, (int32_t)e, bin);
        const int64_t *v = f.rows.data() + e * 6;
        const int rule = (v[1] & VGX_TL_ROW_DIRECT) ? VGX_TL_RULE_DIRECT : VGX_TL_RULE_MULTIEVENT;
        const int32_t c[5] = {(int32_t)(v[1] & ~(int64_t)VGX_TL_ROW_DIRECT), (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5]};
        VgxTlMoves m;
        const int64_t w = vgx_tl_classify_row((int)io->semantics, rule, v[0], c, m);
        if (m.all_ds) g_ds[bin] += w;
        if (m.all_s) g_s[bin] += w;
        for (int k = 0; k < 2; k++) {
            const VgxTlOp &o = m.op[k];
            if (o.side < 0) continue;
            const int32_t row = vgx_tl_find(tab.data(), ts, o.side, o.major, o.minor);
            if (row < 0) continue;
            cn[row * T + bin] += o.delta < 0 ? -w : w;
            if (o.sample) cn[(row + ni) * T + bin] += w;
        }
    }
    const bool reference = io->semantics == VGX_TL_REFERENCE;
    for (int64_t r = 0; r < rows; r++) {
        int64_t acc = r < ni ? io->inf_start[r] : r < 2 * ni ? 0 : io->sus_start[r - 2 * ni];
        double *dst = r < ni ? io->inf_data + r * T : r < 2 * ni ? io->inf_sample + (r - ni) * T : io->sus_data + (r - 2 * ni) * T;
        for (int64_t c = 0; c < T; c++) {
            if (c <= last) {
                acc += cn[r * T + c];
                if (reference && r < ni) acc -= g_ds[c];
                if (reference && r >= ni && r < 2 * ni) acc += g_s[c];
                dst[c] = (double)acc;
            } else {
                dst[c] = reference ? 0.0 : (double)acc;
            }
        }
    }
    return VGX_OK;
}
