// vgx_tau_tree_shapes.hip — balance, depth and branch statistics of the sampled tree of every selected replicate of a TAU ensemble
// (vgx_get_tau_tree_shapes), with the node times formed on the device; the node-time kernel, the host side of the call and the two
// test hooks (vgx_test_tau_node_times, vgx_test_tau_node_times_device).  DESIGN.md §30.  Per pass, on one stream:
//   1. the canonicalise kernel of vgx_tau_genealogies.hip brings every own step's rows into the reference's order and granularity;
//   2. its report sizes the walk's table and arena (the one host step inside a pass);
//   3. the walk kernel of vgx_tau_genealogies.hip as it is: tree, node event indices, result and generator words stay on the device;
//   4. the node-time kernel here: one workgroup of 256 threads per tree strides over its nodes and writes
//      times[k] = vgx_tts_time_of(node_ev[k], ...) (vgx_tau_tree_shape.h): consecutive lanes read consecutive 4-byte indices and
//      write consecutive 8-byte times; the table reads (the shared prefix times, the tree's own step times) are gathers into small
//      tables that stay in the L2.  The lowest node whose index lies outside the chain is reduced over the workgroup (shuffles inside
//      a wavefront, four LDS words across them) and thread 0 writes it, or INT32_MAX, to bad[tree]: every cell is written by its own
//      workgroup with a plain store, no atomics, no initialisation from the host;
//   5. the shape kernel of vgx_tree_shapes.hip as it is.
// Nothing of a tree comes to the host: the [n][12] and [n][7] rows, status, generator words and bad[] do.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_tau_lineages.h"     // vgxi_tg_canon, vgxi_tg_count, vgxi_tg_walk
#include "vgx_tau_chain.h"
#include "vgx_tau_tree_shape.h"

namespace {

__global__ void __launch_bounds__(256) vgxtts_times_kernel(VgxTtsLaunch a) {
    __shared__ int32_t s_bad[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = (int64_t)blockIdx.x;
    const VgxTtsDesc d = a.desc[t];
    int32_t bad = INT32_MAX;
    if (!a.res || a.res[t * 5] == 0) {   // (the whole workgroup)
        const int32_t *ev = a.node_ev + d.node_off;
        const double *step_time = a.step_time + d.step_off;
        double *times = a.times + d.node_off;
        for (int64_t k = tid; k < d.nodes; k += 256) {
            bool ok = true;
            times[k] = vgx_tts_time_of(ev[k], d.n_pre, a.pre_time, d.n_steps, step_time, &ok);
            if (!ok && k < bad) bad = (int32_t)k;   // (ascending k: the thread's first)
        }
    }
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) {
        const int32_t o = __shfl_xor(bad, dd);
        bad = o < bad ? o : bad;
    }
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) bad = s_bad[w] < bad ? s_bad[w] : bad;
        a.bad[t] = bad;
    }
}

using namespace vgxtc;

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tts_times(const VgxTtsLaunch *a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxtts_times_kernel, dim3((unsigned)a->n), dim3(256), 0, s, *a);
    return hipGetLastError();
}

extern "C" int vgx_get_tau_tree_shapes(vgx_engine *e, vgx_tau_tree_shapes_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->stats || !io->lengths || !io->status || !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_tree_shapes: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    io->kernel_ms[0] = io->kernel_ms[1] = io->kernel_ms[2] = io->kernel_ms[3] = 0.0;
    // preconditions and refusals: those of vgx_get_tau_genealogies
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (walks tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, PH = P * H, mev_cap = e->tau_mev_cap;
    const int64_t pre_ev = prefix ? prefix->ev_ptr : 0;
    if (pre_ev < 0 || pre_ev >= ((int64_t)1 << 30) ||
        (pre_ev > 0 && (!prefix->ev_times || !prefix->ev_types || !prefix->ev_haplotypes || !prefix->ev_populations || !prefix->ev_newHaplotypes ||
                        !prefix->ev_newPopulations)))
        return fail(e, VGX_ERR_ARG, me + "null prefix column");
    std::vector<char> with_prefix((size_t)n, 0);
    std::vector<int64_t> sC((size_t)n), raw((size_t)n), steps((size_t)n);
    bool any_prefix = false;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : e->ev_ptr0;
            if (s.restarts == 0 && first != pre_ev)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain continues a log of " + std::to_string(first) +
                                                " events, the prefix holds " + std::to_string(pre_ev));
            with_prefix[(size_t)i] = s.restarts == 0 && pre_ev > 0;
            any_prefix = any_prefix || with_prefix[(size_t)i];
            const auto &lg = e->tau_log[(size_t)r];
            for (size_t k = 0; k < lg.size(); k++)
                if (lg[k].m0 != (k ? lg[k - 1].m1 : 0) || lg[k].m1 < lg[k].m0)
                    return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": row ranges of its steps are not contiguous");
            const int64_t rows = lg.empty() ? 0 : lg.back().m1;
            if (rows > mev_cap) return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " logged more rows than its block holds");
            if (rows >= ((int64_t)1 << 30) || (int64_t)lg.size() >= ((int64_t)1 << 30) || 2 * s.sCounter > ((int64_t)1 << 31))
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": chain too long");
            sC[(size_t)i] = s.sCounter;
            raw[(size_t)i] = rows;
            steps[(size_t)i] = (int64_t)lg.size();
        }
    }
    FlatChain pre;
    pre.off.assign(1, 0);
    FlatCaps pre_caps;
    if (any_prefix) {
        const EventCols ev{pre_ev, prefix->ev_times, prefix->ev_types, prefix->ev_haplotypes, prefix->ev_populations, prefix->ev_newHaplotypes, prefix->ev_newPopulations};
        const RowCols mv{prefix->mev_rows, prefix->mev_num, prefix->mev_times, prefix->mev_types, prefix->mev_haplotypes, prefix->mev_populations,
                         prefix->mev_newHaplotypes, prefix->mev_newPopulations};
        if (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np)) return fail(e, VGX_ERR_ARG, me + "null prefix multievent column");
        const std::string why = flatten(ev, pre_ev, mv, P, H, pre);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + "prefix: " + why);
    }
    pre_caps.of(pre);
    const int64_t pre_rows = (int64_t)pre.rows.size(), pre_times = (int64_t)pre.time.size();   // (pre_times: pre_ev with a prefix in use, else 0)
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    typedef std::unique_ptr<char, void (*)(char *)> Hold;
    hipError_t er;

    // what stays for the whole call: [rep | raw rows | sCounter | row sums | prefix rows | prefix offsets | prefix times]
    const int64_t o_rep = 0, o_raw = o_rep + up8(n * 8), o_sc = o_raw + up8(n * 8), o_cnt = o_sc + up8(n * 8), o_prow = o_cnt + up8(n * 24),
                  o_poff = o_prow + up8(pre_rows * 32 + 32), o_ptime = o_poff + up8((int64_t)pre.off.size() * 4), keep_total = o_ptime + up8(pre_times * 8 + 8);
    char *kws = nullptr;
    if ((er = hipMalloc((void **)&kws, (size_t)keep_total)) != hipSuccess)
        return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    Hold khold(kws, dev_free);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_raw, raw.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_sc, sC.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    if (pre_rows) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 32, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_poff, pre.off.data(), pre.off.size() * 4, hipMemcpyHostToDevice, e->stream));
    if (pre_times) HIPCHECK(e, hipMemcpyAsync(kws + o_ptime, pre.time.data(), (size_t)pre_times * 8, hipMemcpyHostToDevice, e->stream));
    // raw sums of min(num, sCounter): MUTATION rows, MIGRATION rows, rows that can push a lineage: the record capacities of the
    // sizing branch of vgx_get_tau_genealogies and the bound of a pass's workspace
    std::vector<int64_t> cnt((size_t)n * 3);
    HIPCHECK(e, vgxi_tg_count((const int64_t *)e->t_mev.p, mev_cap, (const int64_t *)(kws + o_rep), (const int64_t *)(kws + o_raw),
                              (const int64_t *)(kws + o_sc), n, (int64_t *)(kws + o_cnt), e->stream));
    HIPCHECK(e, hipMemcpyAsync(cnt.data(), kws + o_cnt, (size_t)n * 24, hipMemcpyDeviceToHost, e->stream));
    if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));
    auto nodes_of = [&](int64_t i) { return sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0; };
    auto mut_need = [&](int64_t i) {
        if (sC[(size_t)i] < 2) return (int64_t)0;
        return cnt[(size_t)(3 * i)] + (with_prefix[(size_t)i] ? pre_caps.direct_mut + pre_caps.mut(sC[(size_t)i]) : 0);
    };
    auto mig_need = [&](int64_t i) {
        if (sC[(size_t)i] < 2) return (int64_t)0;
        return cnt[(size_t)(3 * i + 1)] + (with_prefix[(size_t)i] ? pre_caps.direct_mig + pre_caps.mig(sC[(size_t)i]) : 0) + nodes_of(i);
    };

    // passes: what a replicate can need at most, from its raw rows (vgx_get_tau_genealogies' sum, the node times, the accumulators
    // and the step times added)
    auto table_of = [&](int64_t rows) { return vgx_gw_table_size(rows, PH); };
    auto arena_of = [&](int64_t i, int64_t tsize, int64_t pushes) {
        const int64_t all = pushes + (with_prefix[(size_t)i] ? pre_caps.direct_push + pre_caps.push(sC[(size_t)i]) : 0);
        return std::min(all, (tsize / 2) * sC[(size_t)i]);
    };
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t rows = raw[(size_t)i] + (with_prefix[(size_t)i] ? pre_rows : 0), nodes = nodes_of(i);
        const int64_t tsize = nodes ? table_of(rows) : 0;
        bytes[(size_t)i] = raw[(size_t)i] * 32 + (steps[(size_t)i] + 1) * 8 + tsize * 28 + (nodes ? arena_of(i, tsize, cnt[(size_t)(3 * i + 2)]) : 0) * 4 +
                           nodes * (16 + 8 + VGX_TS_NODE_BYTES) + mut_need(i) * 20 + mig_need(i) * 16 + steps[(size_t)i] * 8 +
                           (int64_t)(sizeof(VgxGtDesc) + sizeof(VgxGtCanonDesc) + sizeof(VgxGtCanonStat) + sizeof(VgxTsDesc) + sizeof(VgxTtsDesc)) +
                           8 * (VGX_TS_K + VGX_TS_L + 2) + 2048;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // the three kernels behind the canonicalise kernel, timed apart
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        // ---- canonicalise: [desc | stat | step ranges | canonical row ranges | canonical rows]; the pass's step times beside them
        auto t_host = std::chrono::steady_clock::now();
        std::vector<VgxGtCanonDesc> cd((size_t)m);
        std::vector<int32_t> mrange;
        std::vector<double> step_time;
        std::vector<int64_t> step_off((size_t)m);
        int64_t RO = 0, OO = 0, longest = 0;
        for (int64_t j = 0; j < m; j++) {
            const int64_t gi = i0 + j;
            const auto &lg = e->tau_log[(size_t)io->replicates[gi]];
            VgxGtCanonDesc &d = cd[(size_t)j];
            d.rep = io->replicates[gi]; d.n_steps = (int64_t)lg.size(); d.sCounter = sC[(size_t)gi];
            d.step_off = (int64_t)mrange.size(); d.row_off = RO; d.off_off = OO;
            step_off[(size_t)j] = (int64_t)step_time.size();
            for (const auto &st : lg) {
                mrange.push_back((int32_t)st.m0);
                step_time.push_back(st.time);
                longest = std::max(longest, std::min<int64_t>(st.m1 - st.m0, VGX_GT_STEP_ROWS_MAX));
            }
            mrange.push_back((int32_t)raw[(size_t)gi]);
            RO += raw[(size_t)gi];
            OO += d.n_steps + 1;
        }
        io->ms[1] += since(t_host);
        const int64_t S = (int64_t)step_time.size();
        const int64_t c_desc = 0, c_stat = c_desc + up8(m * (int64_t)sizeof(VgxGtCanonDesc)), c_mr = c_stat + up8(m * (int64_t)sizeof(VgxGtCanonStat)),
                      c_off = c_mr + up8((int64_t)mrange.size() * 4), c_rows = c_off + up8(OO * 4), c_st = c_rows + up8(RO * 32 + 32),
                      c_total = c_st + up8(S * 8 + 8);
        char *cws = nullptr;
        if ((er = hipMalloc((void **)&cws, (size_t)c_total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(c_total) + " bytes: " + hipGetErrorString(er));
        Hold chold(cws, dev_free);
        VgxGtCanonLaunch ca{};
        ca.n = m;
        ca.desc = (const VgxGtCanonDesc *)(cws + c_desc);
        ca.mev = (const int64_t *)e->t_mev.p; ca.mev_cap = mev_cap;
        ca.mrange = (const int32_t *)(cws + c_mr);
        ca.P = P; ca.H = H; ca.sites = e->d.sites;
        ca.cap = 64;
        while (ca.cap < longest) ca.cap <<= 1;
        ca.can = (VgxGtRow *)(cws + c_rows); ca.can_off = (int32_t *)(cws + c_off); ca.stat = (VgxGtCanonStat *)(cws + c_stat);
        HIPCHECK(e, hipMemcpyAsync(cws + c_desc, cd.data(), (size_t)m * sizeof(VgxGtCanonDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_mr, mrange.data(), mrange.size() * 4, hipMemcpyHostToDevice, e->stream));
        if (S) HIPCHECK(e, hipMemcpyAsync(cws + c_st, step_time.data(), (size_t)S * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_tg_canon(&ca, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // the sizes of the walk's workspace come from its report
            return fail(e, VGX_ERR_HIP, me + "canonicalise kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->kernel_ms[0] += kms;
        io->ms[0] += kms;
        std::vector<VgxGtCanonStat> stat((size_t)m);
        HIPCHECK(e, hipMemcpy(stat.data(), ca.stat, (size_t)m * sizeof(VgxGtCanonStat), hipMemcpyDeviceToHost));

        // ---- walk, node times, shape: the walk's [desc | res | rng | key | cnt | base | len | lcap | arena | fresh | node x3 | mut x5 | mig x4],
        // then [tree descs | time descs | node times | A, B | seven int32 accumulators | stats | lengths | status | bad]
        t_host = std::chrono::steady_clock::now();
        std::vector<VgxGtDesc> dp((size_t)m);
        std::vector<VgxTsDesc> ts((size_t)m);
        std::vector<VgxTtsDesc> tt((size_t)m);
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        for (int64_t j = 0; j < m; j++) {
            const int64_t gi = i0 + j;
            VgxGtDesc &d = dp[(size_t)j];
            const VgxGtCanonStat &st = stat[(size_t)j];
            d.rep = io->replicates[gi];
            d.n_pre = with_prefix[(size_t)gi] ? pre_ev : 0;
            d.n_steps = cd[(size_t)j].n_steps;
            d.sCounter = sC[(size_t)gi];
            d.status = st.status; d.arg = st.arg;
            const bool walk = d.sCounter >= 2 && st.status == VGX_GW_OK;
            d.tsize = walk ? table_of(st.n_rows + (with_prefix[(size_t)gi] ? pre_rows : 0)) : 0;
            d.arena_cap = walk ? arena_of(gi, d.tsize, st.pushes) : 0;
            d.mut_cap = mut_need(gi);
            d.mig_cap = mig_need(gi);
            d.row_off = cd[(size_t)j].row_off; d.off_off = cd[(size_t)j].off_off;
            for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[gi * 6 + k];
            d.has32 = io->rng_state[gi * 6 + 4] != 0; d.spare = (int64_t)(uint32_t)io->rng_state[gi * 6 + 5];
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            ts[(size_t)j] = VgxTsDesc{N, nodes_of(gi)};
            tt[(size_t)j] = VgxTtsDesc{N, nodes_of(gi), d.n_pre, step_off[(size_t)j], d.n_steps};
            T += d.tsize; A += d.arena_cap; N += nodes_of(gi); M += d.mut_cap; G += d.mig_cap;
        }
        io->ms[1] += since(t_host);
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGtDesc)), o_rng = o_res + up8(m * 40), o_key = o_rng + up8(m * 48),
                      o_cnt2 = o_key + up8(T * 8), o_base = o_cnt2 + up8(T * 8), o_len = o_base + up8(T * 4), o_lcap = o_len + up8(T * 4),
                      o_arena = o_lcap + up8(T * 4), o_fresh = o_arena + up8(A * 4), o_out = o_fresh + up8(N * 4),
                      o_ts = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_tt = o_ts + up8(m * (int64_t)sizeof(VgxTsDesc)),
                      o_times = o_tt + up8(m * (int64_t)sizeof(VgxTtsDesc)), o_w64 = o_times + up8(N * 8), o_w32 = o_w64 + up8(2 * N * 8),
                      o_stats = o_w32 + up8(7 * N * 4), o_lens = o_stats + up8(m * VGX_TS_K * 8), o_status = o_lens + up8(m * VGX_TS_L * 8),
                      o_bad = o_status + up8(m * 16), total = o_bad + up8(m * 4);
        char *ws = nullptr;
        if ((er = hipMalloc((void **)&ws, (size_t)total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        Hold hold(ws, dev_free);
        VgxGtLaunch a{};
        a.n = m;
        a.desc = (const VgxGtDesc *)(ws + o_desc);
        a.pre = (const VgxGtRow *)(kws + o_prow); a.pre_off = (const int32_t *)(kws + o_poff);
        a.can = ca.can; a.can_off = ca.can_off;
        a.I = (const int32_t *)e->t_I.p;
        a.P = P; a.H = H;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt2);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena); a.fresh = (int32_t *)(ws + o_fresh);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        VgxTtsLaunch b{};
        b.n = m;
        b.desc = (const VgxTtsDesc *)(ws + o_tt);
        b.res = a.res;
        b.node_ev = a.node_ev;
        b.pre_time = (const double *)(kws + o_ptime); b.step_time = (const double *)(cws + c_st);
        b.times = (double *)(ws + o_times);
        b.bad = (int32_t *)(ws + o_bad);
        VgxTsLaunch c{};
        c.n = m;
        c.desc = (const VgxTsDesc *)(ws + o_ts);
        c.res = a.res;
        c.tree = a.tree; c.node_ev = a.node_ev; c.times = b.times;
        int32_t *w32 = (int32_t *)(ws + o_w32);
        int64_t *w64 = (int64_t *)(ws + o_w64);
        c.w = VgxTsWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N, w32 + 4 * N, w32 + 5 * N, w32 + 6 * N, w64, w64 + N};
        c.stats = (int64_t *)(ws + o_stats); c.lengths = (double *)(ws + o_lens); c.status = (int64_t *)(ws + o_status);
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGtDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_ts, ts.data(), (size_t)m * sizeof(VgxTsDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_tt, tt.data(), (size_t)m * sizeof(VgxTtsDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        // walk, node times and shape with no host step between them
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_tg_walk(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        HIPCHECK(e, vgxi_tts_times(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        HIPCHECK(e, vgxi_ts_shape(&c, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[3], e->stream));
        std::vector<int64_t> st2((size_t)m * 2);
        std::vector<int32_t> bad((size_t)m);
        HIPCHECK(e, hipMemcpyAsync(io->stats + i0 * VGX_TS_K, c.stats, (size_t)m * VGX_TS_K * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->lengths + i0 * VGX_TS_L, c.lengths, (size_t)m * VGX_TS_L * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(st2.data(), c.status, (size_t)m * 16, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(bad.data(), b.bad, (size_t)m * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 6, a.rng_out, (size_t)m * 48, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // before anything reads the rows
            return fail(e, VGX_ERR_HIP, me + "walk, node-time or shape kernel failed: " + hipGetErrorString(er));
        for (int k = 0; k < 3; k++) {
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->kernel_ms[k + 1] += kms;
            io->ms[0] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            if (bad[(size_t)j] != INT32_MAX) return fail(e, VGX_ERR_ARG, me + "an event index outside the chain");
            io->status[i0 + j] = st2[(size_t)(2 * j)];
            io->status_arg[i0 + j] = st2[(size_t)(2 * j + 1)];
        }
        io->passes += 1;
        i0 = i1;
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- test hooks: the rule on the host, and given trees through the kernel (no engine) ---------------------------------------------
extern "C" int vgx_test_tau_node_times(const int32_t *node_ev, int64_t nodes, int64_t n_pre, const double *pre_times, int64_t n_steps,
                                       const double *step_times, double *times, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    const std::string me = "vgx_test_tau_node_times: ";
    if (nodes < 0 || n_pre < 0 || n_steps < 0 || (nodes > 0 && (!node_ev || !times)) || (n_pre > 0 && !pre_times) || (n_steps > 0 && !step_times))
        return fail_(me + "null argument");
    for (int64_t k = 0; k < nodes; k++) {
        bool ok = true;
        times[k] = vgx_tts_time_of(node_ev[k], n_pre, pre_times, n_steps, step_times, &ok);
        if (!ok)
            return fail_(me + "node " + std::to_string(k) + ": event index " + std::to_string(node_ev[k]) + " outside the chain of " +
                         std::to_string(n_pre + n_steps) + " events");
    }
    return VGX_OK;
}

extern "C" int vgx_test_tau_node_times_device(int64_t n, const int64_t *node_off, const int32_t *node_ev, const int64_t *n_pre, int64_t n_pre_times,
                                              const double *pre_times, const int64_t *step_off, const double *step_times, double *times, int32_t *bad,
                                              char *errbuf, int64_t errcap) {
    auto fail_ = [&](int code, const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return code;
    };
    const std::string me = "vgx_test_tau_node_times_device: ";
    if (n < 0 || n_pre_times < 0 || (n > 0 && (!node_off || !n_pre || !step_off || !bad)) || (n_pre_times > 0 && !pre_times))
        return fail_(VGX_ERR_ARG, me + "null argument");
    if (n == 0) return VGX_OK;
    if (node_off[0] != 0 || step_off[0] != 0) return fail_(VGX_ERR_ARG, me + "node_off[0] and step_off[0] must be 0");
    // every table the kernel indexes is bounded here: the kernel checks an index against these lengths before it loads
    std::vector<VgxTtsDesc> dp((size_t)n);
    for (int64_t t = 0; t < n; t++) {
        const int64_t N = node_off[t + 1] - node_off[t], S = step_off[t + 1] - step_off[t];
        if (N < 0 || N > INT32_MAX) return fail_(VGX_ERR_ARG, me + "node_off must not decrease (a tree holds fewer than 2^31 nodes)");
        if (S < 0) return fail_(VGX_ERR_ARG, me + "step_off must not decrease");
        if (n_pre[t] < 0 || n_pre[t] > n_pre_times)
            return fail_(VGX_ERR_ARG, me + "tree " + std::to_string(t) + ": n_pre = " + std::to_string(n_pre[t]) + " is outside the table of " +
                                          std::to_string(n_pre_times) + " prefix times");
        dp[(size_t)t] = VgxTtsDesc{node_off[t], N, n_pre[t], step_off[t], S};
    }
    const int64_t T = node_off[n], S = step_off[n];
    if ((T > 0 && (!node_ev || !times)) || (S > 0 && !step_times)) return fail_(VGX_ERR_ARG, me + "null argument");
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t o_desc = 0, o_nev = o_desc + up(n * (int64_t)sizeof(VgxTtsDesc)), o_pre = o_nev + up(T * 4), o_st = o_pre + up(n_pre_times * 8 + 8),
                  o_times = o_st + up(S * 8 + 8), o_bad = o_times + up(T * 8), total = o_bad + up(n * 4);
    char *ws = nullptr;
    hipError_t er = hipMalloc((void **)&ws, (size_t)total);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
    VgxTtsLaunch a{};
    a.n = n;
    a.desc = (const VgxTtsDesc *)(ws + o_desc);
    a.res = nullptr;
    a.node_ev = (const int32_t *)(ws + o_nev);
    a.pre_time = (const double *)(ws + o_pre); a.step_time = (const double *)(ws + o_st);
    a.times = (double *)(ws + o_times);
    a.bad = (int32_t *)(ws + o_bad);
    er = hipMemcpy(ws + o_desc, dp.data(), (size_t)n * sizeof(VgxTtsDesc), hipMemcpyHostToDevice);
    if (er == hipSuccess && T) er = hipMemcpy(ws + o_nev, node_ev, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && n_pre_times) er = hipMemcpy(ws + o_pre, pre_times, (size_t)n_pre_times * 8, hipMemcpyHostToDevice);
    if (er == hipSuccess && S) er = hipMemcpy(ws + o_st, step_times, (size_t)S * 8, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = vgxi_tts_times(&a, nullptr);
    if (er == hipSuccess) er = hipStreamSynchronize(nullptr);
    if (er == hipSuccess && T) er = hipMemcpy(times, a.times, (size_t)T * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(bad, a.bad, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + hipGetErrorString(er));
    return VGX_OK;
}
