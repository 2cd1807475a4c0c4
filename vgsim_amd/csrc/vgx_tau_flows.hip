// vgx_tau_flows.hip — new infections per time bin, source population, destination population and variant class of every selected
// replicate of a TAU ensemble on the device (vgx_get_tau_flows), the host side of that call, and the same rule and tile walk
// compiled for the host (vgx_test_tau_flows).  The rule is vgx_tau_flows.h; DESIGN.md §24.
//
// COUNTING kernel.  The geometry and the row loads of vgx_tau_incidence.hip: a workgroup of 256 threads takes one chain (a
// selected replicate's own rows in its block of t_mev, or the flattened prefix) and a TILE of consecutive rows; consecutive lanes
// read consecutive rows (three 16-byte loads per lane).  The tile is clipped to the window [cut[0], cut[T]); its first bin comes
// from a search in the chain's cuts, read where they lie; bin by bin `num` is added with 64-bit LDS atomics to the int64 cells
// the form keeps (vgx_flows.h: all P * P * V, or the P * V of the diagonal, a row off the diagonal then adding num to its cell of
// the bin's block in device memory with one 64-bit atomic), and at every bin change and at the tile's end the nonzero cells go to
// the block in device memory with 64-bit integer atomics and are cleared.  variant_of is staged in LDS behind the cells when it
// fits.  Rows outside the window feed the chain's two `outside` counters: a per-thread sum, a wave sum, one atomic per wavefront.
// All arithmetic is integer: the block does not depend on the form, the tile size, the launch geometry or the chunking.
// The tile size is VGX_FLOWS_TILE_EVENTS (rows here; default 4096, DESIGN.md §16 for why).
// The prefix is counted ONCE per call as a chain of its own; an init kernel then starts the block of every selected replicate
// that did not restart from the prefix block, and the replicates' own rows are added on top.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_tau_flows.h"
#include "vgx_tau_rows.h"   // EventCols, RowCols, FlatChain, flatten

namespace {

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void add64(long long *p, long long v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);   // two's complement: the sum is the signed one
}

template <int FORM>
__global__ void __launch_bounds__(256) vgxtf_count_kernel(VgxTauFlowLaunch a, int stage) {
    extern __shared__ __attribute__((aligned(16))) long long hist[];   // dense: [P][P][V] cells, split: [P][V]; then (stage) variant_of [hapNum]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_rows[row], T = a.T, P = a.P, V = a.V, cells = P * P * V;
    const int32_t kept = FORM == VGX_FLOW_DENSE ? cells : P * V;
    const int32_t *cut = a.cut + row * (int64_t)(T + 1);   // (uniform addresses: every thread reads the same cuts)
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *rows = (const longlong2 *)(a.rows + (a.rep ? a.rep[row] * a.stride * 6 : 0));
    long long *out = (long long *)a.counts + row * (int64_t)T * cells, *outside = (long long *)a.outside + 2 * row;
    const int32_t *vo = a.variant_of;
    long long before = 0, after = 0;       // this thread's share of the rows outside the window
    bool clean = false;                    // the cells are zeroed and the map staged before the first tile that counts
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e0 = (int32_t)t0, e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t b1, a0;
        vgx_tau_inc_outside(cut, T, e0, e1, b1, a0);
        for (int64_t e = (int64_t)e0 + tid; e < b1; e += 256) {   // (only num is needed: the row's first 16 bytes)
            const long long w = rows[e * 3].x;
            if (w > 0) before += w;
        }
        for (int64_t e = (int64_t)a0 + tid; e < e1; e += 256) {
            const long long w = rows[e * 3].x;
            if (w > 0) after += w;
        }
        int32_t pos, hi;
        vgx_inc_clip(cut, T, e0, e1, pos, hi);
        if (pos >= hi) continue;           // (the whole workgroup: nothing of the tile lies inside the window)
        if (!clean) {
            for (int i = tid; i < kept; i += 256) hist[i] = 0;
            if (stage) {
                int32_t *map = (int32_t *)(hist + kept);
                for (int i = tid; i < a.hapNum; i += 256) map[i] = vo[i];
                vo = map;
            }
            clean = true;
            __syncthreads();
        }
        while (pos < hi) {
            const int32_t b = vgx_inc_bin(cut, T, pos);
            const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
            long long *dstb = out + (int64_t)b * cells;
            for (int64_t e = (int64_t)pos + tid; e < end; e += 256) {
                const longlong2 r0 = rows[e * 3], r1 = rows[e * 3 + 1], r2 = rows[e * 3 + 2];
                int32_t src, dst, cls;
                const long long w = vgx_tau_flow_row(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, P, a.hapNum, vo, a.within, src, dst, cls);
                if (!w) continue;
                if (FORM == VGX_FLOW_DENSE) add64(&hist[vgx_flow_index(P, V, src, dst, cls)], w);
                else if (src == dst) add64(&hist[src * V + cls], w);
                else add64(&dstb[vgx_flow_index(P, V, src, dst, cls)], w);
            }
            __syncthreads();
            for (int i = tid; i < kept; i += 256) {
                const long long v = hist[i];
                if (v) { add64(&dstb[FORM == VGX_FLOW_DENSE ? i : vgx_flow_diag_index(P, V, i)], v); hist[i] = 0; }
            }
            __syncthreads();
            pos = end;
        }
    }
    before = wave_sum(before);
    after = wave_sum(after);
    if (lane == 0) {
        if (before) add64(&outside[0], before);
        if (after) add64(&outside[1], after);
    }
}

// the blocks and `outside` counters of m chains start from the prefix's (with[i] != 0) or from zero
__global__ void __launch_bounds__(256) vgxtf_init_kernel(int64_t m, int64_t tc, const int32_t *with, const long long *pre, const long long *pre_out,
                                                         long long *counts, long long *outside) {
    const int64_t total = m * tc, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int64_t c = i / tc;
        counts[i] = with[c] ? pre[i - c * tc] : 0;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 2 * m; i += stride) outside[i] = with[i >> 1] ? pre_out[i & 1] : 0;
}

unsigned flat_grid(int64_t total) { return (unsigned)std::min<int64_t>(std::max<int64_t>((total + 255) / 256, 1), 1 << 16); }

template <int FORM>
hipError_t launch(const VgxTauFlowLaunch *a, hipStream_t s) {
    const bool stage = vgx_tau_flow_stage_map(FORM, a->P, a->V, a->hapNum);
    const int64_t lds = vgx_tau_flow_lds_bytes(FORM, a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxtf_count_kernel<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtf_count_kernel<FORM>, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

// what both the call and the hook check about the grid, the map and the form; "" or why not.  `ran` gets the form that runs.
std::string check_request(const double *edges, int64_t T, int64_t V, const int32_t *variant_of, int64_t P, int64_t H, int asked, int &ran) {
    if (T < 1 || T >= VGX_FLOW_MAX_BINS || !edges) return "T = " + std::to_string(T) + " bins: at least 1, below 2^24, with edges";
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(edges[k])) return "edges[" + std::to_string(k) + "] is not finite";
        if (k > 0 && !(edges[k - 1] < edges[k])) return "edges must increase strictly (edges[" + std::to_string(k) + "])";
    }
    if (V < 1 || V > INT32_MAX || !variant_of) return "V = " + std::to_string(V) + " classes: at least 1, with variant_of";
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")";
    ran = vgx_tau_flow_form(asked, P, V);
    if (!ran) {
        char why[256];
        vgx_tau_flow_refusal(asked, P, V, why, sizeof why);
        return why;
    }
    return "";
}

// The prefix as a chain of its own: its cuts (the literal loop over its events, then its row count) and where the loop stands
// after it.  cut: [T + 1].
int64_t prefix_cuts(const FlatChain &f, int64_t n_ev, const double *times, const double *edges, int64_t T, int32_t *cut) {
    VgxIncCutter ct{edges, T, cut};
    for (int64_t i = 0; i < n_ev; i++) ct.event(f.ev_row[(size_t)i], times[i]);
    const int64_t point0 = ct.point;
    ct.finish(f.ev_row[(size_t)n_ev]);
    return point0;
}

// A chain's own events after a prefix that left the loop at point0: cuts relative to the chain's first own row
template <class OwnTime, class OwnRow>
void own_cuts(const double *edges, int64_t T, int64_t point0, int64_t n_own, OwnTime own_time, OwnRow own_m0, int64_t n_rows, int32_t *cut) {
    for (int64_t k = 0; k < point0; k++) cut[k] = 0;   // these cuts lie inside the prefix: before the first own row
    VgxIncCutter ct{edges, T, cut};
    ct.point = point0;
    for (int64_t k = 0; k < n_own; k++) ct.event(own_m0(k), own_time(k));
    ct.finish(n_rows);
}

}  // namespace

extern "C" hipError_t vgxi_tau_flow_count(const VgxTauFlowLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if ((a->form != VGX_FLOW_DENSE && a->form != VGX_FLOW_SPLIT) || vgx_tau_flow_form(a->form, a->P, a->V) != a->form || a->tile < 1)
        return hipErrorInvalidValue;
    return a->form == VGX_FLOW_DENSE ? launch<VGX_FLOW_DENSE>(a, s) : launch<VGX_FLOW_SPLIT>(a, s);
}

extern "C" hipError_t vgxi_tau_flow_init(int64_t m, int64_t tc, const int32_t *with, const int64_t *pre, const int64_t *pre_out, int64_t *counts,
                                         int64_t *outside, hipStream_t s) {
    hipLaunchKernelGGL(vgxtf_init_kernel, dim3(flat_grid(m * tc)), dim3(256), 0, s, m, tc, with, (const long long *)pre, (const long long *)pre_out,
                       (long long *)counts, (long long *)outside);
    return hipGetLastError();
}

// vgx_get_tau_incidence step for step, with the block [n][T][P][P][V], vgx_get_flows's variant_of, `within` and form in place of
// the mask.
extern "C" int vgx_get_tau_flows(vgx_engine *e, vgx_tau_flows_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_flows: ";
    io->passes = 0;
    io->form = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (counts tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V, mev_cap = e->tau_mev_cap;
    int asked = VGX_FLOW_AUTO, form = 0;
    if (const char *fm = getenv("VGX_FLOWS_FORM")) {
        if (!strcmp(fm, "dense")) asked = VGX_FLOW_DENSE;
        else if (!strcmp(fm, "split")) asked = VGX_FLOW_SPLIT;
        else if (*fm) return fail(e, VGX_ERR_ARG, me + "VGX_FLOWS_FORM=" + fm + " is neither dense nor split");
    }
    {
        const std::string why = check_request(io->edges, T, V, io->variant_of, P, H, asked, form);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + why);
    }
    io->form = form;
    const int64_t cells = P * P * V, tc = T * cells;   // (P * V <= 2^13 and P <= 2^13: cells below 2^26)
    // the prefix: what the model held when the call started
    const int64_t pre_ev = prefix ? prefix->ev_ptr : 0;
    if (pre_ev < 0 || (pre_ev > 0 && (!prefix->ev_times || !prefix->ev_types || !prefix->ev_haplotypes || !prefix->ev_populations ||
                                      !prefix->ev_newHaplotypes || !prefix->ev_newPopulations)))
        return fail(e, VGX_ERR_ARG, me + "null prefix column");
    std::vector<int32_t> n_own((size_t)n), with_prefix((size_t)n, 0);
    bool any_prefix = false;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : e->ev_ptr0;   // vgx_counters.ev_first_new
            if (s.restarts == 0 && first != pre_ev)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain continues a log of " + std::to_string(first) +
                                                " events, the prefix holds " + std::to_string(pre_ev));
            with_prefix[(size_t)i] = s.restarts == 0 && pre_ev > 0;
            any_prefix = any_prefix || with_prefix[(size_t)i];
            const auto &lg = e->tau_log[(size_t)r];
            for (size_t k = 0; k < lg.size(); k++)   // the steps' row ranges tile the replicate's block
                if (lg[k].m0 != (k ? lg[k - 1].m1 : 0) || lg[k].m1 < lg[k].m0)
                    return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": row ranges of its steps are not contiguous");
            if (!lg.empty() && lg.back().m1 > mev_cap) return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " logged more rows than its block holds");
        }
    }
    FlatChain pre;
    pre.ev_row.assign(1, 0);
    if (any_prefix) {
        const EventCols ev{pre_ev, prefix->ev_times, prefix->ev_types, prefix->ev_haplotypes, prefix->ev_populations, prefix->ev_newHaplotypes, prefix->ev_newPopulations};
        const RowCols mv{prefix->mev_rows, prefix->mev_num, prefix->mev_types, prefix->mev_haplotypes, prefix->mev_populations, prefix->mev_newHaplotypes,
                         prefix->mev_newPopulations};
        if (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np)) return fail(e, VGX_ERR_ARG, me + "null prefix multievent column");
        const std::string why = flatten(ev, pre_ev, mv, pre);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + "prefix: " + why);
    }
    const int64_t pre_rows = pre.n_rows();
    for (int64_t i = 0; i < n; i++) {
        const auto &lg = e->tau_log[(size_t)io->replicates[i]];
        const int64_t own = lg.empty() ? 0 : lg.back().m1, total = (with_prefix[(size_t)i] ? pre_rows : 0) + own;
        if (total >= ((int64_t)1 << 31))
            return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(io->replicates[i]) + ": prefix and own rows reach 2^31 (" + std::to_string(total) + ")");
        n_own[(size_t)i] = (int32_t)own;
    }
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    const std::string dims = std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x " + std::to_string(P) + " x " + std::to_string(V);
    if (tc >= ((int64_t)1 << 40) / n)
        return fail(e, VGX_ERR_ARG, me + "the block of " + dims + " counts holds 2^40 cells or more: select fewer replicates per call");
    int64_t tile = VGX_FLOW_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_FLOWS_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_FLOW_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_own | with | variant_of | prefix: rows, cut, n_rows, block, outside | counts | outside | narrow | min/max]
    const int64_t block_bytes = n * tc * 8, narrow_bytes = io->summary ? n * tc * 4 : 0;
    const int64_t o_rep = 0, o_nown = o_rep + up8(n * 8), o_with = o_nown + up8(n * 4), o_map = o_with + up8(n * 4),
                  o_prow = o_map + up8(H * 4), o_pcut = o_prow + up8(pre_rows * 48 + 8), o_pn = o_pcut + up8((T + 1) * 4),
                  o_pcnt = o_pn + up8(4), o_pout = o_pcnt + up8(tc * 8), o_cnt = o_pout + up8(16), o_out = o_cnt + up8(block_bytes),
                  o_nar = o_out + up8(n * 16), o_mm = o_nar + up8(narrow_bytes + 8), keep_total = o_mm + up8(16);
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + dims + " counts of 8 bytes, the prefix block, the prefix rows and " +
                                        (io->summary ? "the summary's 4-byte copy take " : "their counters take ") + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_with, with_prefix.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_pcnt, 0, (size_t)(o_cnt - o_pcnt), e->stream));   // the prefix block and its outside counters
    auto fill = [&](VgxTauFlowLaunch &a) {
        a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V;
        a.variant_of = (const int32_t *)(kws + o_map);
        a.within = io->within ? 1 : 0; a.form = form; a.tile = (int32_t)tile;
    };

    // the prefix, once: flattened rows uploaded, its cuts, counted as a chain of its own
    int64_t point0 = 0;
    std::vector<int32_t> pcut((size_t)(T + 1), 0);
    const int32_t pn = (int32_t)pre_rows;
    if (any_prefix) {
        const auto t_cuts = std::chrono::steady_clock::now();
        point0 = prefix_cuts(pre, pre_ev, prefix->ev_times, io->edges, T, pcut.data());
        io->ms[1] += since(t_cuts);
        if (pre_rows > 0) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 48, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_pcut, pcut.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_pn, &pn, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        VgxTauFlowLaunch a{};
        fill(a);
        a.m = 1;
        a.rows = (const int64_t *)(kws + o_prow); a.stride = 0; a.rep = nullptr;
        a.n_rows = (const int32_t *)(kws + o_pn); a.cut = (const int32_t *)(kws + o_pcut);
        a.max_n = pre_rows;
        a.counts = (int64_t *)(kws + o_pcnt); a.outside = (int64_t *)(kws + o_pout);
        HIPCHECK(e, vgxi_tau_flow_count(&a, e->stream));
        if (pre_rows > 0) io->passes += 1;
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting kernel failed on the prefix: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
    }

    // chunks of replicates: the cuts of a chunk fit `share` bytes of device memory
    int64_t share = std::min<int64_t>((int64_t)(free_b / 2) - keep_total + 4096, (int64_t)1 << 30);
    if (const char *cb = getenv("VGX_TIMELINES_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    const int64_t per_rep = (T + 1) * 4 + 64;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(share / per_rep, (int64_t)1 << 20));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t i1 = std::min(n, i0 + chunk), m = i1 - i0;
        char *ws = nullptr;
        const int64_t total = up8(m * (T + 1) * 4);
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, dev_free);
        // host: every replicate's cuts in the row index space of its own block (the loop continued where the prefix left it)
        const auto t_cuts = std::chrono::steady_clock::now();
        std::vector<int32_t> cuts((size_t)(m * (T + 1)));
        int64_t steps_all = 0, max_n = 0;
        for (int64_t j = 0; j < m; j++) {
            steps_all += (int64_t)e->tau_log[(size_t)io->replicates[i0 + j]].size();
            max_n = std::max<int64_t>(max_n, n_own[(size_t)(i0 + j)]);
        }
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j;
                const auto &lg = e->tau_log[(size_t)io->replicates[gi]];
                own_cuts(io->edges, T, with_prefix[(size_t)gi] ? point0 : 0, (int64_t)lg.size(), [&](int64_t k) { return lg[(size_t)k].time; },
                         [&](int64_t k) { return lg[(size_t)k].m0; }, n_own[(size_t)gi], cuts.data() + j * (T + 1));
            }
        }, std::max<int64_t>(steps_all / std::max<int64_t>(m, 1), 1) + T);
        io->ms[1] += since(t_cuts);
        HIPCHECK(e, hipMemcpyAsync(ws, cuts.data(), (size_t)(m * (T + 1)) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_tau_flow_init(m, tc, (const int32_t *)(kws + o_with) + i0, (const int64_t *)(kws + o_pcnt), (const int64_t *)(kws + o_pout),
                                       (int64_t *)(kws + o_cnt) + i0 * tc, (int64_t *)(kws + o_out) + 2 * i0, e->stream));
        VgxTauFlowLaunch a{};
        fill(a);
        a.m = m;
        a.rows = (const int64_t *)e->t_mev.p; a.stride = mev_cap;
        a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_rows = (const int32_t *)(kws + o_nown) + i0;
        a.cut = (const int32_t *)ws;
        a.max_n = max_n;
        a.counts = (int64_t *)(kws + o_cnt) + i0 * tc; a.outside = (int64_t *)(kws + o_out) + 2 * i0;
        HIPCHECK(e, vgxi_tau_flow_count(&a, e->stream));
        if (max_n > 0) io->passes += 1;
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
    }
    HIPCHECK(e, hipMemcpy(io->outside, kws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (io->counts) HIPCHECK(e, hipMemcpy(io->counts, kws + o_cnt, (size_t)block_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        // the column summary takes whole numbers below 2^31: narrow the block, and find its largest count on the way
        const uint64_t init[2] = {~(uint64_t)0, 0};
        uint64_t mm[2] = {0, 0};
        HIPCHECK(e, hipMemcpyAsync(kws + o_mm, init, sizeof init, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_tau_prev_minmax(n * tc, (const int64_t *)(kws + o_cnt), (int32_t *)(kws + o_nar), (uint64_t *)(kws + o_mm), e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "narrowing kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        const int64_t lo = (int64_t)(mm[0] ^ 0x8000000000000000ull), hi = (int64_t)(mm[1] ^ 0x8000000000000000ull);
        if (lo <= hi && hi >= ((int64_t)1 << 31))
            return fail(e, VGX_ERR_ARG, me + "summary: the largest count is " + std::to_string(hi) + ", the column summary takes whole numbers below 2^31 (use narrower bins, or summarise the int64 counts on the host)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_tau_flows: summary", (const int32_t *)(kws + o_nar), n, tc, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, cuts, cell and tile walk on a chain given as arrays (no device, no engine).  The
// last n_own_events events play the replicate's own steps (their rows are taken as they are, as the device reads t_mev), everything
// before them the prefix, which is flattened, counted once as a chain of its own and added, as on the device.
extern "C" int vgx_test_tau_flows(vgx_tau_flows_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_flows: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->counts || !io->outside) return fail_("null argument");
    const int64_t n = io->ev_ptr, T = io->T, P = io->popNum, H = io->hapNum, V = io->V;
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail_("bad dimensions");
    if (io->form != VGX_FLOW_AUTO && io->form != VGX_FLOW_DENSE && io->form != VGX_FLOW_SPLIT)
        return fail_("form = " + std::to_string(io->form) + " is none of 0 (automatic), 1 (dense), 2 (split)");
    int ran = 0;
    {
        const std::string why = check_request(io->edges, T, V, io->variant_of, P, H, (int)io->form, ran);
        if (!why.empty()) return fail_(why);
    }
    io->form_ran = ran;
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail_("chain too long");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail_("null event column");
    if (io->mev_rows < 0 || (io->mev_rows > 0 && (!io->mev_num || !io->mev_types || !io->mev_haplotypes || !io->mev_populations ||
                                                  !io->mev_newHaplotypes || !io->mev_newPopulations)))
        return fail_("null multievent column");
    int64_t tile = io->tile;
    if (tile < 0) return fail_("tile must not be negative");
    if (tile == 0) tile = VGX_FLOW_TILE_DEFAULT;
    const int64_t cells = P * P * V;
    if (T * cells >= ((int64_t)1 << 40)) return fail_("block too large");
    int64_t n_own_ev = io->n_own_events;
    if (n_own_ev < -1 || n_own_ev > n) return fail_("n_own_events must be -1 or lie in [0, ev_ptr]");
    if (n_own_ev < 0) {   // the chain's trailing MULTITYPE events
        n_own_ev = 0;
        while (n_own_ev < n && io->ev_types[n - 1 - n_own_ev] == VGX_TL_MULTITYPE) n_own_ev++;
    }
    const int64_t n_pre_ev = n - n_own_ev;
    const EventCols ev{n, io->ev_times, io->ev_types, io->ev_haplotypes, io->ev_populations, io->ev_newHaplotypes, io->ev_newPopulations};
    const RowCols mv{io->mev_rows, io->mev_num, io->mev_types, io->mev_haplotypes, io->mev_populations, io->mev_newHaplotypes, io->mev_newPopulations};
    FlatChain pre;
    {
        const std::string why = flatten(ev, n_pre_ev, mv, pre);
        if (!why.empty()) return fail_(why);
    }
    // the own rows as a block of their own, unjudged, with every own event's first row
    std::vector<int64_t> own, own_m0((size_t)n_own_ev);
    for (int64_t k = 0; k < n_own_ev; k++) {
        const int64_t i = n_pre_ev + k, t = ev.types[i];
        own_m0[(size_t)k] = (int64_t)own.size() / 6;
        if (t == VGX_TL_MULTITYPE) {
            const int64_t j0 = ev.hap[i], j1 = ev.pop[i];
            if (j1 <= j0) continue;
            if (j0 < 0 || j1 > mv.n) return fail_("event " + std::to_string(i) + ": MULTITYPE row range outside the multievent log");
            for (int64_t j = j0; j < j1; j++) {
                const int64_t v[6] = {mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]};
                own.insert(own.end(), v, v + 6);
            }
        } else {
            const int64_t v[6] = {1, t, ev.hap[i], ev.pop[i], ev.nh[i], ev.np[i]};
            own.insert(own.end(), v, v + 6);
        }
        if (pre.n_rows() + (int64_t)own.size() / 6 >= ((int64_t)1 << 31)) return fail_("the chain has 2^31 rows or more");
    }
    const int64_t pre_rows = pre.n_rows(), own_rows = (int64_t)own.size() / 6;
    std::vector<int32_t> pcut((size_t)(T + 1)), ocut((size_t)(T + 1));
    const int64_t point0 = prefix_cuts(pre, n_pre_ev, io->ev_times, io->edges, T, pcut.data());
    own_cuts(io->edges, T, point0, n_own_ev, [&](int64_t k) { return io->ev_times[n_pre_ev + k]; }, [&](int64_t k) { return own_m0[(size_t)k]; }, own_rows,
             ocut.data());
    const int32_t within = io->within ? 1 : 0;
    // the prefix block, counted once ...
    std::vector<int64_t> pblock((size_t)(T * cells), 0), hist((size_t)(vgx_tau_flow_lds_bytes(ran, P, V) / 8), 0);
    int64_t pout[2] = {0, 0};
    for (int64_t t0 = 0; t0 < pre_rows; t0 += tile)
        vgx_tau_flow_tile_host(ran, pre.rows.data(), pcut.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, within, (int32_t)t0,
                               (int32_t)std::min<int64_t>(t0 + tile, pre_rows), hist.data(), pblock.data(), pout);
    // ... is what the chain's block starts from; its own rows are added on top
    for (int64_t i = 0; i < T * cells; i++) io->counts[i] = pblock[(size_t)i];
    io->outside[0] = pout[0];
    io->outside[1] = pout[1];
    for (int64_t t0 = 0; t0 < own_rows; t0 += tile)
        vgx_tau_flow_tile_host(ran, own.data(), ocut.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, within, (int32_t)t0,
                               (int32_t)std::min<int64_t>(t0 + tile, own_rows), hist.data(), io->counts, io->outside);
    return VGX_OK;
}
