// vgx_timelines.hip — the log replays (get_data_infectious / get_data_susceptible, reference pyx:1967-2045) of every replicate
// of a direct ensemble on the device (vgx_get_timelines), and the same replay compiled for the host (vgx_test_timelines).
//
// Two kernels.  The PACK kernel gathers what the host clock needs of the selected replicates, the 8-byte rate log and the
// 32-bit iteration index (column 5 of the 24-byte records), into two contiguous staging arrays: 12 bytes per event go to the
// host instead of 32.  The REPLAY kernel is a streaming pass: one workgroup of 256 threads per replicate reads the log in
// place, consecutive lanes consecutive records (three 8-byte loads per lane: every byte of a fetched line is used), finds the
// record's bin in the cuts the host clock gave (vgx_tline.h; held in LDS, one comparison unless a cut was passed), looks the at
// most two compartments the event moves up in an LDS table of the queries (the cost per event does not grow with the number of
// queries) and adds to int32 per-bin counters in LDS.  The two query-independent rows of the reference semantics are reduced
// per wavefront before one LDS add.  The finish is an int64 prefix sum over the bins of every series by wavefront scans,
// start + sum stored as f64 (whole numbers far below 2^53) with coalesced stores.  Its floor is log bytes / HBM rate.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_tline.h"
#include "vgx_timelines.h"

namespace {

#define VGX_TL_PACK_TILE 4096   // events per workgroup of the pack kernel

__global__ void __launch_bounds__(256) vgxt_pack_kernel(const int32_t *log, const double *evrate, int64_t evcap, const int64_t *rep,
                                                        const int32_t *n_ev, const int64_t *off, int32_t *iter_out, double *rate_out) {
    const int64_t r = rep[blockIdx.x];
    const int32_t n = n_ev[blockIdx.x];
    const int32_t *lg = log + r * evcap * 6;
    const double *rt = evrate + r * evcap;
    const int64_t o = off[blockIdx.x];
    for (int64_t e0 = (int64_t)blockIdx.y * VGX_TL_PACK_TILE; e0 < n; e0 += (int64_t)gridDim.y * VGX_TL_PACK_TILE) {
        const int64_t e1 = e0 + VGX_TL_PACK_TILE < n ? e0 + VGX_TL_PACK_TILE : n;
        for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
            iter_out[o + e] = lg[e * 6 + 5];
            rate_out[o + e] = rt[e];
        }
    }
}

struct Rec { int2 a, b, c; };

__global__ void __launch_bounds__(256) vgxt_replay_kernel(VgxTlLaunch a) {
    extern __shared__ int32_t lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int step = a.step, T = step + 1, ni = a.ni, ns = a.ns, rows = 2 * ni + ns, ts = a.tsize;
    int32_t *cut = lds, *tab = cut + step, *g_ds = tab + 3 * ts, *g_s = g_ds + T, *cnt = g_s + T;
    for (int i = tid; i < step; i += 256) cut[i] = a.cut[b * step + i];
    for (int i = tid; i < 3 * ts; i += 256) tab[i] = a.tab[i];
    for (int i = tid; i < (2 + rows) * T; i += 256) g_ds[i] = 0;
    __syncthreads();
    const int32_t n = a.n_ev[b];
    const int2 *lg = (const int2 *)(a.log + a.rep[b] * a.evcap * 6);   // 8-byte aligned: 24-byte records from a 256-byte aligned base
    const bool reference = a.semantics == VGX_TL_REFERENCE;
    int bin = 0;

    auto load = [&](int32_t e, Rec &r) {
        if (e < n) { r.a = lg[(int64_t)e * 3]; r.b = lg[(int64_t)e * 3 + 1]; r.c = lg[(int64_t)e * 3 + 2]; }
        else r.a = r.b = r.c = make_int2(-1, -1);
    };
    auto apply = [&](int32_t e, const Rec &r) {
        const bool act = e < n;
        if (act) bin = vgx_tl_bin(cut, step, e, bin);
        const int32_t c[5] = {r.a.x, r.a.y, r.b.x, r.b.y, r.c.x};
        VgxTlMoves m;
        vgx_tl_classify(a.semantics, c, m);     // (a record past the end carries type -1: no moves)
        if (reference) {
            // the rows every event of a type moves are the contended ones: one add per wavefront when its records share a bin
            const int b0 = __shfl(bin, 0);
            if (__all(!act || bin == b0)) {
                const int nds = __popcll(__ballot(m.all_ds)), nsm = __popcll(__ballot(m.all_s));
                if (lane == 0) {
                    if (nds) atomicAdd(&g_ds[b0], nds);
                    if (nsm) atomicAdd(&g_s[b0], nsm);
                }
            } else {
                if (m.all_ds) atomicAdd(&g_ds[bin], 1);
                if (m.all_s) atomicAdd(&g_s[bin], 1);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const VgxTlOp &o = m.op[k];
            if (o.side < 0) continue;
            const int32_t row = vgx_tl_find(tab, ts, o.side, o.major, o.minor);
            if (row < 0) continue;
            atomicAdd(&cnt[row * T + bin], o.delta);
            if (o.sample) atomicAdd(&cnt[(row + ni) * T + bin], 1);
        }
    };
    // two tiles of 256 records in flight per workgroup
    for (int32_t base = 0; base < n; base += 512) {
        Rec r0, r1;
        load(base + tid, r0);
        load(base + 256 + tid, r1);
        apply(base + tid, r0);
        apply(base + 256 + tid, r1);
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
            long long v = c < T ? (long long)cnt[r * T + c] : 0;
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

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tl_pack(const int32_t *log, const double *evrate, int64_t evcap, const int64_t *rep,
                                                                         const int32_t *n_ev, const int64_t *off, int64_t m, int64_t max_n,
                                                                         int32_t *iter_out, double *rate_out, hipStream_t s) {
    if (m <= 0 || max_n <= 0) return hipSuccess;
    const int64_t all_tiles = (max_n + VGX_TL_PACK_TILE - 1) / VGX_TL_PACK_TILE;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipLaunchKernelGGL(vgxt_pack_kernel, dim3((unsigned)m, tiles), dim3(256), 0, s, log, evrate, evcap, rep, n_ev, off, iter_out, rate_out);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tl_replay(const VgxTlLaunch *a, hipStream_t s) {
    if (a->m <= 0) return hipSuccess;
    const int64_t lds = vgx_tl_lds_bytes(a->step, a->ni, a->ns);
    if (lds > VGX_TL_LDS_MAX) return hipErrorInvalidValue;
    hipError_t err = hipFuncSetAttribute((const void *)vgxt_replay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxt_replay_kernel, dim3((unsigned)a->m), dim3(256), (size_t)lds, s, *a);
    return hipGetLastError();
}

// ---- the host instance: the same classification, cuts, bins and table on a chain given as arrays (no device, no engine)
extern "C" int vgx_test_timelines(vgx_timelines_chain *io, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->time_points) return fail("vgx_test_timelines: null argument");
    const int64_t n = io->ev_ptr, step = io->step_num, ni = io->n_inf, ns = io->n_sus, T = step + 1;
    if (step < 1 || step >= ((int64_t)1 << 24)) return fail("vgx_test_timelines: step_num must be at least 1");
    if (io->semantics != VGX_TL_REFERENCE && io->semantics != VGX_TL_COMPARTMENT) return fail("vgx_test_timelines: unknown semantics");
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail("vgx_test_timelines: chain too long");
    if (ni < 0 || ns < 0 || ni + ns >= ((int64_t)1 << 20)) return fail("vgx_test_timelines: bad query count");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail("vgx_test_timelines: null event column");
    if ((ni > 0 && (!io->inf_pop || !io->inf_hap || !io->inf_start || !io->inf_data || !io->inf_sample)) ||
        (ns > 0 && (!io->sus_pop || !io->sus_grp || !io->sus_start || !io->sus_data)))
        return fail("vgx_test_timelines: null query or output array");
    const int ts = vgx_tl_table_size((int)(ni + ns));
    std::vector<int32_t> tab((size_t)(3 * ts), -1);
    for (int64_t k = 0; k < ni; k++) {
        if (io->inf_pop[k] < 0 || io->inf_pop[k] >= io->popNum) return fail("vgx_test_timelines: population index out of range");
        if (io->inf_hap[k] < 0 || io->inf_hap[k] >= io->hapNum) return fail("vgx_test_timelines: haplotype index out of range");
        if (!vgx_tl_insert(tab.data(), ts, 0, (int32_t)io->inf_pop[k], (int32_t)io->inf_hap[k], (int32_t)k))
            return fail("vgx_test_timelines: an infectious query is given twice");
    }
    for (int64_t k = 0; k < ns; k++) {
        if (io->sus_pop[k] < 0 || io->sus_pop[k] >= io->popNum) return fail("vgx_test_timelines: population index out of range");
        if (io->sus_grp[k] < 0 || io->sus_grp[k] >= io->susNum) return fail("vgx_test_timelines: susceptibility group index out of range");
        if (!vgx_tl_insert(tab.data(), ts, 1, (int32_t)io->sus_pop[k], (int32_t)io->sus_grp[k], (int32_t)(2 * ni + k)))
            return fail("vgx_test_timelines: a susceptible query is given twice");
    }
    // the chain in the device log's record layout
    std::vector<int32_t> log((size_t)n * 5);
    for (int64_t e = 0; e < n; e++) {
        const int64_t v[5] = {io->ev_types[e], io->ev_haplotypes[e], io->ev_populations[e], io->ev_newHaplotypes[e], io->ev_newPopulations[e]};
        if (v[0] == VGX_TL_MULTITYPE && v[2] > v[1])
            return fail("vgx_test_timelines: event " + std::to_string(e) + " is a MULTITYPE record with rows: direct chains only");
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_timelines: log value outside 32 bits");
            log[(size_t)(e * 5 + c)] = (int32_t)v[c];
        }
    }
    vgx_tl_time_points(io->currentTime, step, io->time_points);
    std::vector<int32_t> cut((size_t)step);
    VgxTlCutter ct{io->time_points, step, cut.data()};
    for (int64_t e = 0; e < n; e++) ct.event(e, io->ev_times[e]);
    const int64_t last = ct.finish(n);
    io->last_point = last;
    const int64_t rows = 2 * ni + ns;
    std::vector<int32_t> cnt((size_t)((2 + rows) * T), 0);
    int32_t *g_ds = cnt.data(), *g_s = g_ds + T, *cn = g_s + T;
    int bin = 0;
    for (int64_t e = 0; e < n; e++) {
        bin = vgx_tl_bin(cut.data(), (int)step, (int32_t)e, bin);
        VgxTlMoves m;
        vgx_tl_classify((int)io->semantics, log.data() + e * 5, m);
        g_ds[bin] += m.all_ds;
        g_s[bin] += m.all_s;
        for (int k = 0; k < 2; k++) {
            const VgxTlOp &o = m.op[k];
            if (o.side < 0) continue;
            const int32_t row = vgx_tl_find(tab.data(), ts, o.side, o.major, o.minor);
            if (row < 0) continue;
            cn[row * T + bin] += o.delta;
            if (o.sample) cn[(row + ni) * T + bin] += 1;
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
