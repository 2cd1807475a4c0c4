// vgx_milestones.hip — peaks, first passages and last positive events per population (and all populations together) and variant
// class of every selected replicate of a direct ensemble, on the device (vgx_get_milestones), and the same rule, round and merge
// compiled for the host (vgx_test_milestones).  DESIGN.md §21.
//
// A running maximum is not a sum: where vgx_prevalence.hip may count a tile's events in any order, this pass has to respect the
// order of events inside a chain.  It does so in two steps.  Pass A (vgx_prevalence.hip's counting and scan kernels, with the tile
// edges as bounds) gives every tile its base, the values at its first event.  The walk below then takes one wavefront per
// (replicate, tile): 64 consecutive events per round, one per lane; the round forms the ballots of the lanes that add to and take
// from each of its distinct cells, and every lane settles one cell's record in LDS from those masks by population counts
// (vgx_ms_round, vgx_ms_settle), rounds in log order; at the tile's end the records are merged into the replicate's block in device
// memory with integer atomic extrema.  One wavefront per workgroup: the rounds of a tile are sequential, so further wavefronts
// of a workgroup could only take turns behind a barrier.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_milestones.h"

namespace {

// the wave of vgx_ms_round on the device: lane `lane` evaluates f for itself.  With one wavefront per workgroup the round ends with
// the workgroup's barrier; with several the kernel places a barrier after every turn instead.
template <int WAVES>
struct VgxMsDevWave {
    int lane;
    __device__ int slot(int) const { return 0; }
    template <class F> __device__ uint64_t ballot(F f) const { return (uint64_t)__ballot(f(lane) ? 1 : 0); }
    template <class F> __device__ int32_t at(int l, F f) const { return __builtin_amdgcn_readlane(f(lane), l); }   // (l is uniform)
    template <class F> __device__ void each(F f) const { f(lane); }
    __device__ void sync() const { if (WAVES == 1) __syncthreads(); }
};

// WAVES = 1: one wavefront walks the tile's rounds one after another.  WAVES = 4: four wavefronts load four consecutive rounds at
// once and apply them in turn, a barrier after every turn (the diagnostic shape of VGX_MILESTONES_WAVES=4).
template <int WAVES>
__global__ void __launch_bounds__(VGX_MS_LANES * WAVES) vgxm_walk_kernel(VgxMsLaunch g) {
    extern __shared__ int32_t lds[];       // the records: [4 + K][cells]
    constexpr int THREADS = VGX_MS_LANES * WAVES;
    const VgxPrevLaunch &a = g.a;
    const int tid = (int)threadIdx.x, lane = tid & (VGX_MS_LANES - 1), wave = tid / VGX_MS_LANES;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_ev[row], P = a.P, V = a.V, pv = P * V, cells = pv + V, K = g.K;
    if ((int64_t)blockIdx.y * a.tile >= n) return;         // (the whole workgroup: the chain ends before its first tile)
    const int2 *lg = (const int2 *)(a.log + a.rep[row] * a.evcap * 6);   // 8-byte aligned, as in vgx_prevalence.hip
    const VgxMsRecords rec = vgx_ms_records(lds, cells);
    const VgxMsBlock blk{g.peak + row * cells, g.last_pos + row * cells, g.first + row * K * cells};
    const VgxMsDevWave<WAVES> w{lane};
    for (int64_t t = blockIdx.y; t * a.tile < n; t += gridDim.y) {
        for (int32_t i = tid; i < cells; i += THREADS) {
            uint32_t v = 0;
            if (i < pv) v = (uint32_t)vgx_ms_base(a.start, a.val, row, a.T, pv, t, i);
            else for (int32_t p = 0; p < P; p++) v += (uint32_t)vgx_ms_base(a.start, a.val, row, a.T, pv, t, p * V + (i - pv));
            vgx_ms_record_init(rec, i, cells, K, (int32_t)v);
        }
        __syncthreads();
        const int64_t e1 = t * a.tile + a.tile < n ? t * a.tile + a.tile : n;
        for (int64_t r0 = t * a.tile; r0 < e1; r0 += THREADS) {      // (uniform over the workgroup)
            const int64_t e0 = r0 + (int64_t)wave * VGX_MS_LANES;
            const int32_t nl = (int32_t)(e1 - e0 < VGX_MS_LANES ? (e1 - e0 > 0 ? e1 - e0 : 0) : VGX_MS_LANES);
            VgxMsEvents<1> ev;
            if (lane < nl) {
                const int64_t e = e0 + lane;
                const int2 r0v = lg[e * 3], r1v = lg[e * 3 + 1], r2v = lg[e * 3 + 2];
                const int32_t c[5] = {r0v.x, r0v.y, r1v.x, r1v.y, r2v.x};
                vgx_ms_load(ev, 0, c, P, a.hapNum, V, a.variant_of);
            } else {
                vgx_ms_load(ev, 0, (const int32_t *)nullptr, P, a.hapNum, V, a.variant_of);
            }
            if (WAVES == 1) {
                vgx_ms_round(w, ev, (int32_t)e0, nl, g.theta, K, cells, rec);     // (ends with a barrier)
            } else {
                for (int turn = 0; turn < WAVES; turn++) {
                    if (wave == turn && nl > 0) vgx_ms_round(w, ev, (int32_t)e0, nl, g.theta, K, cells, rec);
                    __syncthreads();
                }
            }
        }
        for (int32_t i = tid; i < cells; i += THREADS) {
            if (rec.peak_event[i] != VGX_MS_NONE)
                atomicMax((unsigned long long *)&blk.peak[i], (unsigned long long)vgx_ms_pack_peak(rec.peak[i], rec.peak_event[i]));
            if (rec.last_pos[i] != VGX_MS_NONE) atomicMax(&blk.last_pos[i], rec.last_pos[i]);
            for (int32_t k = 0; k < K; k++) {
                const int32_t fe = rec.first[(int64_t)k * cells + i];
                if (fe != VGX_MS_NEVER) atomicMin(&blk.first[(int64_t)k * cells + i], fe);
            }
        }
        __syncthreads();
    }
}

}  // namespace

// waves: wavefronts of a workgroup, 1 (the shape kept) or 4 (measured against it)
extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ms_walk(const VgxMsLaunch *g, int waves, hipStream_t s) {
    const VgxPrevLaunch &a = g->a;
    if (a.m <= 0 || a.max_n <= 0) return hipSuccess;
    const int64_t lds = vgx_ms_lds_bytes(a.P, a.V, g->K);
    if (lds > VGX_MS_LDS_MAX || a.tile < 1 || g->K < 0 || g->K > VGX_MS_MAX_K || (waves != 1 && waves != 4)) return hipErrorInvalidValue;
    const int64_t all_tiles = (a.max_n + a.tile - 1) / a.tile;
    if (all_tiles > a.T) return hipErrorInvalidValue;      // (the bases of pass A cover every tile)
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    const void *kernel = waves == 1 ? (const void *)vgxm_walk_kernel<1> : (const void *)vgxm_walk_kernel<4>;
    hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    if (waves == 1) hipLaunchKernelGGL(vgxm_walk_kernel<1>, dim3((unsigned)a.m, tiles), dim3(VGX_MS_LANES), (size_t)lds, s, *g);
    else hipLaunchKernelGGL(vgxm_walk_kernel<4>, dim3((unsigned)a.m, tiles), dim3(VGX_MS_LANES * 4), (size_t)lds, s, *g);
    return hipGetLastError();
}

// ---- the host instance: the same deltas, tile nets and bases, rounds of 64 emulated lanes and merge on a chain given as arrays
extern "C" int vgx_test_milestones(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                                   const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                                   const int32_t *variant_of, int64_t V, const int64_t *start, const int32_t *thresholds, int64_t K, int64_t tile,
                                   double t_start, int32_t *final, int32_t *peak, int32_t *peak_event, int32_t *last_positive_event,
                                   int32_t *first_event, double *peak_time, double *extinction_time, double *first_time, char *errbuf,
                                   int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!variant_of || !start || !final || !peak || !peak_event || !last_positive_event || !peak_time || !extinction_time)
        return fail("vgx_test_milestones: null argument");
    if (K < 0 || K > VGX_MS_MAX_K) return fail("vgx_test_milestones: K = " + std::to_string(K) + " thresholds: at most 16");
    if (K > 0 && (!thresholds || !first_event || !first_time)) return fail("vgx_test_milestones: null argument");
    if (P < 1 || hapNum < 1 || P >= INT32_MAX || hapNum > INT32_MAX) return fail("vgx_test_milestones: bad dimensions");
    if (V < 1 || V > INT32_MAX) return fail("vgx_test_milestones: V = " + std::to_string(V) + " must be at least 1");
    if (vgx_ms_lds_bytes(P, V, K) > VGX_MS_LDS_MAX)
        return fail("vgx_test_milestones: " + std::to_string(P) + " populations (and their total) x " + std::to_string(V) + " classes x " + std::to_string(K) +
                    " thresholds need " + std::to_string(vgx_ms_lds_bytes(P, V, K)) + " bytes of records, above the " + std::to_string((int64_t)VGX_MS_LDS_MAX) +
                    " bytes of LDS a walking workgroup may use");
    for (int64_t h = 0; h < hapNum; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return fail("vgx_test_milestones: variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " +
                        std::to_string(V) + ")");
    const int64_t pv = P * V, cells = pv + V;
    std::vector<int32_t> st((size_t)cells, 0);
    for (int64_t c = 0; c < V; c++) {
        int64_t sum = 0;
        for (int64_t p = 0; p < P; p++) {
            const int64_t v = start[p * V + c];
            if (v < 0 || v > INT32_MAX) return fail("vgx_test_milestones: start value outside [0, 2^31)");
            st[(size_t)(p * V + c)] = (int32_t)v;
            sum += v;
        }
        if (sum > INT32_MAX) return fail("vgx_test_milestones: start value outside [0, 2^31)");
        st[(size_t)(pv + c)] = (int32_t)sum;
    }
    if (n_ev < 0 || n_ev >= VGX_MS_MAX_EVENTS) return fail("vgx_test_milestones: a chain of " + std::to_string(n_ev) + " events (2^30 or more)");
    if (n_ev > 0 && (!times || !types || !haplotypes || !populations || !newHaplotypes || !newPopulations))
        return fail("vgx_test_milestones: null event column");
    if (tile < 0) return fail("vgx_test_milestones: tile must not be negative");
    if (tile == 0) tile = VGX_MS_TILE_DEFAULT;
    tile = std::min<int64_t>(tile, VGX_MS_MAX_EVENTS);
    std::vector<int32_t> log((size_t)n_ev * 5);
    for (int64_t e = 0; e < n_ev; e++) {
        const int64_t v[5] = {types[e], haplotypes[e], populations[e], newHaplotypes[e], newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_milestones: log value outside 32 bits");
            log[(size_t)(e * 5 + c)] = (int32_t)v[c];
        }
    }
    const int32_t Pi = (int32_t)P, Vi = (int32_t)V, Ki = (int32_t)K, Hi = (int32_t)hapNum;
    // pass A: the tile edges as bounds, the tile nets, the running sums
    const int64_t T = std::max<int64_t>((n_ev + tile - 1) / tile, 1);
    std::vector<int32_t> bound((size_t)(T + 2));
    for (int64_t j = 0; j <= T + 1; j++) bound[(size_t)j] = (int32_t)std::min<int64_t>(j * tile, n_ev);
    std::vector<int32_t> val((size_t)(T * pv), 0), fin((size_t)pv, 0), hist((size_t)pv, 0);
    for (int64_t t0 = 0; t0 < n_ev; t0 += tile)
        vgx_prev_tile_host(log.data(), bound.data(), (int32_t)T, Pi, Hi, Vi, variant_of, (int32_t)t0, (int32_t)std::min<int64_t>(t0 + tile, n_ev),
                           hist.data(), val.data(), fin.data());
    for (int64_t i = 0; i < pv; i++) vgx_prev_scan_column(val.data() + i, fin.data() + i, st[(size_t)i], (int32_t)T, pv);
    // the block from the start, then every tile: records from its base, its rounds, the merge
    std::vector<uint64_t> bpeak((size_t)cells);
    std::vector<int32_t> blast((size_t)cells), bfirst((size_t)(std::max<int64_t>(K, 1) * cells));
    const VgxMsBlock blk{bpeak.data(), blast.data(), bfirst.data()};
    for (int64_t i = 0; i < cells; i++) vgx_ms_init_cell(blk, (int32_t)i, (int32_t)cells, st[(size_t)i], thresholds, Ki);
    std::vector<int32_t> lds((size_t)((4 + K) * cells));
    const VgxMsRecords rec = vgx_ms_records(lds.data(), (int32_t)cells);
    const VgxMsHostWave w;
    VgxMsEvents<VGX_MS_LANES> ev;
    for (int64_t t = 0; t * tile < n_ev; t++) {
        for (int32_t i = 0; i < cells; i++) {
            uint32_t v = 0;
            if (i < pv) v = (uint32_t)vgx_ms_base(st.data(), val.data(), 0, (int32_t)T, (int32_t)pv, t, i);
            else for (int32_t p = 0; p < Pi; p++) v += (uint32_t)vgx_ms_base(st.data(), val.data(), 0, (int32_t)T, (int32_t)pv, t, p * Vi + (i - (int32_t)pv));
            vgx_ms_record_init(rec, i, (int32_t)cells, Ki, (int32_t)v);
        }
        const int64_t e1 = std::min<int64_t>(t * tile + tile, n_ev);
        for (int64_t e0 = t * tile; e0 < e1; e0 += VGX_MS_LANES) {
            const int32_t nl = (int32_t)std::min<int64_t>(VGX_MS_LANES, e1 - e0);
            for (int l = 0; l < VGX_MS_LANES; l++)
                vgx_ms_load(ev, l, l < nl ? log.data() + (e0 + l) * 5 : (const int32_t *)nullptr, Pi, Hi, Vi, variant_of);
            vgx_ms_round(w, ev, (int32_t)e0, nl, thresholds, Ki, (int32_t)cells, rec);
        }
        vgx_ms_merge_host(rec, blk, (int32_t)cells, Ki);
    }
    const VgxMsOut out{final, peak, peak_event, last_positive_event, first_event, peak_time, extinction_time, first_time};
    vgx_ms_outputs(blk, fin.data(), Pi, Vi, Ki, n_ev, times, t_start, out);
    return VGX_OK;
}
