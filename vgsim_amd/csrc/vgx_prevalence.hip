// vgx_prevalence.hip — infectious hosts per population and variant class of every selected replicate of a direct ensemble at the
// times of one grid, on the device (vgx_get_prevalence), and the same rule, tile walk and scan compiled for the host
// (vgx_test_prevalence).  DESIGN.md §18.
//
// A stock is the running sum of flows, and a chain is long where the grid is short: instead of one sequential walk per replicate
// the counting kernel forms the NET change of every (interval, population, class) as a signed histogram, tile-parallel like
// vgx_incidence.hip, and the scan kernel adds the T + 1 intervals up per column.  A workgroup of 256 threads takes one replicate
// and a TILE of consecutive events, reads the log in place (three 8-byte loads per lane), finds the interval of its first event
// by a search in the replicate's bounds, and accumulates +1 / -1 into P * V int32 cells in LDS with LDS atomics; at every
// interval change and at the tile's end it adds the nonzero cells to the block in device memory and clears them (the form that
// adds every change straight to device memory was built and measured slower where it would apply: DESIGN.md §18).
// variant_of is staged in LDS behind the cells when it fits.  All arithmetic is integer: the block does not depend on the tile
// size or the launch geometry.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_prevalence.h"

namespace {

__global__ void __launch_bounds__(256) vgxp_count_kernel(VgxPrevLaunch a, int stage) {
    extern __shared__ int32_t hist[];      // [P][V] cells, then (stage) variant_of [hapNum]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_ev[row], T = a.T, P = a.P, V = a.V, cells = P * V;
    if ((int64_t)blockIdx.y * a.tile >= n) return;         // (the whole workgroup: the chain ends before its first tile)
    const int32_t *bound = a.bound + row * (int64_t)(T + 2);   // (uniform addresses: every thread reads the same bounds)
    const int2 *lg = (const int2 *)(a.log + a.rep[row] * a.evcap * 6);   // 8-byte aligned: 24-byte records from a 256-byte aligned base
    const int32_t *vo = a.variant_of;
    for (int i = tid; i < cells; i += 256) hist[i] = 0;
    if (stage) {
        int32_t *map = hist + cells;
        for (int i = tid; i < a.hapNum; i += 256) map[i] = vo[i];
        vo = map;
    }
    __syncthreads();
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t pos = (int32_t)t0;
        while (pos < e1) {
            const int32_t j = vgx_inc_bin(bound, T + 1, pos);
            const int32_t end = e1 < bound[j + 1] ? e1 : bound[j + 1];
            for (int32_t e = pos + tid; e < end; e += 256) {
                const int2 r0 = lg[(int64_t)e * 3], r1 = lg[(int64_t)e * 3 + 1], r2 = lg[(int64_t)e * 3 + 2];
                const int32_t c[5] = {r0.x, r0.y, r1.x, r1.y, r2.x};
                int32_t cell[2], sign[2];
                const int k = vgx_prev_deltas(c, P, a.hapNum, V, vo, cell, sign);
                if (k > 0) atomicAdd(&hist[cell[0]], sign[0]);
                if (k > 1) atomicAdd(&hist[cell[1]], sign[1]);
            }
            __syncthreads();
            int32_t *dst = vgx_prev_net(a.val, a.fin, row, T, cells, j);
            for (int i = tid; i < cells; i += 256) {
                const int32_t v = hist[i];
                if (v) { atomicAdd(&dst[i], v); hist[i] = 0; }
            }
            __syncthreads();
            pos = end;
        }
    }
}

// one thread per (replicate, population, class) column, consecutive threads consecutive classes: every step of the running sum
// reads and writes whole lines
__global__ void __launch_bounds__(256) vgxp_scan_kernel(VgxPrevLaunch a) {
    const int64_t cells = (int64_t)a.P * a.V, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.m * cells) return;
    const int64_t row = idx / cells, cell = idx % cells;
    vgx_prev_scan_column(a.val + row * a.T * cells + cell, a.fin + idx, a.start[idx], a.T, cells);
}

// smallest and largest of x[0 .. n): out[0] = min, out[1] = max (the caller sets INT32_MAX, INT32_MIN)
__global__ void __launch_bounds__(256) vgxp_minmax_kernel(const int32_t *__restrict__ x, int64_t n, int32_t *out) {
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t v = x[i];
        lo = min(lo, v);
        hi = max(hi, v);
    }
    for (int s = 32; s > 0; s >>= 1) {
        lo = min(lo, __shfl_xor(lo, s));
        hi = max(hi, __shfl_xor(hi, s));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
    }
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_prev_count(const VgxPrevLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if (vgx_prev_lds_bytes(a->P, a->V) > VGX_PREV_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const bool stage = vgx_prev_stage_map(a->P, a->V, a->hapNum);
    const int64_t lds = vgx_prev_lds_bytes(a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxp_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxp_count_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_prev_scan(const VgxPrevLaunch *a, hipStream_t s) {
    const int64_t cols = a->m * a->P * a->V;
    if (cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxp_scan_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, *a);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_prev_minmax(const int32_t *x, int64_t n, int32_t *out, hipStream_t s) {
    const int32_t init[2] = {INT32_MAX, INT32_MIN};
    hipError_t err = hipMemcpyAsync(out, init, sizeof init, hipMemcpyHostToDevice, s);
    if (err != hipSuccess || n <= 0) return err;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(vgxp_minmax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, out);
    return hipGetLastError();
}

// ---- the host instance: the same deltas, bounds, tile walk and scan on a chain given as arrays (no device, no engine)
extern "C" int vgx_test_prevalence(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                                   const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                                   const double *grid, int64_t T, const int32_t *variant_of, int64_t V, const int64_t *start, int64_t tile,
                                   int32_t *values, int32_t *final, int64_t *outside, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!grid || !variant_of || !start || !values || !final || !outside) return fail("vgx_test_prevalence: null argument");
    if (T < 1 || T >= VGX_PREV_MAX_POINTS) return fail("vgx_test_prevalence: T = " + std::to_string(T) + " must be at least 1 and below 2^24");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(grid[k])) return fail("vgx_test_prevalence: grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(grid[k - 1] < grid[k])) return fail("vgx_test_prevalence: grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (P < 1 || hapNum < 1 || P > INT32_MAX || hapNum > INT32_MAX) return fail("vgx_test_prevalence: bad dimensions");
    if (V < 1 || V > INT32_MAX) return fail("vgx_test_prevalence: V = " + std::to_string(V) + " must be at least 1");
    if (vgx_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail("vgx_test_prevalence: " + std::to_string(P) + " populations x " + std::to_string(V) + " classes need " +
                    std::to_string(vgx_prev_lds_bytes(P, V)) + " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) +
                    " bytes of LDS a counting workgroup may use");
    for (int64_t h = 0; h < hapNum; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return fail("vgx_test_prevalence: variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " +
                        std::to_string(V) + ")");
    const int64_t cells = P * V;
    for (int64_t i = 0; i < cells; i++)
        if (start[i] < 0 || start[i] > INT32_MAX) return fail("vgx_test_prevalence: start value outside [0, 2^31)");
    if (n_ev < 0 || n_ev >= VGX_PREV_MAX_EVENTS) return fail("vgx_test_prevalence: a chain of " + std::to_string(n_ev) + " events (2^30 or more)");
    if (n_ev > 0 && (!times || !types || !haplotypes || !populations || !newHaplotypes || !newPopulations))
        return fail("vgx_test_prevalence: null event column");
    if (tile < 0) return fail("vgx_test_prevalence: tile must not be negative");
    if (tile == 0) tile = VGX_PREV_TILE_DEFAULT;
    std::vector<int32_t> log((size_t)n_ev * 5);
    for (int64_t e = 0; e < n_ev; e++) {
        const int64_t v[5] = {types[e], haplotypes[e], populations[e], newHaplotypes[e], newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_prevalence: log value outside 32 bits");
            log[(size_t)(e * 5 + c)] = (int32_t)v[c];
        }
    }
    std::vector<int32_t> bound((size_t)(T + 2));
    VgxPrevCutter ct{grid, T, bound.data()};
    for (int64_t e = 0; e < n_ev; e++) ct.event(e, times[e]);
    ct.finish(n_ev);
    outside[0] = bound[1];
    outside[1] = n_ev - bound[(size_t)T];
    for (int64_t i = 0; i < T * cells; i++) values[i] = 0;
    for (int64_t i = 0; i < cells; i++) final[i] = 0;
    std::vector<int32_t> hist((size_t)cells, 0);
    for (int64_t t0 = 0; t0 < n_ev; t0 += tile)
        vgx_prev_tile_host(log.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)hapNum, (int32_t)V, variant_of, (int32_t)t0,
                           (int32_t)std::min<int64_t>(t0 + tile, n_ev), hist.data(), values, final);
    for (int64_t i = 0; i < cells; i++) vgx_prev_scan_column(values + i, final + i, (int32_t)start[i], (int32_t)T, cells);
    return VGX_OK;
}
