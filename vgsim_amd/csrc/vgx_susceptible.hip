// vgx_susceptible.hip — susceptible hosts per population and class of immunity groups of every selected replicate of a direct
// ensemble at the times of one grid: the counting kernel of vgx_get_susceptibles (vgx_api.hip), and the same rule, tile walk and
// scan compiled for the host (vgx_test_susceptibles).  The rule is vgx_susceptible.h; DESIGN.md §20.
//
// The pass is vgx_prevalence.hip's with another table: a workgroup of 256 threads takes one replicate and a TILE of consecutive
// events, reads the log in place (three 8-byte loads per lane), finds the interval of its first event by a search in the
// replicate's bounds, and accumulates +1 / -1 into P * G int32 cells in LDS with LDS atomics; at every interval change and at the
// tile's end it adds the nonzero cells to the net block in device memory and clears them.  class_of is staged in LDS behind the
// cells when it fits.  The cells are few here (P * G is rarely above a few hundred), so the LDS atomics of a tile land on a
// handful of addresses; one private copy of the cells per wavefront, summed at the flush, was built and measured against this
// form at 16 and at 140 cells and made no difference, so the plain form stays.
// The scan and the min/max pass are vgxi_prev_scan and vgxi_prev_minmax as they are (VgxPrevLaunch with hapNum := susNum,
// V := G, variant_of := class_of).  All arithmetic is integer: the block does not depend on the tile size or the launch geometry.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_susceptible.h"

namespace {

__global__ void __launch_bounds__(256) vgxs_count_kernel(VgxPrevLaunch a, int stage) {
    extern __shared__ int32_t hist[];      // [P][G] cells, then (stage) class_of [susNum]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_ev[row], T = a.T, P = a.P, G = a.V, cells = P * G;
    if ((int64_t)blockIdx.y * a.tile >= n) return;         // (the whole workgroup: the chain ends before its first tile)
    const int32_t *bound = a.bound + row * (int64_t)(T + 2);   // (uniform addresses: every thread reads the same bounds)
    const int2 *lg = (const int2 *)(a.log + a.rep[row] * a.evcap * 6);   // 8-byte aligned: 24-byte records from a 256-byte aligned base
    const int32_t *co = a.variant_of;
    for (int i = tid; i < cells; i += 256) hist[i] = 0;
    if (stage) {
        int32_t *map = hist + cells;
        for (int i = tid; i < a.hapNum; i += 256) map[i] = co[i];
        co = map;
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
                const int k = vgx_sus_deltas(c, P, a.hapNum, G, co, cell, sign);
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

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_sus_count(const VgxPrevLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if (vgx_prev_lds_bytes(a->P, a->V) > VGX_PREV_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const bool stage = vgx_prev_stage_map(a->P, a->V, a->hapNum);
    const int64_t lds = vgx_prev_lds_bytes(a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxs_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxs_count_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

// ---- the host instance: the same deltas, bounds, tile walk and scan on a chain given as arrays (no device, no engine)
extern "C" int vgx_test_susceptibles(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                                     const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t susNum,
                                     const double *grid, int64_t T, const int32_t *class_of, int64_t G, const int64_t *start, int64_t tile,
                                     int32_t *values, int32_t *final, int64_t *outside, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_susceptibles: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!grid || !class_of || !start || !values || !final || !outside) return fail("null argument");
    if (T < 1 || T >= VGX_PREV_MAX_POINTS) return fail("T = " + std::to_string(T) + " must be at least 1 and below 2^24");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(grid[k])) return fail("grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(grid[k - 1] < grid[k])) return fail("grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (P < 1 || susNum < 1 || P > INT32_MAX || susNum > INT32_MAX) return fail("bad dimensions");
    if (G < 1 || G > INT32_MAX) return fail("G = " + std::to_string(G) + " must be at least 1");
    if (vgx_prev_lds_bytes(P, G) > VGX_PREV_LDS_MAX)
        return fail(std::to_string(P) + " populations x " + std::to_string(G) + " classes need " + std::to_string(vgx_prev_lds_bytes(P, G)) +
                    " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    for (int64_t g = 0; g < susNum; g++)
        if (class_of[g] < -1 || class_of[g] >= G)
            return fail("class_of[" + std::to_string(g) + "] = " + std::to_string(class_of[g]) + " is outside [-1, " + std::to_string(G) + ")");
    const int64_t cells = P * G;
    for (int64_t i = 0; i < cells; i++)
        if (start[i] < 0 || start[i] > INT32_MAX) return fail("start value outside [0, 2^31)");
    if (n_ev < 0 || n_ev >= VGX_PREV_MAX_EVENTS) return fail("a chain of " + std::to_string(n_ev) + " events (2^30 or more)");
    if (n_ev > 0 && (!times || !types || !haplotypes || !populations || !newHaplotypes || !newPopulations)) return fail("null event column");
    if (tile < 0) return fail("tile must not be negative");
    if (tile == 0) tile = VGX_PREV_TILE_DEFAULT;
    std::vector<int32_t> log((size_t)n_ev * 5);
    for (int64_t e = 0; e < n_ev; e++) {
        const int64_t v[5] = {types[e], haplotypes[e], populations[e], newHaplotypes[e], newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("log value outside 32 bits");
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
        vgx_sus_tile_host(log.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)susNum, (int32_t)G, class_of, (int32_t)t0,
                          (int32_t)std::min<int64_t>(t0 + tile, n_ev), hist.data(), values, final);
    for (int64_t i = 0; i < cells; i++) vgx_prev_scan_column(values + i, final + i, (int32_t)start[i], (int32_t)T, cells);
    return VGX_OK;
}
