// vgx_tree_events.hip — the binning kernel of vgx_get_tree_events and vgx_get_tau_tree_events: the lineage logs the walks of
// vgx_lineages.hip and vgx_tau_lineages.hip wrote, counted per interval of the grid, population, variant class and kind by the
// rule of vgx_tree_events.h.  DESIGN.md §28.  The tile scheme is vgxl_bin_kernel's: a workgroup of 256 threads takes one replicate
// and a TILE of consecutive records (VGX_LINEAGES_TILE_RECORDS: it is the same log), finds the interval of its first record by a
// search on its event index in the replicate's bounds, finds the run's end where a search in the tile meets the first record below
// the interval's lower bound (records lie in descending event order), counts the run into P * V * VGX_TE_K int32 cells in LDS
// with LDS atomics, and adds the nonzero cells to the interval's row of the block at every interval change and at the tile's end.
// No scan follows: counts are per interval.  All of it is integer addition: the block does not depend on the tile size or the
// launch geometry.
#include <hip/hip_runtime.h>
#include "vgx_tree_events.h"

namespace {

__global__ void __launch_bounds__(256) vgxe_bin_kernel(VgxTeLaunch a, int stage) {
    extern __shared__ int32_t hist[];      // [P][V][K] cells, then (stage) variant_of [H]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    int64_t n = a.n_rec[row];
    const int64_t cap = a.desc[row].rec_cap;
    n = n < 0 ? 0 : (n > cap ? cap : n);                    // (never past the replicate's log)
    const int32_t T = a.T, P = a.P, H = a.H, V = a.V, cells = P * V * VGX_TE_K;
    if ((int64_t)blockIdx.y * a.tile >= n) return;         // (the whole workgroup: the log ends before its first tile)
    const int32_t *bound = a.bound + row * (int64_t)(T + 2);   // (uniform addresses: every thread reads the same bounds)
    const int32_t *rec = a.rec + a.desc[row].rec_off * 6;
    const int2 *rc = (const int2 *)rec;                    // 8-byte aligned: 24-byte records from a 256-byte aligned base
    const int32_t *vo = a.variant_of;
    for (int i = tid; i < cells; i += 256) hist[i] = 0;
    if (stage) {
        int32_t *map = hist + cells;
        for (int i = tid; i < H; i += 256) map[i] = vo[i];
        vo = map;
    }
    __syncthreads();
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int64_t r1 = t0 + a.tile < n ? t0 + a.tile : n;
        int64_t pos = t0;
        while (pos < r1) {
            const int32_t j = vgx_ln_interval(bound, T, rec[pos * 6 + 5]);
            const int64_t end = vgx_ln_run_end(rec, pos, r1, bound[j]);
            for (int64_t r = pos + tid; r < end; r += 256) {
                const int2 r0 = rc[r * 3], r1w = rc[r * 3 + 1], r2 = rc[r * 3 + 2];
                const int32_t c[5] = {r0.x, r0.y, r1w.x, r1w.y, r2.x};
                int32_t cell[2];
                const int k = vgx_te_cells(c, P, H, V, vo, cell);
                if (k > 0) atomicAdd(&hist[cell[0]], 1);
                if (k > 1) atomicAdd(&hist[cell[1]], 1);
            }
            __syncthreads();
            int32_t *dst = a.counts + (row * (T + 1) + j) * (int64_t)cells;   // (j in 0 .. T by vgx_ln_interval)
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

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_te_bin(const VgxTeLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_rec <= 0) return hipSuccess;
    if (vgx_te_lds_bytes(a->P, a->V) > VGX_PREV_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const bool stage = vgx_te_stage_map(a->P, a->V, a->H);
    const int64_t lds = vgx_te_lds_bytes(a->P, a->V) + (stage ? 4 * (int64_t)a->H : 0);
    const int64_t all_tiles = (a->max_rec + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxe_bin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxe_bin_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}
