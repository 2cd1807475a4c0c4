// vgx_lineages.hip — ancestral lineages per population and variant class of every selected replicate of a direct ensemble at the
// times of one grid, on the device (vgx_get_lineages).  DESIGN.md §26.  Three kernels, chained on one stream per pass:
//   1. the backward walk of vgx_genealogies.hip with the logging observer of vgx_lineages.h: one replicate per wavefront, lane 0
//      working (the layout DESIGN.md §10 measured as the faster one), the log prefetched through LDS, the same draws and the same
//      generator afterwards.  It keeps the parents of the tree as workspace (the closing pass reads them) and writes no tree,
//      mutation or migration outputs: what leaves it is the lineage log, the result and the generator;
//   2. the binning of the lineage logs, in the geometry of vgx_prevalence.hip: a workgroup of 256 threads takes one replicate and
//      a TILE of consecutive records, finds the interval of its first record by a search on its event index in the replicate's
//      bounds, accumulates +1 / -1 into P * V int32 cells in LDS, and adds the nonzero cells to the block of net changes at every
//      interval change and at the tile's end.  Records lie in descending event order, so the run of one interval ends where a
//      search in the tile finds the first record below the interval's lower bound;
//   3. the suffix sum that turns every (replicate, population, class) column of net changes into values and root where it lies.
// All arithmetic after the walk is integer: the block does not depend on the tile size or the launch geometry.
#include <hip/hip_runtime.h>
#include "vgx_lineages.h"
#include "vgx_gwalk_lds.h"

namespace {

__global__ void __launch_bounds__(64) vgxl_walk_kernel(VgxLnLaunch a) {
    __shared__ int32_t buf[VGX_GW_CHUNK * 6 * 64];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x;
    if (lane != 0 || i >= a.m) return;
    const VgxLnDesc d = a.desc[i];
    VgxGwRep w;
    w.n_ev = d.n_ev; w.sCounter = d.sCounter; w.H = a.H; w.tsize = d.tsize;
    w.key = a.key + d.tab_off; w.cnt = a.cnt + d.tab_off;
    w.base = a.base + d.tab_off; w.len = a.len + d.tab_off; w.lcap = a.lcap + d.tab_off;
    w.arena = a.arena + d.arena_off; w.arena_cap = d.arena_cap;
    w.tree = a.tree + d.node_off; w.tree_pop = nullptr; w.node_ev = nullptr;   // (an observer without records: never touched)
    w.mut_cap = 0; w.mut_node = w.mut_AS = w.mut_DS = w.mut_site = w.mut_ev = nullptr;
    w.mig_cap = 0; w.mig_node = w.mig_old = w.mig_new = w.mig_ev = nullptr;
    VgxGwLdsReader rd{a.log + d.rep * a.evcap * 6, d.n_ev, buf + lane, -1};
    VgxGwResult res{};
    VgxPcg64 g{d.rng[0], d.rng[1], d.rng[2], d.rng[3]};
    VgxLnLog lg{a.rec + d.rec_off * 6, d.rec_cap, 0, 0};
    res.status = d.sCounter < 2 ? VGX_GW_FEW_SAMPLES : vgx_gw_prepass(w, rd);   // (no workspace below two samples)
    if (res.status == VGX_GW_OK) {
        // infectious counts of the compartments the chain touches, from the final occupancy lists
        for (int64_t p = 0; p < a.P; p++) {
            int64_t no = a.nocc[d.rep * a.P + p];
            no = no < 0 ? 0 : (no > a.cap ? a.cap : no);
            const int64_t l0 = (d.rep * a.P + p) * a.cap;
            for (int64_t k = 0; k < no; k++) {
                const int64_t s = vgx_gw_find(w, p * a.H + a.lhap[l0 + k]);
                if (s >= 0) w.cnt[s] = a.lcnt[l0 + k];
            }
        }
        vgx_gw_walk(w, rd, g, res, VgxLnObserver{&lg});
        if (res.status == VGX_GW_OK && lg.dropped > 0) res.status = VGX_GW_WORKSPACE;   // a full lineage log
    }
    int64_t *r = a.res + i * 5;
    r[0] = res.status; r[1] = res.arg; r[2] = res.nodes_used; r[3] = res.mut_n; r[4] = res.mig_n;
    a.rng_out[i * 4 + 0] = g.sh; a.rng_out[i * 4 + 1] = g.sl; a.rng_out[i * 4 + 2] = g.ih; a.rng_out[i * 4 + 3] = g.il;
    a.n_rec[i] = res.status == VGX_GW_OK ? lg.n : 0;
}

__global__ void __launch_bounds__(256) vgxl_bin_kernel(VgxLnLaunch a, int stage) {
    extern __shared__ int32_t hist[];      // [P][V] cells, then (stage) variant_of [H]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    int64_t n = a.n_rec[row];
    const int64_t cap = a.desc[row].rec_cap;
    n = n < 0 ? 0 : (n > cap ? cap : n);                    // (never past the replicate's log)
    const int32_t T = a.T, P = (int32_t)a.P, H = (int32_t)a.H, V = a.V, cells = P * V;
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
                int32_t cell[2], sign[2];
                const int k = vgx_ln_deltas(c, P, H, V, vo, cell, sign);
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

// one thread per (replicate, population, class) column, consecutive threads consecutive classes: every step of the suffix sum
// reads and writes whole lines
__global__ void __launch_bounds__(256) vgxl_scan_kernel(VgxLnLaunch a) {
    const int64_t cells = a.P * a.V, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.m * cells) return;
    const int64_t row = idx / cells, cell = idx % cells;
    vgx_ln_scan_column(a.val + row * a.T * cells + cell, a.fin + idx, a.T, cells);
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ln_walk(const VgxLnLaunch *a, hipStream_t s) {
    if (a->m <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxl_walk_kernel, dim3((unsigned)a->m), dim3(64), 0, s, *a);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ln_bin(const VgxLnLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_rec <= 0) return hipSuccess;
    if (vgx_prev_lds_bytes(a->P, a->V) > VGX_PREV_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const bool stage = vgx_prev_stage_map(a->P, a->V, a->H);
    const int64_t lds = vgx_prev_lds_bytes(a->P, a->V) + (stage ? 4 * a->H : 0);
    const int64_t all_tiles = (a->max_rec + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxl_bin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxl_bin_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ln_scan(const VgxLnLaunch *a, hipStream_t s) {
    const int64_t cols = a->m * a->P * a->V;
    if (cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxl_scan_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, *a);
    return hipGetLastError();
}
