// vgx_incidence.hip — event counts per time bin, population and channel of every selected replicate of a direct ensemble on the
// device (vgx_get_incidence), and the same rule and tile walk compiled for the host (vgx_test_incidence).  DESIGN.md §16.
//
// One kernel.  A workgroup of 256 threads takes one replicate and a TILE of consecutive events of its chain, so that a single
// long chain spreads over the whole device.  It reads the log in place, consecutive lanes consecutive records (three 8-byte
// loads per lane: every byte of a fetched line is used).  A bin is a contiguous range of event indices (vgx_incidence.h), so
// the workgroup finds the bin of its first event by a search in the replicate's cuts, counts into a histogram of P * 7 int32
// cells in LDS with LDS atomics, and at every bin change and at the tile's end adds the nonzero cells to the block in device
// memory with 32-bit integer atomics and clears them.  Global atomics of different workgroups meet only at the bins that
// straddle a tile border.  All arithmetic is integer: the block does not depend on the tile size or the launch geometry.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_incidence.h"

namespace {

__global__ void __launch_bounds__(256) vgxn_count_kernel(VgxIncLaunch a) {
    extern __shared__ int32_t hist[];      // [P][7]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_ev[row], T = a.T, P = a.P, cells = P * VGX_INC_CHANNELS;
    const int32_t *cut = a.cut + row * (int64_t)(T + 1);   // (uniform addresses: every thread reads the same cuts)
    const int2 *lg = (const int2 *)(a.log + a.rep[row] * a.evcap * 6);   // 8-byte aligned: 24-byte records from a 256-byte aligned base
    int32_t *out = a.counts + row * (int64_t)T * cells;
    bool clean = false;                    // the histogram is zeroed before the first tile that counts
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t pos, hi;
        vgx_inc_clip(cut, T, (int32_t)t0, e1, pos, hi);
        if (pos >= hi) continue;           // (the whole workgroup: the tile lies outside the window)
        if (!clean) {
            for (int i = tid; i < cells; i += 256) hist[i] = 0;
            clean = true;
            __syncthreads();
        }
        while (pos < hi) {
            const int32_t b = vgx_inc_bin(cut, T, pos);
            const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
            for (int32_t e = pos + tid; e < end; e += 256) {
                const int2 r0 = lg[(int64_t)e * 3], r1 = lg[(int64_t)e * 3 + 1], r2 = lg[(int64_t)e * 3 + 2];
                const int32_t c[5] = {r0.x, r0.y, r1.x, r1.y, r2.x};
                int32_t cell[2];
                const int k = vgx_inc_cells(c, P, a.hapNum, a.mask, cell);
                if (k > 0) atomicAdd(&hist[cell[0]], 1);
                if (k > 1) atomicAdd(&hist[cell[1]], 1);
            }
            __syncthreads();
            int32_t *dst = out + (int64_t)b * cells;
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

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_inc_count(const VgxIncLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    const int64_t lds = vgx_inc_lds_bytes(a->P);
    if (lds > VGX_INC_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxn_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxn_count_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a);
    return hipGetLastError();
}

// ---- the host instance: the same cells, cuts, bins and tile walk on a chain given as arrays (no device, no engine)
extern "C" int vgx_test_incidence(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                                  const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                                  const double *edges, int64_t T, const uint32_t *hap_mask, int64_t tile, int32_t *counts, int64_t *outside,
                                  char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!edges || !counts || !outside) return fail("vgx_test_incidence: null argument");
    if (T < 1 || T >= VGX_INC_MAX_BINS) return fail("vgx_test_incidence: T = " + std::to_string(T) + " must be at least 1 and below 2^24");
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(edges[k])) return fail("vgx_test_incidence: edges[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(edges[k - 1] < edges[k])) return fail("vgx_test_incidence: edges must increase strictly (edges[" + std::to_string(k) + "])");
    }
    if (P < 1 || hapNum < 1 || P > INT32_MAX / VGX_INC_CHANNELS || hapNum > INT32_MAX) return fail("vgx_test_incidence: bad dimensions");
    if (vgx_inc_lds_bytes(P) > VGX_INC_LDS_MAX)
        return fail("vgx_test_incidence: " + std::to_string(P) + " populations need " + std::to_string(vgx_inc_lds_bytes(P)) +
                    " bytes of counters, above the " + std::to_string((int64_t)VGX_INC_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    if (n_ev < 0 || n_ev >= VGX_INC_MAX_EVENTS) return fail("vgx_test_incidence: a chain of " + std::to_string(n_ev) + " events (2^30 or more)");
    if (n_ev > 0 && (!times || !types || !haplotypes || !populations || !newHaplotypes || !newPopulations))
        return fail("vgx_test_incidence: null event column");
    if (tile < 0) return fail("vgx_test_incidence: tile must not be negative");
    if (tile == 0) tile = VGX_INC_TILE_DEFAULT;
    if (T * P * VGX_INC_CHANNELS >= ((int64_t)1 << 40)) return fail("vgx_test_incidence: block too large");
    std::vector<int32_t> log((size_t)n_ev * 5);
    for (int64_t e = 0; e < n_ev; e++) {
        const int64_t v[5] = {types[e], haplotypes[e], populations[e], newHaplotypes[e], newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_incidence: log value outside 32 bits");
            log[(size_t)(e * 5 + c)] = (int32_t)v[c];
        }
    }
    std::vector<int32_t> cut((size_t)(T + 1));
    VgxIncCutter ct{edges, T, cut.data()};
    for (int64_t e = 0; e < n_ev; e++) ct.event(e, times[e]);
    ct.finish(n_ev);
    outside[0] = cut[0];
    outside[1] = n_ev - cut[(size_t)T];
    const int64_t cells = P * VGX_INC_CHANNELS;
    for (int64_t i = 0; i < T * cells; i++) counts[i] = 0;
    std::vector<int32_t> hist((size_t)cells, 0);
    for (int64_t t0 = 0; t0 < n_ev; t0 += tile)
        vgx_inc_tile_host(log.data(), cut.data(), (int32_t)T, (int32_t)P, (int32_t)hapNum, hap_mask, (int32_t)t0,
                          (int32_t)std::min<int64_t>(t0 + tile, n_ev), hist.data(), counts);
    return VGX_OK;
}
