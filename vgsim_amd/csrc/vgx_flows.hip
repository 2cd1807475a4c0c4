// vgx_flows.hip — new infections per time bin, source population, destination population and variant class of every selected
// replicate of a direct ensemble on the device (vgx_get_flows), and the same rule and tile walk compiled for the host
// (vgx_test_flows).  DESIGN.md §23.
//
// The geometry and the record loads of vgx_incidence.hip: a workgroup of 256 threads takes one replicate and a TILE of
// consecutive events, reads the log in place (three 8-byte loads per lane), finds the bin of its first event by a search in the
// replicate's cuts, and at every bin change and at the tile's end adds the nonzero cells it keeps in LDS to the bin's block in
// device memory with 32-bit integer atomics and clears them.  What it keeps is the form (vgx_flows.h): all P * P * V cells
// (dense), or the P * V cells of the diagonal (split), a record off the diagonal then adding 1 to its cell in device memory at
// once.  variant_of is staged in LDS behind the cells when it fits.  All arithmetic is integer: the block does not depend on the
// form, the tile size or the launch geometry.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_flows.h"

namespace {

template <int FORM>
__global__ void __launch_bounds__(256) vgxf_count_kernel(VgxFlowLaunch a, int stage) {
    extern __shared__ int32_t hist[];      // dense: [P][P][V] cells, split: [P][V]; then (stage) variant_of [hapNum]
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_ev[row], T = a.T, P = a.P, V = a.V, cells = P * P * V;
    const int32_t kept = FORM == VGX_FLOW_DENSE ? cells : P * V;
    const int32_t *cut = a.cut + row * (int64_t)(T + 1);   // (uniform addresses: every thread reads the same cuts)
    const int2 *lg = (const int2 *)(a.log + a.rep[row] * a.evcap * 6);   // 8-byte aligned: 24-byte records from a 256-byte aligned base
    int32_t *out = a.counts + row * (int64_t)T * cells;
    const int32_t *vo = a.variant_of;
    bool clean = false;                    // the cells are zeroed and the map staged before the first tile that counts
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t pos, hi;
        vgx_inc_clip(cut, T, (int32_t)t0, e1, pos, hi);
        if (pos >= hi) continue;           // (the whole workgroup: the tile lies outside the window)
        if (!clean) {
            for (int i = tid; i < kept; i += 256) hist[i] = 0;
            if (stage) {
                int32_t *map = hist + kept;
                for (int i = tid; i < a.hapNum; i += 256) map[i] = vo[i];
                vo = map;
            }
            clean = true;
            __syncthreads();
        }
        while (pos < hi) {
            const int32_t b = vgx_inc_bin(cut, T, pos);
            const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
            int32_t *dstb = out + (int64_t)b * cells;
            for (int32_t e = pos + tid; e < end; e += 256) {
                const int2 r0 = lg[(int64_t)e * 3], r1 = lg[(int64_t)e * 3 + 1], r2 = lg[(int64_t)e * 3 + 2];
                const int32_t c[5] = {r0.x, r0.y, r1.x, r1.y, r2.x};
                int32_t src, dst, cls;
                if (!vgx_flow_cell(c, P, a.hapNum, vo, a.within, src, dst, cls)) continue;
                if (FORM == VGX_FLOW_DENSE) atomicAdd(&hist[vgx_flow_index(P, V, src, dst, cls)], 1);
                else if (src == dst) atomicAdd(&hist[src * V + cls], 1);
                else atomicAdd(&dstb[vgx_flow_index(P, V, src, dst, cls)], 1);
            }
            __syncthreads();
            for (int i = tid; i < kept; i += 256) {
                const int32_t v = hist[i];
                if (v) { atomicAdd(&dstb[FORM == VGX_FLOW_DENSE ? i : vgx_flow_diag_index(P, V, i)], v); hist[i] = 0; }
            }
            __syncthreads();
            pos = end;
        }
    }
}

template <int FORM>
hipError_t launch(const VgxFlowLaunch *a, hipStream_t s) {
    const bool stage = vgx_flow_stage_map(FORM, a->P, a->V, a->hapNum);
    const int64_t lds = vgx_flow_lds_bytes(FORM, a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxf_count_kernel<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxf_count_kernel<FORM>, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_flow_count(const VgxFlowLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if ((a->form != VGX_FLOW_DENSE && a->form != VGX_FLOW_SPLIT) || vgx_flow_form(a->form, a->P, a->V) != a->form || a->tile < 1)
        return hipErrorInvalidValue;
    return a->form == VGX_FLOW_DENSE ? launch<VGX_FLOW_DENSE>(a, s) : launch<VGX_FLOW_SPLIT>(a, s);
}

// ---- the host instance: the same cell, cuts, bins and tile walk on a chain given as arrays (no device, no engine)
extern "C" int vgx_test_flows(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                              const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                              const double *edges, int64_t T, const int32_t *variant_of, int64_t V, int32_t within, int64_t tile, int64_t form,
                              int32_t *counts, int64_t *outside, int64_t *form_ran, char *errbuf, int64_t errcap) {
    auto fail = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!edges || !variant_of || !counts || !outside) return fail("vgx_test_flows: null argument");
    if (T < 1 || T >= VGX_FLOW_MAX_BINS) return fail("vgx_test_flows: T = " + std::to_string(T) + " must be at least 1 and below 2^24");
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(edges[k])) return fail("vgx_test_flows: edges[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(edges[k - 1] < edges[k])) return fail("vgx_test_flows: edges must increase strictly (edges[" + std::to_string(k) + "])");
    }
    if (P < 1 || hapNum < 1 || P > INT32_MAX || hapNum > INT32_MAX) return fail("vgx_test_flows: bad dimensions");
    if (V < 1 || V > INT32_MAX) return fail("vgx_test_flows: V = " + std::to_string(V) + " must be at least 1");
    if (form != VGX_FLOW_AUTO && form != VGX_FLOW_DENSE && form != VGX_FLOW_SPLIT)
        return fail("vgx_test_flows: form = " + std::to_string(form) + " is none of 0 (automatic), 1 (dense), 2 (split)");
    const int ran = vgx_flow_form((int)form, P, V);
    if (!ran) {
        char why[256];
        vgx_flow_refusal((int)form, P, V, why, sizeof why);
        return fail(std::string("vgx_test_flows: ") + why);
    }
    for (int64_t h = 0; h < hapNum; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return fail("vgx_test_flows: variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " +
                        std::to_string(V) + ")");
    if (n_ev < 0 || n_ev >= VGX_FLOW_MAX_EVENTS) return fail("vgx_test_flows: a chain of " + std::to_string(n_ev) + " events (2^30 or more)");
    if (n_ev > 0 && (!times || !types || !haplotypes || !populations || !newHaplotypes || !newPopulations))
        return fail("vgx_test_flows: null event column");
    if (tile < 0) return fail("vgx_test_flows: tile must not be negative");
    if (tile == 0) tile = VGX_FLOW_TILE_DEFAULT;
    const int64_t cells = P * P * V;   // (P * V <= 2^14 and P <= 2^14: below 2^28)
    if (T * cells >= ((int64_t)1 << 40)) return fail("vgx_test_flows: block too large");
    std::vector<int32_t> log((size_t)n_ev * 5);
    for (int64_t e = 0; e < n_ev; e++) {
        const int64_t v[5] = {types[e], haplotypes[e], populations[e], newHaplotypes[e], newPopulations[e]};
        for (int c = 0; c < 5; c++) {
            if (v[c] < INT32_MIN || v[c] > INT32_MAX) return fail("vgx_test_flows: log value outside 32 bits");
            log[(size_t)(e * 5 + c)] = (int32_t)v[c];
        }
    }
    std::vector<int32_t> cut((size_t)(T + 1));
    VgxIncCutter ct{edges, T, cut.data()};
    for (int64_t e = 0; e < n_ev; e++) ct.event(e, times[e]);
    ct.finish(n_ev);
    outside[0] = cut[0];
    outside[1] = n_ev - cut[(size_t)T];
    if (form_ran) *form_ran = ran;
    for (int64_t i = 0; i < T * cells; i++) counts[i] = 0;
    std::vector<int32_t> hist((size_t)(vgx_flow_lds_bytes(ran, P, V) / 4), 0);
    for (int64_t t0 = 0; t0 < n_ev; t0 += tile)
        vgx_flow_tile_host(ran, log.data(), cut.data(), (int32_t)T, (int32_t)P, (int32_t)hapNum, (int32_t)V, variant_of, within, (int32_t)t0,
                           (int32_t)std::min<int64_t>(t0 + tile, n_ev), hist.data(), counts);
    return VGX_OK;
}
