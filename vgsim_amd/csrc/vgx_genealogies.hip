// vgx_genealogies.hip — the backward pass of every replicate of a direct ensemble on the device (vgx_get_genealogies).
//
// The walk (vgx_gwalk.h) is one long dependent chain per replicate with data-dependent branches, so a replicate is one lane
// of work: every working lane reads its own replicate's log in place (r_evcols, walked back from ev_ptr - 1), keeps its compartment table,
// lineage arena and outputs in workspace of its own, and shares nothing with other lanes or workgroups (the per-XCD L2s
// never see a line written by two CUs).  Log records are prefetched VGX_GW_CHUNK at a time into LDS: one round trip to
// HBM per chunk instead of per event.  Event times are not formed here: nodes and records carry event indices, which the
// host maps through its clock.  Two layouts of the same walk: one replicate per lane (vgx_genealogies_io.layout = 0) and one
// replicate per wavefront, lane 0 working (layout = 1): the latter is the faster one measured (the walk is latency-bound; a
// wavefront's one address per load beats 64 scattered ones, and 4096 wavefronts spread over every CU).
#include <hip/hip_runtime.h>
#include "vgx_gwalk.h"
#include "vgx_gwalk_lds.h"

namespace {

using LdsReader = VgxGwLdsReader;

template <bool WAVE>
__global__ void __launch_bounds__(64) vgxg_walk_kernel(VgxGwLaunch a) {
    __shared__ int32_t buf[VGX_GW_CHUNK * 6 * 64];
    const int lane = (int)threadIdx.x;
    const int64_t i = WAVE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 64 + lane;
    if ((WAVE && lane != 0) || i >= a.n) return;
    const VgxGwDesc d = a.desc[i];
    VgxGwRep w;
    w.n_ev = d.n_ev; w.sCounter = d.sCounter; w.H = a.H; w.tsize = d.tsize;
    w.key = a.key + d.tab_off; w.cnt = a.cnt + d.tab_off;
    w.base = a.base + d.tab_off; w.len = a.len + d.tab_off; w.lcap = a.lcap + d.tab_off;
    w.arena = a.arena + d.arena_off; w.arena_cap = d.arena_cap;
    w.tree = a.tree + d.node_off; w.tree_pop = a.tree_pop + d.node_off; w.node_ev = a.node_ev + d.node_off;
    w.mut_cap = d.mut_cap;
    w.mut_node = a.mut_node + d.mut_off; w.mut_AS = a.mut_AS + d.mut_off; w.mut_DS = a.mut_DS + d.mut_off;
    w.mut_site = a.mut_site + d.mut_off; w.mut_ev = a.mut_ev + d.mut_off;
    w.mig_cap = d.mig_cap;
    w.mig_node = a.mig_node + d.mig_off; w.mig_old = a.mig_old + d.mig_off; w.mig_new = a.mig_new + d.mig_off;
    w.mig_ev = a.mig_ev + d.mig_off;
    LdsReader rd{a.log + d.rep * a.evcap * 6, d.n_ev, buf + lane, -1};
    VgxGwResult res{};
    VgxPcg64 g{d.rng[0], d.rng[1], d.rng[2], d.rng[3]};
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
        vgx_gw_walk(w, rd, g, res);
    }
    int64_t *r = a.res + i * 5;
    r[0] = res.status; r[1] = res.arg; r[2] = res.nodes_used; r[3] = res.mut_n; r[4] = res.mig_n;
    a.rng_out[i * 4 + 0] = g.sh; a.rng_out[i * 4 + 1] = g.sl; a.rng_out[i * 4 + 2] = g.ih; a.rng_out[i * 4 + 3] = g.il;
}

// sizing pass: MUTATION and MIGRATION events in [0, n_ev) of every selected replicate (one workgroup per replicate)
__global__ void __launch_bounds__(256) vgxg_count_kernel(const int32_t *log, int64_t evcap, const int64_t *reps, const int64_t *n_ev,
                                                         int64_t *out) {
    __shared__ unsigned long long tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const int32_t *lg = log + reps[blockIdx.x] * evcap * 6;
    const int64_t n = n_ev[blockIdx.x];
    unsigned long long mu = 0, mi = 0;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        const int32_t t = lg[e * 6];
        mu += t == VGX_GW_MUTATION;
        mi += t == VGX_GW_MIGRATION;
    }
    atomicAdd(&tot[0], mu);
    atomicAdd(&tot[1], mi);
    __syncthreads();
    if (threadIdx.x < 2) out[blockIdx.x * 2 + threadIdx.x] = (int64_t)tot[threadIdx.x];
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_gw_count(const int32_t *log, int64_t evcap, const int64_t *reps,
                                                                          const int64_t *n_ev, int64_t n, int64_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxg_count_kernel, dim3((unsigned)n), dim3(256), 0, s, log, evcap, reps, n_ev, out);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_gw_walk(const VgxGwLaunch *a, int wave, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    if (wave) hipLaunchKernelGGL(vgxg_walk_kernel<true>, dim3((unsigned)a->n), dim3(64), 0, s, *a);
    else hipLaunchKernelGGL(vgxg_walk_kernel<false>, dim3((unsigned)((a->n + 63) / 64)), dim3(64), 0, s, *a);
    return hipGetLastError();
}
