// vgx_tau_genealogies.hip — the backward pass of every replicate of a TAU ensemble on the device (vgx_get_tau_genealogies), the
// host side of that call, and the same code compiled for the host (vgx_test_tau_genealogy_walk, vgx_test_hypergeometric).
//
// The tau kernels append a step's rows in whatever order their threads get there, one row per drawn transmission, mutant or
// migrant; the backward pass (vgx_gwalk_tau.h) walks the reference's rows: one per channel, in a fixed order.  Two kernels:
//   CANONICALISE, the data-parallel part: one workgroup of 256 threads per replicate works through the step ranges [m0, m1) of its
//     block of t_mev in place.  Per step: the two-word key of every raw row and its index within the step go to LDS, a bitonic
//     sort orders them (ties by index: the first row of a channel speaks for it), a head flag scan numbers the distinct keys, the
//     heads write compact 32-byte rows into the pass's workspace and every raw row adds its `num` to its channel's row.  t_mev is
//     only read.  A step with more raw rows than the sort holds (VGX_GT_STEP_ROWS_MAX) gives its replicate VGX_GW_STEP_ROWS.
//   WALK: one replicate per wavefront, lane 0 working (the layout DESIGN.md §10 measured faster for the direct walk): pre-pass
//     over the canonical rows and the prefix, counts of the touched compartments from the dense final state t_I, the walk from the
//     last own step back, then the prefix, then the closing pass.  The prefix (the model's chain before the tau call) is flattened
//     into the same 32-byte rows once per call and shared by every replicate that did not restart.
// Nodes and records carry the chain's event index; the host maps it to the prefix's event / row times or the step times of tau_log.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_gwalk_tau.h"
#include "vgx_tau_chain.h"

namespace {

// ---- canonicalise ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool key_after(uint64_t ah, uint64_t al, uint16_t ai, uint64_t bh, uint64_t bl, uint16_t bi) {
    return ah != bh ? ah > bh : (al != bl ? al > bl : ai > bi);
}

__global__ void __launch_bounds__(256) vgxtg_canon_kernel(VgxGtCanonLaunch a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    // all of it in the dynamic region, every carve a multiple of 16 bytes (a static would shift the region's base off the
    // alignment of the 8-byte key accesses): keys hi, keys lo, row indices, then 64 bytes of scan and flag scratch
    uint64_t *khi = (uint64_t *)lds_raw, *klo = khi + a.cap;
    uint16_t *kid = (uint16_t *)(klo + a.cap);
    unsigned long long *s_push = (unsigned long long *)(kid + a.cap);
    int *s_wtot = (int *)(s_push + 4);
    int &s_bad = s_wtot[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VgxGtCanonDesc d = a.desc[blockIdx.x];
    const int64_t *mev = a.mev + d.rep * a.mev_cap * 6;
    const int32_t *mr = a.mrange + d.step_off;
    VgxGtRow *can = a.can + d.row_off;
    int32_t *coff = a.can_off + d.off_off;
    int64_t out = 0, status = VGX_GW_OK, arg = 0;
    unsigned long long pushes = 0;
    for (int64_t k = 0; k < d.n_steps; k++) {
        const int64_t m0 = mr[k];
        const int n = (int)(mr[k + 1] - m0);
        if (tid == 0) coff[k] = (int32_t)out;
        if (n <= 0) continue;
        if (n > a.cap) { status = VGX_GW_STEP_ROWS; arg = k; break; }
        int N = 2;
        while (N < n) N <<= 1;
        if (tid == 0) s_bad = 0;
        __syncthreads();
        for (int i = tid; i < N; i += 256) {
            uint64_t hi = ~0ull, lo = ~0ull;
            if (i < n) {
                const int64_t *r = mev + (m0 + i) * 6;
                if (!vgx_gt_row_ok(a.P, a.H, r[0], r[1], r[2], r[3], r[4], r[5]) || r[1] < 0 || r[1] >= VGX_GT_ROW_DIRECT) s_bad = 1;
                vgx_gt_row_key(a.sites, r[1], r[2], r[3], r[4], r[5], hi, lo);
            }
            khi[i] = hi; klo[i] = lo; kid[i] = (uint16_t)(i < n ? i : 0xFFFF);
        }
        __syncthreads();
        if (s_bad) { status = VGX_GW_BAD_ROW; arg = k; break; }
        for (int k2 = 2; k2 <= N; k2 <<= 1) {
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < N / 2; t += 256) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                    const bool up = (i & k2) == 0;
                    const uint64_t ah = khi[i], al = klo[i], bh = khi[l], bl = klo[l];
                    const uint16_t ai = kid[i], bi = kid[l];
                    if (key_after(ah, al, ai, bh, bl, bi) == up) {
                        khi[i] = bh; klo[i] = bl; kid[i] = bi;
                        khi[l] = ah; klo[l] = al; kid[l] = ai;
                    }
                }
                __syncthreads();
            }
        }
        // every thread a contiguous run of the sorted rows: heads before it (scan), then slot = heads up to and including the row - 1
        const int per = (n + 255) / 256, i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
        auto head = [&](int i) { return i == 0 || khi[i] != khi[i - 1] || klo[i] != klo[i - 1]; };
        int mine = 0;
        for (int i = i0; i < i1; i++) mine += head(i) ? 1 : 0;
        int incl = mine;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const int u = __shfl_up(incl, dd);
            if (lane >= dd) incl += u;
        }
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        int before = incl - mine, total = 0;
        for (int wv = 0; wv < 4; wv++) {
            if (wv < wave) before += s_wtot[wv];
            total += s_wtot[wv];
        }
        int pos = before;
        for (int i = i0; i < i1; i++) {
            if (!head(i)) continue;
            const int64_t *r = mev + (m0 + kid[i]) * 6;
            VgxGtRow row;
            row.num = 0; row.type = (int32_t)r[1]; row.hap = (int32_t)r[2]; row.pop = (int32_t)r[3]; row.nh = (int32_t)r[4]; row.np = (int32_t)r[5];
            row.pad = 0;
            can[out + pos] = row;
            pos++;
        }
        __syncthreads();   // the heads' rows are written before any thread of the workgroup adds to them
        pos = before;
        for (int i = i0; i < i1; i++) {
            pos += head(i) ? 1 : 0;
            atomicAdd((unsigned long long *)&can[out + pos - 1].num, (unsigned long long)mev[(m0 + kid[i]) * 6]);
        }
        __syncthreads();
        pos = before;
        for (int i = i0; i < i1; i++) {
            if (!head(i)) continue;
            // (the sums were formed by atomics at the L2: read there, not from a line this CU may still hold)
            const int64_t num = __hip_atomic_load(&can[out + pos].num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pushes += (unsigned long long)vgx_gt_row_pushes(mev[(m0 + kid[i]) * 6 + 1], num, d.sCounter);
            pos++;
        }
        out += total;
        __syncthreads();   // (s_wtot and the keys are rewritten by the next step)
    }
    // the pushes of all threads
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) pushes += __shfl_xor(pushes, dd);
    if (lane == 0) s_push[wave] = pushes;
    __syncthreads();
    if (tid == 0) {
        coff[d.n_steps] = (int32_t)out;
        VgxGtCanonStat st;
        st.status = status; st.arg = arg; st.n_rows = out;
        st.pushes = (int64_t)(s_push[0] + s_push[1] + s_push[2] + s_push[3]);
        a.stat[blockIdx.x] = st;
    }
}

// sizing: sums of min(num, sCounter) over a replicate's raw MUTATION rows, MIGRATION rows, and all rows that can push a lineage
__global__ void __launch_bounds__(256) vgxtg_count_kernel(const int64_t *mev, int64_t mev_cap, const int64_t *reps, const int64_t *n_rows,
                                                          const int64_t *sC, int64_t *out) {
    __shared__ unsigned long long tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t *rows = mev + reps[blockIdx.x] * mev_cap * 6;
    const int64_t n = n_rows[blockIdx.x], s = sC[blockIdx.x];
    unsigned long long mu = 0, mi = 0, pu = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int64_t num = rows[i * 6], t = rows[i * 6 + 1];
        const unsigned long long v = (unsigned long long)(num < 0 ? 0 : (num < s ? num : s));
        mu += t == VGX_GW_MUTATION ? v : 0;
        mi += t == VGX_GW_MIGRATION ? v : 0;
        pu += (t == VGX_GW_BIRTH || t == VGX_GW_SAMPLING || t == VGX_GW_MUTATION || t == VGX_GW_MIGRATION) ? v : 0;
    }
    atomicAdd(&tot[0], mu);
    atomicAdd(&tot[1], mi);
    atomicAdd(&tot[2], pu);
    __syncthreads();
    if (threadIdx.x < 3) out[blockIdx.x * 3 + threadIdx.x] = (int64_t)tot[threadIdx.x];
}

// ---- walk ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) vgxtg_walk_kernel(VgxGtLaunch a) {
    const int64_t i = (int64_t)blockIdx.x;
    if (threadIdx.x != 0 || i >= a.n) return;
    const VgxGtDesc d = a.desc[i];
    VgxGwRep w;
    w.n_ev = d.n_pre + d.n_steps; w.sCounter = d.sCounter; w.H = a.H; w.tsize = d.tsize;
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
    const VgxGtChain c{a.pre, a.pre_off, d.n_pre, a.can + d.row_off, a.can_off + d.off_off, d.n_steps};
    VgxGtGen gen{{d.rng[0], d.rng[1], d.rng[2], d.rng[3]}, (int32_t)d.has32, (uint32_t)d.spare};
    VgxGwResult res{};
    if (d.sCounter < 2) res.status = VGX_GW_FEW_SAMPLES;   // (no workspace below two samples)
    else if (d.status != VGX_GW_OK) { res.status = d.status; res.arg = d.arg; }
    else res.status = vgx_gt_prepass(w, c);
    if (res.status == VGX_GW_OK) {
        const int64_t PH = a.P * a.H;
        const int32_t *I = a.I + d.rep * PH;
        for (int64_t s = 0; s < w.tsize; s++) {
            const int64_t k = w.key[s];
            if (k >= 0 && k < PH) w.cnt[s] = I[k];
        }
        vgx_gt_walk(w, c, a.fresh + d.node_off, gen, res);
    }
    int64_t *r = a.res + i * 5;
    r[0] = res.status; r[1] = res.arg; r[2] = res.nodes_used; r[3] = res.mut_n; r[4] = res.mig_n;
    uint64_t *g = a.rng_out + i * 6;
    g[0] = gen.g.sh; g[1] = gen.g.sl; g[2] = gen.g.ih; g[3] = gen.g.il; g[4] = (uint64_t)gen.has32; g[5] = gen.spare;
}

__global__ void __launch_bounds__(64) vgxtg_hyper_kernel(int64_t good, int64_t bad, int64_t sample, int64_t n, uint64_t *state, int64_t *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    VgxGtGen gen{{state[0], state[1], state[2], state[3]}, (int32_t)state[4], (uint32_t)state[5]};
    for (int64_t i = 0; i < n; i++) out[i] = vgx_gt_hypergeometric(gen, good, bad, sample);
    state[0] = gen.g.sh; state[1] = gen.g.sl; state[2] = gen.g.ih; state[3] = gen.g.il; state[4] = (uint64_t)gen.has32; state[5] = gen.spare;
}

// ---- host: a chain's events as rows, its capacities and the chain of a test hook: vgx_tau_chain.h
using namespace vgxtc;

hipError_t launch_canon(const VgxGtCanonLaunch *a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    const int lds = a->cap * 18 + 64;
    hipError_t err = hipFuncSetAttribute((const void *)vgxtg_canon_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtg_canon_kernel, dim3((unsigned)a->n), dim3(256), (size_t)lds, s, *a);
    return hipGetLastError();
}

}  // namespace

// the canonicalise and counting launches as vgx_tau_lineages.hip shares them (declared in vgx_tau_lineages.h)
extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tg_canon(const VgxGtCanonLaunch *a, hipStream_t s) { return launch_canon(a, s); }

// the walk launch as vgx_tau_tree_shapes.hip shares it
extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tg_walk(const VgxGtLaunch *a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxtg_walk_kernel, dim3((unsigned)a->n), dim3(64), 0, s, *a);
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tg_count(const int64_t *mev, int64_t mev_cap, const int64_t *reps, const int64_t *n_rows,
                                                                          const int64_t *sC, int64_t n, int64_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxtg_count_kernel, dim3((unsigned)n), dim3(256), 0, s, mev, mev_cap, reps, n_rows, sC, out);
    return hipGetLastError();
}

extern "C" int vgx_get_tau_genealogies(vgx_engine *e, vgx_tau_genealogies_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->node_off || !io->mut_off || !io->mig_off))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_genealogies: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (walks tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, PH = P * H, mev_cap = e->tau_mev_cap;
    const int64_t pre_ev = prefix ? prefix->ev_ptr : 0;
    if (pre_ev < 0 || pre_ev >= ((int64_t)1 << 30) ||
        (pre_ev > 0 && (!prefix->ev_times || !prefix->ev_types || !prefix->ev_haplotypes || !prefix->ev_populations || !prefix->ev_newHaplotypes ||
                        !prefix->ev_newPopulations)))
        return fail(e, VGX_ERR_ARG, me + "null prefix column");
    std::vector<char> with_prefix((size_t)n, 0);
    std::vector<int64_t> sC((size_t)n), raw((size_t)n), steps((size_t)n);
    bool any_prefix = false;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : e->ev_ptr0;
            if (s.restarts == 0 && first != pre_ev)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain continues a log of " + std::to_string(first) +
                                                " events, the prefix holds " + std::to_string(pre_ev));
            with_prefix[(size_t)i] = s.restarts == 0 && pre_ev > 0;
            any_prefix = any_prefix || with_prefix[(size_t)i];
            const auto &lg = e->tau_log[(size_t)r];
            for (size_t k = 0; k < lg.size(); k++)
                if (lg[k].m0 != (k ? lg[k - 1].m1 : 0) || lg[k].m1 < lg[k].m0)
                    return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": row ranges of its steps are not contiguous");
            const int64_t rows = lg.empty() ? 0 : lg.back().m1;
            if (rows > mev_cap) return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " logged more rows than its block holds");
            if (rows >= ((int64_t)1 << 30) || (int64_t)lg.size() >= ((int64_t)1 << 30) || 2 * s.sCounter > ((int64_t)1 << 31))
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": chain too long");
            sC[(size_t)i] = s.sCounter;
            raw[(size_t)i] = rows;
            steps[(size_t)i] = (int64_t)lg.size();
        }
    }
    FlatChain pre;
    pre.off.assign(1, 0);
    FlatCaps pre_caps;
    if (any_prefix) {
        const EventCols ev{pre_ev, prefix->ev_times, prefix->ev_types, prefix->ev_haplotypes, prefix->ev_populations, prefix->ev_newHaplotypes, prefix->ev_newPopulations};
        const RowCols mv{prefix->mev_rows, prefix->mev_num, prefix->mev_times, prefix->mev_types, prefix->mev_haplotypes, prefix->mev_populations,
                         prefix->mev_newHaplotypes, prefix->mev_newPopulations};
        if (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np)) return fail(e, VGX_ERR_ARG, me + "null prefix multievent column");
        const std::string why = flatten(ev, pre_ev, mv, P, H, pre);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + "prefix: " + why);
    }
    pre_caps.of(pre);
    const int64_t pre_rows = (int64_t)pre.rows.size();
    if (n == 0) return VGX_OK;
    HIPCHECK(e, hipSetDevice(e->device));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    typedef std::unique_ptr<char, void (*)(char *)> Hold;

    // raw sums of min(num, sCounter): MUTATION rows, MIGRATION rows, rows that can push a lineage (both calls: the sizing call's
    // capacities and the bound of a pass's workspace)
    std::vector<int64_t> cnt((size_t)n * 3);
    {
        char *ws = nullptr;
        hipError_t er = hipMalloc((void **)&ws, (size_t)n * 8 * 6);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc: " + hipGetErrorString(er));
        Hold hold(ws, dev_free);
        int64_t *d_rep = (int64_t *)ws, *d_n = d_rep + n, *d_s = d_rep + 2 * n, *d_out = d_rep + 3 * n;
        HIPCHECK(e, hipMemcpyAsync(d_rep, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(d_n, raw.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(d_s, sC.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(vgxtg_count_kernel, dim3((unsigned)n), dim3(256), 0, e->stream, (const int64_t *)e->t_mev.p, mev_cap, d_rep, d_n, d_s, d_out);
        HIPCHECK(e, hipGetLastError());
        hipError_t sr = hipStreamSynchronize(e->stream);
        if (sr != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(sr));
        HIPCHECK(e, hipMemcpy(cnt.data(), d_out, (size_t)n * 24, hipMemcpyDeviceToHost));
    }
    auto nodes_of = [&](int64_t i) { return sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0; };
    auto mut_need = [&](int64_t i) {
        return cnt[(size_t)(3 * i)] + (with_prefix[(size_t)i] ? pre_caps.direct_mut + pre_caps.mut(sC[(size_t)i]) : 0);
    };
    auto mig_need = [&](int64_t i) {
        return cnt[(size_t)(3 * i + 1)] + (with_prefix[(size_t)i] ? pre_caps.direct_mig + pre_caps.mig(sC[(size_t)i]) : 0) + nodes_of(i);
    };
    if (!io->tree) {   // sizing
        io->node_off[0] = io->mut_off[0] = io->mig_off[0] = 0;
        for (int64_t i = 0; i < n; i++) {
            const bool few = sC[(size_t)i] < 2;
            io->node_off[i + 1] = io->node_off[i] + nodes_of(i);
            io->mut_off[i + 1] = io->mut_off[i] + (few ? 0 : mut_need(i));
            io->mig_off[i + 1] = io->mig_off[i] + (few ? 0 : mig_need(i));
        }
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    if (!io->rng_state || !io->tree_pop || !io->times || !io->status || !io->status_arg || !io->nodes_used || !io->mut_n || !io->mig_n ||
        !io->rng_out || (io->mut_off[n] > 0 && (!io->mut_node || !io->mut_AS || !io->mut_DS || !io->mut_site || !io->mut_time)) ||
        (io->mig_off[n] > 0 && (!io->mig_node || !io->mig_old || !io->mig_new || !io->mig_time)))
        return fail(e, VGX_ERR_ARG, me + "null output");
    for (int64_t i = 0; i < n; i++)
        if (io->node_off[i + 1] - io->node_off[i] < nodes_of(i) || io->mut_off[i + 1] < io->mut_off[i] || io->mig_off[i + 1] < io->mig_off[i])
            return fail(e, VGX_ERR_ARG, me + "output capacities smaller than the sizing call gave");

    // the prefix on the device, once per call: [rows | offsets]
    const int64_t q_rows = 0, q_off = up8(pre_rows * 32 + 32), q_total = q_off + up8((int64_t)pre.off.size() * 4);
    char *qws = nullptr;
    hipError_t er = hipMalloc((void **)&qws, (size_t)q_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(q_total) + " bytes: " + hipGetErrorString(er));
    Hold qhold(qws, dev_free);
    if (pre_rows) HIPCHECK(e, hipMemcpy(qws + q_rows, pre.rows.data(), (size_t)pre_rows * 32, hipMemcpyHostToDevice));
    HIPCHECK(e, hipMemcpy(qws + q_off, pre.off.data(), pre.off.size() * 4, hipMemcpyHostToDevice));

    // passes: what a replicate can need at most, from its raw rows
    auto table_of = [&](int64_t rows) { return vgx_gw_table_size(rows, PH); };
    auto arena_of = [&](int64_t i, int64_t tsize, int64_t pushes) {
        const int64_t all = pushes + (with_prefix[(size_t)i] ? pre_caps.direct_push + pre_caps.push(sC[(size_t)i]) : 0);
        return std::min(all, (tsize / 2) * sC[(size_t)i]);
    };
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t rows = raw[(size_t)i] + (with_prefix[(size_t)i] ? pre_rows : 0), nodes = nodes_of(i);
        const int64_t tsize = nodes ? table_of(rows) : 0;
        bytes[(size_t)i] = raw[(size_t)i] * 32 + (steps[(size_t)i] + 1) * 8 + tsize * 28 + (nodes ? arena_of(i, tsize, cnt[(size_t)(3 * i + 2)]) : 0) * 4 +
                           nodes * 16 + (io->mut_off[i + 1] - io->mut_off[i]) * 20 + (io->mig_off[i + 1] - io->mig_off[i]) * 16 +
                           (int64_t)(sizeof(VgxGtDesc) + sizeof(VgxGtCanonDesc) + sizeof(VgxGtCanonStat)) + 2048;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        // ---- canonicalise: [desc | stat | step ranges | canonical row ranges | canonical rows]
        std::vector<VgxGtCanonDesc> cd((size_t)m);
        std::vector<int32_t> mrange;
        int64_t RO = 0, OO = 0, longest = 0;
        for (int64_t j = 0; j < m; j++) {
            const int64_t gi = i0 + j;
            const auto &lg = e->tau_log[(size_t)io->replicates[gi]];
            VgxGtCanonDesc &d = cd[(size_t)j];
            d.rep = io->replicates[gi]; d.n_steps = (int64_t)lg.size(); d.sCounter = sC[(size_t)gi];
            d.step_off = (int64_t)mrange.size(); d.row_off = RO; d.off_off = OO;
            for (const auto &st : lg) {
                mrange.push_back((int32_t)st.m0);
                longest = std::max(longest, std::min<int64_t>(st.m1 - st.m0, VGX_GT_STEP_ROWS_MAX));
            }
            mrange.push_back((int32_t)raw[(size_t)gi]);
            RO += raw[(size_t)gi];
            OO += d.n_steps + 1;
        }
        const int64_t c_desc = 0, c_stat = c_desc + up8(m * (int64_t)sizeof(VgxGtCanonDesc)), c_mr = c_stat + up8(m * (int64_t)sizeof(VgxGtCanonStat)),
                      c_off = c_mr + up8((int64_t)mrange.size() * 4), c_rows = c_off + up8(OO * 4), c_total = c_rows + up8(RO * 32 + 32);
        char *cws = nullptr;
        er = hipMalloc((void **)&cws, (size_t)c_total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(c_total) + " bytes: " + hipGetErrorString(er));
        Hold chold(cws, dev_free);
        VgxGtCanonLaunch ca{};
        ca.n = m;
        ca.desc = (const VgxGtCanonDesc *)(cws + c_desc);
        ca.mev = (const int64_t *)e->t_mev.p; ca.mev_cap = mev_cap;
        ca.mrange = (const int32_t *)(cws + c_mr);
        ca.P = P; ca.H = H; ca.sites = e->d.sites;
        ca.cap = 64;
        while (ca.cap < longest) ca.cap <<= 1;
        ca.can = (VgxGtRow *)(cws + c_rows); ca.can_off = (int32_t *)(cws + c_off); ca.stat = (VgxGtCanonStat *)(cws + c_stat);
        HIPCHECK(e, hipMemcpyAsync(cws + c_desc, cd.data(), (size_t)m * sizeof(VgxGtCanonDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_mr, mrange.data(), mrange.size() * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, launch_canon(&ca, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "canonicalise kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        std::vector<VgxGtCanonStat> stat((size_t)m);
        HIPCHECK(e, hipMemcpy(stat.data(), ca.stat, (size_t)m * sizeof(VgxGtCanonStat), hipMemcpyDeviceToHost));

        // ---- walk: [desc | res | rng | key | cnt | base | len | lcap | arena | fresh | node x3 | mut x5 | mig x4]
        std::vector<VgxGtDesc> dp((size_t)m);
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        for (int64_t j = 0; j < m; j++) {
            const int64_t gi = i0 + j;
            VgxGtDesc &d = dp[(size_t)j];
            const VgxGtCanonStat &st = stat[(size_t)j];
            d.rep = io->replicates[gi];
            d.n_pre = with_prefix[(size_t)gi] ? pre_ev : 0;
            d.n_steps = cd[(size_t)j].n_steps;
            d.sCounter = sC[(size_t)gi];
            d.status = st.status; d.arg = st.arg;
            const bool walk = d.sCounter >= 2 && st.status == VGX_GW_OK;
            d.tsize = walk ? table_of(st.n_rows + (with_prefix[(size_t)gi] ? pre_rows : 0)) : 0;
            d.arena_cap = walk ? arena_of(gi, d.tsize, st.pushes) : 0;
            d.mut_cap = io->mut_off[gi + 1] - io->mut_off[gi];
            d.mig_cap = io->mig_off[gi + 1] - io->mig_off[gi];
            d.row_off = cd[(size_t)j].row_off; d.off_off = cd[(size_t)j].off_off;
            for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[gi * 6 + k];
            d.has32 = io->rng_state[gi * 6 + 4] != 0; d.spare = (int64_t)(uint32_t)io->rng_state[gi * 6 + 5];
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            T += d.tsize; A += d.arena_cap; N += nodes_of(gi); M += d.mut_cap; G += d.mig_cap;
        }
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGtDesc)), o_rng = o_res + up8(m * 40), o_key = o_rng + up8(m * 48),
                      o_cnt = o_key + up8(T * 8), o_base = o_cnt + up8(T * 8), o_len = o_base + up8(T * 4), o_lcap = o_len + up8(T * 4),
                      o_arena = o_lcap + up8(T * 4), o_fresh = o_arena + up8(A * 4), o_out = o_fresh + up8(N * 4),
                      total = o_out + up8((3 * N + 5 * M + 4 * G) * 4);
        char *ws = nullptr;
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        Hold hold(ws, dev_free);
        VgxGtLaunch a{};
        a.n = m;
        a.desc = (const VgxGtDesc *)(ws + o_desc);
        a.pre = (const VgxGtRow *)(qws + q_rows); a.pre_off = (const int32_t *)(qws + q_off);
        a.can = ca.can; a.can_off = ca.can_off;
        a.I = (const int32_t *)e->t_I.p;
        a.P = P; a.H = H;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena); a.fresh = (int32_t *)(ws + o_fresh);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGtDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        hipLaunchKernelGGL(vgxtg_walk_kernel, dim3((unsigned)m), dim3(64), 0, e->stream, a);
        HIPCHECK(e, hipGetLastError());
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "walk kernel failed: " + hipGetErrorString(er));
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        std::vector<int64_t> res((size_t)m * 5);
        std::vector<uint64_t> rng((size_t)m * 6);
        std::vector<int32_t> out((size_t)(3 * N + 5 * M + 4 * G));
        HIPCHECK(e, hipMemcpy(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(rng.data(), a.rng_out, (size_t)m * 48, hipMemcpyDeviceToHost));
        if (!out.empty()) HIPCHECK(e, hipMemcpy(out.data(), o32, out.size() * 4, hipMemcpyDeviceToHost));
        hold.reset();
        chold.reset();
        // event indices -> times: the prefix's, then the step times of tau_log
        const auto t_host = std::chrono::steady_clock::now();
        const int32_t *h_tree = out.data(), *h_pop = h_tree + N, *h_nev = h_tree + 2 * N, *h_mu = h_tree + 3 * N, *h_mg = h_mu + 5 * M;
        std::vector<char> bad((size_t)m, 0);
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t j = j0; j < j1; j++) {
                const VgxGtDesc &d = dp[(size_t)j];
                const int64_t gi = i0 + j;
                const auto &lg = e->tau_log[(size_t)d.rep];
                const int64_t *r5 = res.data() + j * 5;
                io->status[gi] = r5[0]; io->status_arg[gi] = r5[1]; io->nodes_used[gi] = r5[2];
                io->mut_n[gi] = r5[0] == VGX_GW_OK ? r5[3] : 0;
                io->mig_n[gi] = r5[0] == VGX_GW_OK ? r5[4] : 0;
                for (int k = 0; k < 6; k++) io->rng_out[gi * 6 + k] = rng[(size_t)(j * 6 + k)];
                if (r5[0] != VGX_GW_OK) continue;
                bool ok = true;
                auto time_of = [&](int32_t ev) {
                    if (ev < 0) return 0.0;
                    if (ev < d.n_pre) return pre.time[(size_t)ev];
                    if (ev - d.n_pre < (int64_t)lg.size()) return lg[(size_t)(ev - d.n_pre)].time;
                    ok = false;
                    return 0.0;
                };
                const int64_t nodes = 2 * d.sCounter - 1, no = io->node_off[gi];
                for (int64_t k = 0; k < nodes; k++) {
                    io->tree[no + k] = h_tree[d.node_off + k];
                    io->tree_pop[no + k] = h_pop[d.node_off + k];
                    io->times[no + k] = time_of(h_nev[d.node_off + k]);
                }
                const int64_t mo = io->mut_off[gi];
                for (int64_t k = 0; k < r5[3]; k++) {
                    const int64_t q = d.mut_off + k;
                    io->mut_node[mo + k] = h_mu[q]; io->mut_AS[mo + k] = h_mu[M + q]; io->mut_DS[mo + k] = h_mu[2 * M + q];
                    io->mut_site[mo + k] = h_mu[3 * M + q];
                    io->mut_time[mo + k] = time_of(h_mu[4 * M + q]);
                }
                const int64_t go = io->mig_off[gi];
                for (int64_t k = 0; k < r5[4]; k++) {
                    const int64_t q = d.mig_off + k;
                    io->mig_node[go + k] = h_mg[q]; io->mig_old[go + k] = h_mg[G + q]; io->mig_new[go + k] = h_mg[2 * G + q];
                    io->mig_time[go + k] = time_of(h_mg[3 * G + q]);
                }
                bad[(size_t)j] = !ok;
            }
        }, std::max<int64_t>((N + M + G) / std::max<int64_t>(m, 1), 1) * 4);
        for (int64_t j = 0; j < m; j++)
            if (bad[(size_t)j]) return fail(e, VGX_ERR_ARG, me + "an event index outside the chain");
        io->ms[1] += since(t_host);
        io->passes += 1;
        i0 = i1;
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same key, merge rule, pre-pass, row rule and sampler on a chain given as arrays (no device, no
// engine).  The chain's trailing MULTITYPE events play the replicate's own steps: their rows may come in any order and
// granularity.  Everything before them plays the prefix.
extern "C" int vgx_test_tau_genealogy_walk(vgx_genealogy_io *io, int64_t sites, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    auto message = [](int64_t status, int64_t arg) {
        char buf[512];
        vgx_genealogy_message(status, arg, buf, 512);
        return std::string(buf);
    };
    const std::string me = "vgx_test_tau_genealogy_walk: ";
    if (!io || !io->infectious || !io->tree || !io->tree_pop || !io->times) return fail_(me + "null argument");
    if (io->sCounter < 2) return fail_(message(VGX_GW_FEW_SAMPLES, 0));
    const int64_t n = io->ev_ptr, P = io->popNum, H = io->hapNum, PH = P * H, sC = io->sCounter;
    if (n < 0 || n >= ((int64_t)1 << 30) || 2 * sC > ((int64_t)1 << 31) || sites < 0) return fail_(me + "chain too long");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail_(me + "null event column");
    if (io->mev_rows > 0 && (!io->mev_num || !io->mev_types || !io->mev_haplotypes || !io->mev_populations || !io->mev_newHaplotypes || !io->mev_newPopulations))
        return fail_(me + "null multievent column");
    HostChain hc;
    const std::string why = host_chain(io, sites, me, message, hc);
    if (!why.empty()) return fail_(why);
    const int64_t nodes = 2 * sC - 1, tsize = hc.tsize, arena_cap = hc.arena_cap;
    std::vector<int64_t> key((size_t)tsize, -1), cnt((size_t)tsize);
    std::unique_ptr<int32_t[]> base(new int32_t[(size_t)tsize]), len(new int32_t[(size_t)tsize]), lcap(new int32_t[(size_t)tsize]);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(arena_cap, 1)), fresh((size_t)nodes);
    std::vector<int32_t> tree((size_t)nodes), tree_pop((size_t)nodes), node_ev((size_t)nodes);
    const int64_t mut_cap = std::max<int64_t>(io->mut_cap, 0), mig_cap = std::max<int64_t>(io->mig_cap, 0);
    std::vector<int32_t> mu((size_t)mut_cap * 5 + 1), mg((size_t)mig_cap * 4 + 1);
    VgxGwRep w;
    w.n_ev = n; w.sCounter = sC; w.H = H; w.tsize = tsize;
    w.key = key.data(); w.cnt = cnt.data(); w.base = base.get(); w.len = len.get(); w.lcap = lcap.get();
    w.arena = arena.data(); w.arena_cap = arena_cap;
    w.tree = tree.data(); w.tree_pop = tree_pop.data(); w.node_ev = node_ev.data();
    w.mut_cap = mut_cap;
    w.mut_node = mu.data(); w.mut_AS = w.mut_node + mut_cap; w.mut_DS = w.mut_AS + mut_cap; w.mut_site = w.mut_DS + mut_cap;
    w.mut_ev = w.mut_site + mut_cap;
    w.mig_cap = mig_cap;
    w.mig_node = mg.data(); w.mig_old = w.mig_node + mig_cap; w.mig_new = w.mig_old + mig_cap; w.mig_ev = w.mig_new + mig_cap;
    const VgxGtChain c = hc.chain(n);
    VgxGwResult res{};
    res.status = vgx_gt_prepass(w, c);
    if (res.status != VGX_GW_OK) return fail_(message(res.status, res.arg));
    for (int64_t s = 0; s < tsize; s++)
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) cnt[(size_t)s] = io->infectious[key[(size_t)s]];
    VgxGtGen gen{{io->rng_state[0], io->rng_state[1], io->rng_state[2], io->rng_state[3]}, io->rng_has_uint32 != 0, (uint32_t)io->rng_uinteger};
    vgx_gt_walk(w, c, fresh.data(), gen, res);
    for (int64_t s = 0; s < tsize; s++)   // walked back in place, as the host pass does
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) io->infectious[key[(size_t)s]] = cnt[(size_t)s];
    if (res.status != VGX_GW_OK) return fail_(message(res.status, res.arg));
    auto time_of = [&](int32_t e) { return hc.time_of(e); };
    for (int64_t i = 0; i < nodes; i++) {
        io->tree[i] = tree[(size_t)i]; io->tree_pop[i] = tree_pop[(size_t)i]; io->times[i] = time_of(node_ev[(size_t)i]);
    }
    io->mut_n = res.mut_n;
    for (int64_t k = 0; k < res.mut_n; k++) {
        io->mut_node[k] = w.mut_node[k]; io->mut_AS[k] = w.mut_AS[k]; io->mut_DS[k] = w.mut_DS[k]; io->mut_site[k] = w.mut_site[k];
        io->mut_time[k] = time_of(w.mut_ev[k]);
    }
    io->mig_n = res.mig_n;
    for (int64_t k = 0; k < res.mig_n; k++) {
        io->mig_node[k] = w.mig_node[k]; io->mig_old[k] = w.mig_old[k]; io->mig_new[k] = w.mig_new[k];
        io->mig_time[k] = time_of(w.mig_ev[k]);
    }
    io->nodes_used = res.nodes_used;
    io->rng_state[0] = gen.g.sh; io->rng_state[1] = gen.g.sl; io->rng_state[2] = gen.g.ih; io->rng_state[3] = gen.g.il;
    io->rng_has_uint32 = gen.has32 ? 1 : 0;
    io->rng_uinteger = gen.spare;
    return VGX_OK;
}

extern "C" int vgx_test_hypergeometric(int on_device, int64_t good, int64_t bad, int64_t sample, int64_t n, uint64_t state[6], int64_t *out) {
    if (!state || !out || n < 0 || good < 0 || bad < 0 || sample < 0 || good > INT64_MAX - bad || sample > good + bad) return VGX_ERR_ARG;
    if (!on_device) {
        VgxGtGen gen{{state[0], state[1], state[2], state[3]}, state[4] != 0, (uint32_t)state[5]};
        for (int64_t i = 0; i < n; i++) out[i] = vgx_gt_hypergeometric(gen, good, bad, sample);
        state[0] = gen.g.sh; state[1] = gen.g.sl; state[2] = gen.g.ih; state[3] = gen.g.il; state[4] = gen.has32 ? 1 : 0; state[5] = gen.spare;
        return VGX_OK;
    }
    char *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)(n + 6) * 8) != hipSuccess) return VGX_ERR_HIP;
    uint64_t *d_state = (uint64_t *)d;
    int64_t *d_out = (int64_t *)(d + 48);
    hipError_t e1 = hipMemcpy(d_state, state, 48, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(vgxtg_hyper_kernel, dim3(1), dim3(64), 0, 0, good, bad, sample, n, d_state, d_out);
    hipError_t e2 = hipGetLastError(), e3 = hipDeviceSynchronize();
    hipError_t e4 = hipMemcpy(state, d_state, 48, hipMemcpyDeviceToHost);
    hipError_t e5 = n ? hipMemcpy(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost) : hipSuccess;
    (void)hipFree(d);
    return (e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess && e4 == hipSuccess && e5 == hipSuccess) ? VGX_OK : VGX_ERR_HIP;
}
