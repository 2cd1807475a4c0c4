// vgx_mutation_spectrum.hip — the spectrum kernel of vgx_get_mutation_spectrum and vgx_get_tau_mutation_spectrum: the mutation records
// of every tree the walk left on the device reduced where they lie to the row of vgx_mutation_spectrum.h (log2-binned clade sizes,
// substitution counts, three sums per site, four scalars); the host side of the tau call and the device test hook.  DESIGN.md §31.
//
// One wavefront per tree, four trees per workgroup of 256 threads, two phases in one kernel.
//   1. Clade sweep: the 64-lane rounds of vgx_tree_shapes.hip carrying n alone.  Per node kids, got, n and the finished clade as
//      int32 in the pass's global workspace (16 bytes per node); the kernel initialises them.  A first parallel pass checks every
//      parent (i < tree[i] < N: nothing below indexes outside the tree) and counts the children.  The sweep takes 64 consecutive
//      nodes per round in ascending id: a lane is ready when got[i] == kids[i], ready lanes store clade[i] (a plain store) and push
//      n and got into the parent with two atomics, and the round repeats under a ballot until its 64 lanes are done.  Every iteration
//      finishes at least the lowest unfinished lane, so a round takes at most 64 iterations and the loop is bounded by that: a round
//      that does not finish gives status 13, never a hang.
//   2. Binning: the wavefront strides over its own M records, 64 per step: four coalesced 4-byte loads, the comparisons with N, S
//      and 0 .. 3 BEFORE the gather clade[mut_node], bin = 31 - clz(c), LDS atomics into this wavefront's private cells (S * 32
//      spectrum and S * 16 substitution counts of 32 bits: M < 2^30; S * 3 sums of 64 bits).  The static allocation is for S = 15:
//      15 * (48 * 4 + 3 * 8) = 3240 bytes per wavefront, 12960 per workgroup.  max_clade, fixed and the lowest bad record index
//      stay in registers and are reduced by butterfly.  The wavefront then writes every cell of its row once with plain vector stores,
//      zeros included: the host initialises nothing.
//
// Memory order inside the wavefront: as vgx_tree_shapes.hip.  The pushes are relaxed atomics, performed at the L2; VGXM_SYNC waits
// for every vector-memory operation of the wavefront before the next iteration issues, and kids, got, n and (in phase 2) clade are
// read back with agent-scope atomic loads that go to the L2 and not to the vector L1, which may hold the line from before.  No
// other wavefront touches a tree's workspace or this wavefront's LDS cells, so no workgroup barrier is needed (and none could be
// used: wavefronts past the last tree leave at once).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_tau_lineages.h"     // vgxi_tg_canon, vgxi_tg_count, vgxi_tg_walk
#include "vgx_tau_chain.h"
#include "vgx_mutation_spectrum.h"

namespace {

#define VGXM_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   \
        __builtin_amdgcn_wave_barrier();                         \
    } while (0)

#define VGXM_CNT (VGX_MSP_SITES_MAX * (VGX_MSP_BINS + 16))   // 32-bit cells of one wavefront: spectrum, then substitutions
#define VGXM_SUM (VGX_MSP_SITES_MAX * VGX_MSP_SUMS)          // 64-bit cells of one wavefront

__device__ __forceinline__ int32_t ld32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t wave_min(int32_t v) {
    for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_min(int64_t v) {
    for (int d = 32; d > 0; d >>= 1) { const int64_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The 64-lane rounds over one tree (all 64 lanes, wave-uniform control flow).  Returns -1 with clade[N] complete (wave-uniform), or the
// first node that breaks the precondition.
__device__ int64_t clade_rounds(const int32_t *tree, const int32_t N, const VgxMspWork &w, const int lane) {
    int32_t bad = INT32_MAX;
    for (int32_t i = lane; i < N; i += 64) {
        const int32_t p = tree[i];
        if (i == N - 1 ? p != -1 : (p <= i || p >= N)) bad = i < bad ? i : bad;
        w.kids[i] = 0; w.got[i] = 0; w.n[i] = 0;
    }
    bad = wave_min(bad);
    if (bad != INT32_MAX) return bad;
    VGXM_SYNC();
    for (int32_t i = lane; i < N - 1; i += 64) atomicAdd(&w.kids[tree[i]], 1);
    VGXM_SYNC();
    for (int32_t base = 0; base < N; base += 64) {
        const int32_t i = base + lane;
        const bool in = i < N;
        const int32_t kids = in ? ld32(&w.kids[i]) : 0;
        const bool wrong = in && kids != 0 && kids != 2;
        if (__ballot(wrong)) return wave_min(wrong ? i : INT32_MAX);
        const bool tip = kids == 0;
        bool todo = in;
        for (int it = 0; it < 64; it++) {
            if (todo && (tip || ld32(&w.got[i]) == kids)) {
                const int32_t c = tip ? 1 : ld32(&w.n[i]);
                w.clade[i] = c;
                if (i != N - 1) {
                    const int32_t p = tree[i];
                    atomicAdd(&w.n[p], c);
                    atomicAdd(&w.got[p], 1);
                }
                todo = false;
            }
            VGXM_SYNC();
            if (!__ballot(todo)) break;
        }
        if (__ballot(todo)) return wave_min(todo ? i : INT32_MAX);   // (not with the child counts checked above: the loop's bound)
    }
    return -1;
}

__global__ void __launch_bounds__(256) vgxm_spectrum_kernel(VgxMspLaunch a) {
    __shared__ uint32_t s_cnt[4][VGXM_CNT];
    __shared__ unsigned long long s_sum[4][VGXM_SUM];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= a.n) return;   // (the whole wavefront)
    const VgxMspDesc d = a.desc[row];
    const int S = (int)a.S;
    int64_t status = a.res ? a.res[row * 5] : 0, arg = a.res ? a.res[row * 5 + 1] : 0;
    uint32_t *cnt = s_cnt[wave];
    unsigned long long *sum = s_sum[wave];
    for (int k = lane; k < S * (VGX_MSP_BINS + 16); k += 64) cnt[k] = 0;
    for (int k = lane; k < S * VGX_MSP_SUMS; k += 64) sum[k] = 0;
    int64_t st[VGX_MSP_STATS] = {0, 0, 0, 0};
    if (status == 0) {
        const int64_t o = d.node_off;
        const VgxMspWork w{a.w.kids + o, a.w.got + o, a.w.n + o, a.w.clade + o};
        int64_t bad = d.nodes;   // a node count that is even or below 3
        if (d.nodes >= 3 && (d.nodes & 1) && d.nodes <= INT32_MAX) bad = clade_rounds(a.tree + o, (int32_t)d.nodes, w, lane);
        if (bad >= 0) { status = VGX_GW_BAD_TREE; arg = bad; }
        else {
            VGXM_SYNC();   // clade[] and the zeroed LDS cells before the records
            const int32_t N = (int32_t)d.nodes;
            int64_t M = a.res ? a.res[row * 5 + 3] : d.muts;   // (the walk's mut_n, inside the capacity it was given)
            M = M < 0 ? 0 : (M > d.muts ? d.muts : M);
            const int32_t *mn = a.mut_node + d.mut_off, *mA = a.mut_AS + d.mut_off, *mD = a.mut_DS + d.mut_off, *ms = a.mut_site + d.mut_off;
            const int32_t tips = ld32(&w.clade[N - 1]);
            int64_t badk = INT64_MAX, fixed = 0;
            int32_t maxc = 0;
            for (int64_t k0 = 0; k0 < M; k0 += 64) {
                const int64_t k = k0 + lane;
                if (k < M) {
                    const int32_t node = mn[k], AS = mA[k], DS = mD[k], site = ms[k];
                    if (!vgx_msp_record_ok(node, AS, DS, site, N, S)) badk = k < badk ? k : badk;   // (ascending k: the lane's first)
                    else {
                        const int32_t c = ld32(&w.clade[node]);
                        const int b = c > 0 ? 31 - __clz(c) : 0;   // (c >= 1 after a sweep that finished: the index stays in the cells regardless)
                        atomicAdd(&cnt[site * VGX_MSP_BINS + b], 1u);
                        atomicAdd(&cnt[S * VGX_MSP_BINS + site * 16 + AS * 4 + DS], 1u);
                        const unsigned long long c64 = (unsigned long long)c;
                        atomicAdd(&sum[site * VGX_MSP_SUMS + VGX_MSP_CLADE_SUM], c64);
                        atomicAdd(&sum[site * VGX_MSP_SUMS + VGX_MSP_CLADE_SUMSQ], c64 * c64);
                        atomicAdd(&sum[site * VGX_MSP_SUMS + VGX_MSP_PAIR_SUM], c64 * (unsigned long long)(tips - c));
                        fixed += c == tips;
                        maxc = c > maxc ? c : maxc;
                    }
                }
            }
            badk = wave_min(badk);
            if (badk != INT64_MAX) { status = VGX_GW_BAD_RECORD; arg = badk; }
            else { st[VGX_MSP_TIPS] = tips; st[VGX_MSP_MUTATIONS] = M; st[VGX_MSP_FIXED] = wave_sum(fixed); st[VGX_MSP_MAX_CLADE] = wave_max(maxc); }
        }
    }
    VGXM_SYNC();   // this wavefront's LDS atomics before it reads the cells
    const bool ok = status == 0;
    int64_t *o_sp = a.spectrum + row * S * VGX_MSP_BINS, *o_sub = a.substitutions + row * S * 16, *o_sum = a.sums + row * S * VGX_MSP_SUMS;
    for (int k = lane; k < S * VGX_MSP_BINS; k += 64) o_sp[k] = ok ? (int64_t)cnt[k] : 0;
    for (int k = lane; k < S * 16; k += 64) o_sub[k] = ok ? (int64_t)cnt[S * VGX_MSP_BINS + k] : 0;
    for (int k = lane; k < S * VGX_MSP_SUMS; k += 64) o_sum[k] = ok ? (int64_t)sum[k] : 0;
    if (lane < VGX_MSP_STATS) {
        int64_t v = st[0];
#pragma unroll
        for (int k = 1; k < VGX_MSP_STATS; k++) v = lane == k ? st[k] : v;
        a.stats[row * VGX_MSP_STATS + lane] = ok ? v : 0;
    }
    if (lane < 2) a.status[row * 2 + lane] = lane == 0 ? status : arg;
}

using namespace vgxtc;

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ms_spectrum(const VgxMspLaunch *a, hipStream_t s) {
    if (a->S < 0 || a->S > VGX_MSP_SITES_MAX) return hipErrorInvalidValue;   // (the LDS cells are sized for 15 sites)
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxm_spectrum_kernel, dim3((unsigned)((a->n + 3) / 4)), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// ---- the tau call: the frame of vgx_get_tau_tree_shapes without node times ----------------------------------------------------------
// Per pass, on one stream: the canonicalise kernel of vgx_tau_genealogies.hip, its report (the one host step inside a pass: it sizes
// the walk's table and arena), the walk kernel as it is, the spectrum kernel.  Nothing of a tree or a record comes to the host.
extern "C" int vgx_get_tau_mutation_spectrum(vgx_engine *e, vgx_tau_mutation_spectrum_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->spectrum || !io->substitutions || !io->sums || !io->stats || !io->status ||
                       !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_mutation_spectrum: ";
    io->passes = 0;
    io->sites = e->d.sites;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    io->kernel_ms[0] = io->kernel_ms[1] = io->kernel_ms[2] = 0.0;
    // preconditions and refusals: those of vgx_get_tau_genealogies
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (walks tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, PH = P * H, mev_cap = e->tau_mev_cap, S = e->d.sites;
    if (S < 0 || S > VGX_MSP_SITES_MAX) return fail(e, VGX_ERR_ARG, me + "the model has " + std::to_string(S) + " sites (0 .. 15)");
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
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    typedef std::unique_ptr<char, void (*)(char *)> Hold;
    hipError_t er;

    // what stays for the whole call: [rep | raw rows | sCounter | row sums | prefix rows | prefix offsets]
    const int64_t o_rep = 0, o_raw = o_rep + up8(n * 8), o_sc = o_raw + up8(n * 8), o_cnt = o_sc + up8(n * 8), o_prow = o_cnt + up8(n * 24),
                  o_poff = o_prow + up8(pre_rows * 32 + 32), keep_total = o_poff + up8((int64_t)pre.off.size() * 4);
    char *kws = nullptr;
    if ((er = hipMalloc((void **)&kws, (size_t)keep_total)) != hipSuccess)
        return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    Hold khold(kws, dev_free);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_raw, raw.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_sc, sC.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    if (pre_rows) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 32, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_poff, pre.off.data(), pre.off.size() * 4, hipMemcpyHostToDevice, e->stream));
    // raw sums of min(num, sCounter): MUTATION rows, MIGRATION rows, rows that can push a lineage: the record capacities of the
    // sizing branch of vgx_get_tau_genealogies and the bound of a pass's workspace
    std::vector<int64_t> cnt((size_t)n * 3);
    HIPCHECK(e, vgxi_tg_count((const int64_t *)e->t_mev.p, mev_cap, (const int64_t *)(kws + o_rep), (const int64_t *)(kws + o_raw),
                              (const int64_t *)(kws + o_sc), n, (int64_t *)(kws + o_cnt), e->stream));
    HIPCHECK(e, hipMemcpyAsync(cnt.data(), kws + o_cnt, (size_t)n * 24, hipMemcpyDeviceToHost, e->stream));
    if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));
    auto nodes_of = [&](int64_t i) { return sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0; };
    auto mut_need = [&](int64_t i) {
        if (sC[(size_t)i] < 2) return (int64_t)0;
        return cnt[(size_t)(3 * i)] + (with_prefix[(size_t)i] ? pre_caps.direct_mut + pre_caps.mut(sC[(size_t)i]) : 0);
    };
    auto mig_need = [&](int64_t i) {
        if (sC[(size_t)i] < 2) return (int64_t)0;
        return cnt[(size_t)(3 * i + 1)] + (with_prefix[(size_t)i] ? pre_caps.direct_mig + pre_caps.mig(sC[(size_t)i]) : 0) + nodes_of(i);
    };

    // passes: what a replicate can need at most, from its raw rows (vgx_get_tau_genealogies' sum, the 16 bytes of workspace per node
    // and the rows added)
    const int64_t row_bytes = 8 * (S * (VGX_MSP_BINS + 16 + VGX_MSP_SUMS) + VGX_MSP_STATS + 2);
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
                           nodes * (16 + VGX_MSP_NODE_BYTES) + mut_need(i) * 20 + mig_need(i) * 16 +
                           (int64_t)(sizeof(VgxGtDesc) + sizeof(VgxGtCanonDesc) + sizeof(VgxGtCanonStat) + sizeof(VgxMspDesc)) + row_bytes + 2048;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // the two kernels behind the canonicalise kernel, timed apart
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        // ---- canonicalise: [desc | stat | step ranges | canonical row ranges | canonical rows]
        auto t_host = std::chrono::steady_clock::now();
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
        io->ms[1] += since(t_host);
        const int64_t c_desc = 0, c_stat = c_desc + up8(m * (int64_t)sizeof(VgxGtCanonDesc)), c_mr = c_stat + up8(m * (int64_t)sizeof(VgxGtCanonStat)),
                      c_off = c_mr + up8((int64_t)mrange.size() * 4), c_rows = c_off + up8(OO * 4), c_total = c_rows + up8(RO * 32 + 32);
        char *cws = nullptr;
        if ((er = hipMalloc((void **)&cws, (size_t)c_total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(c_total) + " bytes: " + hipGetErrorString(er));
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
        HIPCHECK(e, vgxi_tg_canon(&ca, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // the sizes of the walk's workspace come from its report
            return fail(e, VGX_ERR_HIP, me + "canonicalise kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->kernel_ms[0] += kms;
        io->ms[0] += kms;
        std::vector<VgxGtCanonStat> stat((size_t)m);
        HIPCHECK(e, hipMemcpy(stat.data(), ca.stat, (size_t)m * sizeof(VgxGtCanonStat), hipMemcpyDeviceToHost));

        // ---- walk, spectrum: the walk's [desc | res | rng | key | cnt | base | len | lcap | arena | fresh | node x3 | mut x5 | mig x4],
        // then [tree descs | kids, got, n, clade | spectrum | substitutions | sums | stats | status]
        t_host = std::chrono::steady_clock::now();
        std::vector<VgxGtDesc> dp((size_t)m);
        std::vector<VgxMspDesc> md((size_t)m);
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
            d.mut_cap = mut_need(gi);
            d.mig_cap = mig_need(gi);
            d.row_off = cd[(size_t)j].row_off; d.off_off = cd[(size_t)j].off_off;
            for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[gi * 6 + k];
            d.has32 = io->rng_state[gi * 6 + 4] != 0; d.spare = (int64_t)(uint32_t)io->rng_state[gi * 6 + 5];
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            md[(size_t)j] = VgxMspDesc{N, nodes_of(gi), M, d.mut_cap};
            T += d.tsize; A += d.arena_cap; N += nodes_of(gi); M += d.mut_cap; G += d.mig_cap;
        }
        io->ms[1] += since(t_host);
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGtDesc)), o_rng = o_res + up8(m * 40), o_key = o_rng + up8(m * 48),
                      o_cnt2 = o_key + up8(T * 8), o_base = o_cnt2 + up8(T * 8), o_len = o_base + up8(T * 4), o_lcap = o_len + up8(T * 4),
                      o_arena = o_lcap + up8(T * 4), o_fresh = o_arena + up8(A * 4), o_out = o_fresh + up8(N * 4),
                      o_md = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_w32 = o_md + up8(m * (int64_t)sizeof(VgxMspDesc)),
                      o_sp = o_w32 + up8(4 * N * 4), o_sub = o_sp + up8(m * S * VGX_MSP_BINS * 8), o_sums = o_sub + up8(m * S * 16 * 8),
                      o_stats = o_sums + up8(m * S * VGX_MSP_SUMS * 8), o_status = o_stats + up8(m * VGX_MSP_STATS * 8), total = o_status + up8(m * 16);
        char *ws = nullptr;
        if ((er = hipMalloc((void **)&ws, (size_t)total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        Hold hold(ws, dev_free);
        VgxGtLaunch a{};
        a.n = m;
        a.desc = (const VgxGtDesc *)(ws + o_desc);
        a.pre = (const VgxGtRow *)(kws + o_prow); a.pre_off = (const int32_t *)(kws + o_poff);
        a.can = ca.can; a.can_off = ca.can_off;
        a.I = (const int32_t *)e->t_I.p;
        a.P = P; a.H = H;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt2);
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
        VgxMspLaunch b{};
        b.n = m;
        b.desc = (const VgxMspDesc *)(ws + o_md);
        b.res = a.res;
        b.tree = a.tree;
        b.mut_node = a.mut_node; b.mut_AS = a.mut_AS; b.mut_DS = a.mut_DS; b.mut_site = a.mut_site;
        b.S = S;
        int32_t *w32 = (int32_t *)(ws + o_w32);
        b.w = VgxMspWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N};
        b.spectrum = (int64_t *)(ws + o_sp); b.substitutions = (int64_t *)(ws + o_sub); b.sums = (int64_t *)(ws + o_sums);
        b.stats = (int64_t *)(ws + o_stats); b.status = (int64_t *)(ws + o_status);
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGtDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_md, md.data(), (size_t)m * sizeof(VgxMspDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        // walk and spectrum with no host step between them
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_tg_walk(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        HIPCHECK(e, vgxi_ms_spectrum(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        std::vector<int64_t> st2((size_t)m * 2);
        HIPCHECK(e, hipMemcpyAsync(io->spectrum + i0 * S * VGX_MSP_BINS, b.spectrum, (size_t)(m * S * VGX_MSP_BINS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->substitutions + i0 * S * 16, b.substitutions, (size_t)(m * S * 16) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->sums + i0 * S * VGX_MSP_SUMS, b.sums, (size_t)(m * S * VGX_MSP_SUMS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->stats + i0 * VGX_MSP_STATS, b.stats, (size_t)m * VGX_MSP_STATS * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(st2.data(), b.status, (size_t)m * 16, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 6, a.rng_out, (size_t)m * 48, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // before anything reads the rows
            return fail(e, VGX_ERR_HIP, me + "walk or spectrum kernel failed: " + hipGetErrorString(er));
        for (int k = 0; k < 2; k++) {
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->kernel_ms[k + 1] += kms;
            io->ms[0] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            io->status[i0 + j] = st2[(size_t)(2 * j)];
            io->status_arg[i0 + j] = st2[(size_t)(2 * j + 1)];
        }
        io->passes += 1;
        i0 = i1;
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- test hook: given trees and records through the kernel (no engine) ----------------------------------------------------------------
extern "C" int vgx_test_mutation_spectrum_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int64_t *mut_off, const int32_t *mut_node,
                                                 const int32_t *mut_AS, const int32_t *mut_DS, const int32_t *mut_site, int64_t sites,
                                                 const int64_t *walk_status, int64_t *spectrum, int64_t *substitutions, int64_t *sums, int64_t *stats,
                                                 int64_t *status, int32_t *clade, char *errbuf, int64_t errcap) {
    auto fail_ = [&](int code, const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return code;
    };
    const std::string me = "vgx_test_mutation_spectrum_device: ";
    if (n < 0 || (n > 0 && (!node_off || !tree || !mut_off || !spectrum || !substitutions || !sums || !stats || !status))) return fail_(VGX_ERR_ARG, me + "null argument");
    if (sites < 0 || sites > VGX_MSP_SITES_MAX) return fail_(VGX_ERR_ARG, me + "sites = " + std::to_string(sites) + " (0 .. 15)");
    if (n == 0) return VGX_OK;
    if (node_off[0] != 0 || mut_off[0] != 0) return fail_(VGX_ERR_ARG, me + "node_off[0] and mut_off[0] must be 0");
    // every array the kernel indexes is bounded here: the tree by its parents, the records by mut_off; what a record holds is
    // compared on the device before it is used
    std::vector<VgxMspDesc> dp((size_t)n);
    std::vector<int64_t> res;
    if (walk_status) res.assign((size_t)n * 5, 0);
    for (int64_t t = 0; t < n; t++) {
        const int64_t N = node_off[t + 1] - node_off[t], M = mut_off[t + 1] - mut_off[t];
        if (N < 0) return fail_(VGX_ERR_ARG, me + "node_off must not decrease");
        if (M < 0 || M >= ((int64_t)1 << 30)) return fail_(VGX_ERR_ARG, me + "mut_off must not decrease (a tree holds fewer than 2^30 records)");
        const int64_t bad = vgx_ts_check_parents(tree + node_off[t], N);
        if (bad == N) return fail_(VGX_ERR_ARG, me + "tree " + std::to_string(t) + " has " + std::to_string(N) + " nodes: an odd number, at least 3");
        if (bad >= 0)
            return fail_(VGX_ERR_ARG, me + "tree " + std::to_string(t) + ": the parent of node " + std::to_string(bad) + " is " +
                                          std::to_string(tree[node_off[t] + bad]) + " (a higher id inside the tree, -1 at the last node)");
        dp[(size_t)t] = VgxMspDesc{node_off[t], N, mut_off[t], M};
        if (walk_status) {
            res[(size_t)(t * 5)] = walk_status[2 * t]; res[(size_t)(t * 5 + 1)] = walk_status[2 * t + 1];
            res[(size_t)(t * 5 + 2)] = N; res[(size_t)(t * 5 + 3)] = M;
        }
    }
    const int64_t T = node_off[n], M = mut_off[n], S = sites;
    if (M > 0 && (!mut_node || !mut_AS || !mut_DS || !mut_site)) return fail_(VGX_ERR_ARG, me + "null argument");
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t o_desc = 0, o_res = o_desc + up(n * (int64_t)sizeof(VgxMspDesc)), o_tree = o_res + up(n * 40), o_mut = o_tree + up(T * 4),
                  o_w32 = o_mut + up(4 * M * 4 + 4), o_sp = o_w32 + up(4 * T * 4), o_sub = o_sp + up(n * S * VGX_MSP_BINS * 8),
                  o_sums = o_sub + up(n * S * 16 * 8), o_stats = o_sums + up(n * S * VGX_MSP_SUMS * 8), o_status = o_stats + up(n * VGX_MSP_STATS * 8),
                  total = o_status + up(n * 16);
    char *ws = nullptr;
    hipError_t er = hipMalloc((void **)&ws, (size_t)total);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
    VgxMspLaunch a{};
    a.n = n;
    a.desc = (const VgxMspDesc *)(ws + o_desc);
    a.res = walk_status ? (const int64_t *)(ws + o_res) : nullptr;
    a.tree = (const int32_t *)(ws + o_tree);
    int32_t *mu = (int32_t *)(ws + o_mut);
    a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M;
    a.S = S;
    int32_t *w32 = (int32_t *)(ws + o_w32);
    a.w = VgxMspWork{w32, w32 + T, w32 + 2 * T, w32 + 3 * T};
    a.spectrum = (int64_t *)(ws + o_sp); a.substitutions = (int64_t *)(ws + o_sub); a.sums = (int64_t *)(ws + o_sums);
    a.stats = (int64_t *)(ws + o_stats); a.status = (int64_t *)(ws + o_status);
    er = hipMemcpy(ws + o_desc, dp.data(), (size_t)n * sizeof(VgxMspDesc), hipMemcpyHostToDevice);
    if (er == hipSuccess && walk_status) er = hipMemcpy(ws + o_res, res.data(), (size_t)n * 40, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_tree, tree, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && M) er = hipMemcpy(mu, mut_node, (size_t)M * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && M) er = hipMemcpy(mu + M, mut_AS, (size_t)M * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && M) er = hipMemcpy(mu + 2 * M, mut_DS, (size_t)M * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && M) er = hipMemcpy(mu + 3 * M, mut_site, (size_t)M * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess && clade) er = hipMemset(a.w.clade, 0, (size_t)T * 4);   // (a rejected or skipped tree's clade reads 0 in the hook)
    if (er == hipSuccess) er = vgxi_ms_spectrum(&a, nullptr);
    if (er == hipSuccess) er = hipStreamSynchronize(nullptr);
    if (er == hipSuccess) er = hipMemcpy(spectrum, a.spectrum, (size_t)(n * S * VGX_MSP_BINS) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(substitutions, a.substitutions, (size_t)(n * S * 16) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(sums, a.sums, (size_t)(n * S * VGX_MSP_SUMS) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(stats, a.stats, (size_t)n * VGX_MSP_STATS * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(status, a.status, (size_t)n * 16, hipMemcpyDeviceToHost);
    if (er == hipSuccess && clade) er = hipMemcpy(clade, a.w.clade, (size_t)T * 4, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + hipGetErrorString(er));
    return VGX_OK;
}
