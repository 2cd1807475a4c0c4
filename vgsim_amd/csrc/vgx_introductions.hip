// vgx_introductions.hip — the lineage kernel of vgx_get_introductions and vgx_get_tau_introductions: the population labels of every
// tree the walk left on the device reduced where they lie to the row of vgx_introductions.h (tips per population, introductions by
// source and destination, six figures and a log2 size spectrum per destination, eight scalars); the host side of the tau call and
// the device test hook.  DESIGN.md §32.
//
// One wavefront per tree, four trees per workgroup of 256 threads, two phases in one kernel.
//   1. Sweep: the 64-lane rounds of vgx_mutation_spectrum.hip carrying two sums, n (tips below) and ln (tips below reached without a
//      crossing branch).  Per node kids, got, n and ln as int32 in the pass's global workspace (16 bytes per node); the kernel
//      initialises them.  A first parallel pass checks every parent (i < tree[i] < N: nothing below indexes outside the tree),
//      compares every label with P (the lowest node outside [0, P) is kept; nothing indexes by a label before phase 2) and, after
//      it, counts the children.  A round takes 64 consecutive nodes in ascending id; the crossing flag of a lane's node is one
//      gather pop[tree[i]] compared with pop[i], taken before the round's iterations.  A lane is ready when got[i] == kids[i];
//      ready lanes push n into the parent, ln too unless the branch crosses, then got: three atomics at the most.  The round
//      repeats under a ballot until its 64 lanes are done; every iteration finishes at least the lowest unfinished lane, so the
//      loop is bounded by 64: a round that does not finish gives status 13, never a hang.
//   2. Binning, a second strided pass over the nodes, entered only by a tree whose structure and labels are good: 64 nodes per
//      step, coalesced loads of tree, pop, kids, n and ln, the gather pop[tree[i]], and for a tip one add to its population's
//      cell, for a crossing branch the adds of one introduction.  Binning where a lane finishes a head node (inside the rounds)
//      would save the pass, but a structure fault can show as late as the last round, after cells were already written: the row
//      of a rejected tree has to stay all zeros and imports is counted in place in global memory.  The pass reads 20 bytes per
//      node in full lines; the rounds dominate.
//   Cells.  Up to VGX_IN_LDS_POPS = 32 populations (the kernel with LDS = true) the per-destination cells are private to the
//   wavefront in LDS: per population 36 cells of 32 bits (tips, count, empty, max local, 32 bins: a tree has fewer than 2^31
//   nodes) and 3 of 64 bits (the sums): 168 bytes, 5376 per wavefront, 21504 per workgroup, static (seven workgroups
//   on a CU; at 64 populations it would be three).  The wavefront then writes
//   those blocks of its row once with plain vector stores.  Past 32 populations (LDS = false, no LDS at all) the same adds are
//   64-bit atomics on the tree's own row, which the caller zeroed.  imports[P][P] is counted in the row by global atomics in
//   both forms: introductions are few next to nodes.
//
// Memory order inside the wavefront: as vgx_mutation_spectrum.hip.  The pushes are relaxed atomics, performed at the L2; VGXI_SYNC
// waits for every vector-memory operation of the wavefront before the next iteration issues, and kids, got, n, ln (and the row's
// tips cells in the global form) are read back with agent-scope atomic loads that go to the L2 and not to the vector L1, which may
// hold the line from before.  No other wavefront touches a tree's workspace, its row or this wavefront's LDS cells, so no workgroup
// barrier is needed (and none could be used: wavefronts past the last tree leave at once).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_tau_lineages.h"     // vgxi_tg_canon, vgxi_tg_count, vgxi_tg_walk
#include "vgx_tau_chain.h"
#include "vgx_introductions.h"

namespace {

#define VGXI_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   \
        __builtin_amdgcn_wave_barrier();                         \
    } while (0)

#define VGXI_PER32 (4 + VGX_IN_BINS)                 // 32-bit cells of one population: tips, count, empty, max local, the bins
#define VGXI_C32 (VGX_IN_LDS_POPS * VGXI_PER32)      // 32-bit cells of one wavefront
#define VGXI_C64 (VGX_IN_LDS_POPS * 3)               // 64-bit cells of one wavefront: sum clade, sum local, sum local^2

__device__ __forceinline__ int32_t ld32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int64_t ld64(const int64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t wave_min(int32_t v) {
    for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The 64-lane rounds over one tree (all 64 lanes, wave-uniform control flow).  Returns -1 with n[N] and ln[N] complete
// (wave-uniform), or the first node that breaks the precondition.  *bad_label: the lowest node whose label lies outside [0, P),
// INT32_MAX without one (wave-uniform; meaningful after a return of -1).
__device__ int64_t lineage_rounds(const int32_t *tree, const int32_t *pop, const int32_t N, const int32_t P, const VgxInWork &w, const int lane,
                                  int32_t *bad_label) {
    int32_t bad = INT32_MAX, badl = INT32_MAX;
    for (int32_t i = lane; i < N; i += 64) {
        const int32_t p = tree[i], q = pop[i];
        if (i == N - 1 ? p != -1 : (p <= i || p >= N)) bad = i < bad ? i : bad;
        if (q < 0 || q >= P) badl = i < badl ? i : badl;
        w.kids[i] = 0; w.got[i] = 0; w.n[i] = 0; w.ln[i] = 0;
    }
    bad = wave_min(bad);
    *bad_label = wave_min(badl);
    if (bad != INT32_MAX) return bad;
    VGXI_SYNC();
    for (int32_t i = lane; i < N - 1; i += 64) atomicAdd(&w.kids[tree[i]], 1);
    VGXI_SYNC();
    for (int32_t base = 0; base < N; base += 64) {
        const int32_t i = base + lane;
        const bool in = i < N;
        const int32_t kids = in ? ld32(&w.kids[i]) : 0;
        const bool wrong = in && kids != 0 && kids != 2;
        if (__ballot(wrong)) return wave_min(wrong ? i : INT32_MAX);
        const bool tip = kids == 0, up = in && i != N - 1;
        const int32_t p = up ? tree[i] : 0;                      // (checked above: inside the tree)
        const bool crossing = up && pop[p] != pop[i];            // the one gather; labels are compared here, never used as an index
        bool todo = in;
        for (int it = 0; it < 64; it++) {
            if (todo && (tip || ld32(&w.got[i]) == kids)) {
                if (up) {
                    const int32_t c = tip ? 1 : ld32(&w.n[i]), l = tip ? 1 : ld32(&w.ln[i]);
                    atomicAdd(&w.n[p], c);
                    if (!crossing) atomicAdd(&w.ln[p], l);
                    atomicAdd(&w.got[p], 1);
                }
                todo = false;
            }
            VGXI_SYNC();
            if (!__ballot(todo)) break;
        }
        if (__ballot(todo)) return wave_min(todo ? i : INT32_MAX);   // (not with the child counts checked above: the loop's bound)
    }
    return -1;
}

// the adds of phase 2 in their two forms: LDS cells of the wavefront, or 64-bit cells of the tree's zeroed row
template <bool LDS>
struct Cells {
    uint32_t *c32;                 // LDS: [P][VGXI_PER32]
    unsigned long long *c64;       // LDS: [P][3]
    int64_t *tips, *into, *spec;   // global: the row's blocks
    __device__ __forceinline__ void tip(int32_t dst) const {
        if (LDS) atomicAdd(&c32[dst * VGXI_PER32], 1u);
        else atomicAdd((unsigned long long *)&tips[dst], 1ull);
    }
    __device__ __forceinline__ void introduction(int32_t dst, int32_t c, int32_t l) const {
        const unsigned long long c64v = (unsigned long long)c, l64 = (unsigned long long)l;
        const int b = l > 0 ? 31 - __clz(l) : 0;
        if (LDS) {
            uint32_t *q = c32 + dst * VGXI_PER32;
            atomicAdd(&q[1], 1u);
            if (l == 0) atomicAdd(&q[2], 1u);
            else { atomicMax(&q[3], (uint32_t)l); atomicAdd(&q[4 + b], 1u); }
            atomicAdd(&c64[dst * 3], c64v);
            atomicAdd(&c64[dst * 3 + 1], l64);
            atomicAdd(&c64[dst * 3 + 2], l64 * l64);
        } else {
            int64_t *q = into + (int64_t)dst * VGX_IN_INTO;
            atomicAdd((unsigned long long *)&q[VGX_IN_COUNT], 1ull);
            atomicAdd((unsigned long long *)&q[VGX_IN_CLADE_SUM], c64v);
            if (l == 0) atomicAdd((unsigned long long *)&q[VGX_IN_EMPTY], 1ull);
            else {
                atomicAdd((unsigned long long *)&q[VGX_IN_LOCAL_SUM], l64);
                atomicAdd((unsigned long long *)&q[VGX_IN_LOCAL_SUMSQ], l64 * l64);
                atomicMax((long long *)&q[VGX_IN_MAX_LOCAL], (long long)l);
                atomicAdd((unsigned long long *)&spec[(int64_t)dst * VGX_IN_BINS + b], 1ull);
            }
        }
    }
};

template <bool LDS>
__global__ void __launch_bounds__(256) vgxi_lineages_kernel(VgxInLaunch a) {
    __shared__ uint32_t s_c32[LDS ? 4 : 1][LDS ? VGXI_C32 : 1];
    __shared__ unsigned long long s_c64[LDS ? 4 : 1][LDS ? VGXI_C64 : 1];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= a.n) return;   // (the whole wavefront)
    const VgxInDesc d = a.desc[row];
    const int32_t P = (int32_t)a.P;
    int64_t status = a.res ? a.res[row * 5] : 0, arg = a.res ? a.res[row * 5 + 1] : 0;
    Cells<LDS> cells;
    cells.c32 = s_c32[LDS ? wave : 0];
    cells.c64 = s_c64[LDS ? wave : 0];
    cells.tips = a.tips_by_pop + row * P;
    cells.into = a.into + row * P * VGX_IN_INTO;
    cells.spec = a.spectrum + row * P * VGX_IN_BINS;
    int64_t *imp = a.imports + row * P * P;
    if (LDS) {
        for (int k = lane; k < P * VGXI_PER32; k += 64) cells.c32[k] = 0;
        for (int k = lane; k < P * 3; k += 64) cells.c64[k] = 0;
    }
    int64_t st[VGX_IN_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (status == 0) {
        const int64_t o = d.node_off;
        const VgxInWork w{a.w.kids + o, a.w.got + o, a.w.n + o, a.w.ln + o};
        const int32_t *tree = a.tree + o, *pop = a.pop + o;
        int64_t bad = d.nodes;   // a node count that is even or below 3
        int32_t bad_label = INT32_MAX;
        if (d.nodes >= 3 && (d.nodes & 1) && d.nodes <= INT32_MAX) bad = lineage_rounds(tree, pop, (int32_t)d.nodes, P, w, lane, &bad_label);
        if (bad >= 0) { status = VGX_GW_BAD_TREE; arg = bad; }
        else if (bad_label != INT32_MAX) { status = VGX_GW_BAD_LABEL; arg = bad_label; }
        else {
            VGXI_SYNC();   // n[], ln[] and the zeroed LDS cells before the binning
            const int32_t N = (int32_t)d.nodes;
            int64_t intro = 0, empty = 0;
            int32_t maxl = 0, maxc = 0;
            for (int32_t i = lane; i < N - 1; i += 64) {   // every node but the root: every label is inside [0, P) here
                const int32_t dst = pop[i], src = pop[tree[i]];
                const bool tip = ld32(&w.kids[i]) == 0;
                if (tip) cells.tip(dst);
                if (src != dst) {
                    const int32_t c = tip ? 1 : ld32(&w.n[i]), l = tip ? 1 : ld32(&w.ln[i]);
                    atomicAdd((unsigned long long *)&imp[(int64_t)src * P + dst], 1ull);
                    cells.introduction(dst, c, l);
                    intro += 1;
                    empty += l == 0;
                    maxl = l > maxl ? l : maxl;
                    maxc = c > maxc ? c : maxc;
                }
            }
            const int32_t root_local = ld32(&w.ln[N - 1]);   // (the root has two children: N >= 3)
            maxl = wave_max(maxl);
            st[VGX_IN_TIPS] = ld32(&w.n[N - 1]);
            st[VGX_IN_INTRODUCTIONS] = wave_sum(intro);
            st[VGX_IN_ROOT_POP] = pop[N - 1];
            st[VGX_IN_ROOT_LOCAL] = root_local;
            st[VGX_IN_ST_MAX_LOCAL] = root_local > maxl ? root_local : maxl;
            st[VGX_IN_ST_MAX_CLADE] = wave_max(maxc);
            st[VGX_IN_ST_EMPTY] = wave_sum(empty);
        }
    }
    VGXI_SYNC();   // this wavefront's atomics before it reads the cells
    const bool ok = status == 0;
    if (ok) {   // (a tree that is skipped or rejected keeps the zeros the caller wrote)
        int64_t with_tips = 0;
        if (LDS) {
            for (int k = lane; k < P; k += 64) {
                const uint32_t t = cells.c32[k * VGXI_PER32];
                cells.tips[k] = (int64_t)t;
                with_tips += t > 0;
            }
            for (int k = lane; k < P * VGX_IN_INTO; k += 64) {
                const int p = k / VGX_IN_INTO, j = k - p * VGX_IN_INTO;
                const uint32_t *q = cells.c32 + p * VGXI_PER32;
                const unsigned long long *s = cells.c64 + p * 3;
                int64_t v = (int64_t)q[1];
                v = j == VGX_IN_CLADE_SUM ? (int64_t)s[0] : v;
                v = j == VGX_IN_LOCAL_SUM ? (int64_t)s[1] : v;
                v = j == VGX_IN_LOCAL_SUMSQ ? (int64_t)s[2] : v;
                v = j == VGX_IN_EMPTY ? (int64_t)q[2] : v;
                v = j == VGX_IN_MAX_LOCAL ? (int64_t)q[3] : v;
                cells.into[k] = v;
            }
            for (int k = lane; k < P * VGX_IN_BINS; k += 64) {
                const int p = k / VGX_IN_BINS, b = k - p * VGX_IN_BINS;
                cells.spec[k] = (int64_t)cells.c32[p * VGXI_PER32 + 4 + b];
            }
        } else {
            for (int k = lane; k < P; k += 64) with_tips += ld64(&cells.tips[k]) > 0;
        }
        st[VGX_IN_POPS_WITH_TIPS] = wave_sum(with_tips);
    }
    if (lane < VGX_IN_STATS) {
        int64_t v = st[0];
#pragma unroll
        for (int k = 1; k < VGX_IN_STATS; k++) v = lane == k ? st[k] : v;
        a.stats[row * VGX_IN_STATS + lane] = ok ? v : 0;
    }
    if (lane < 2) a.status[row * 2 + lane] = lane == 0 ? status : arg;
}

using namespace vgxtc;

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_in_lineages(const VgxInLaunch *a, hipStream_t s) {
    if (a->P < 1 || a->P > VGX_IN_POPS_MAX) return hipErrorInvalidValue;
    if (a->n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    if (a->P <= VGX_IN_LDS_POPS) hipLaunchKernelGGL(vgxi_lineages_kernel<true>, grid, block, 0, s, *a);   // (the LDS cells are sized for 32 populations)
    else hipLaunchKernelGGL(vgxi_lineages_kernel<false>, grid, block, 0, s, *a);
    return hipGetLastError();
}

// ---- the tau call: the frame of vgx_get_tau_mutation_spectrum with the lineage kernel ----------------------------------------------
// Per pass, on one stream: the canonicalise kernel of vgx_tau_genealogies.hip, its report (the one host step inside a pass: it sizes
// the walk's table and arena), the walk kernel as it is, the lineage kernel.  Nothing of a tree or a label comes to the host.
extern "C" int vgx_get_tau_introductions(vgx_engine *e, vgx_tau_introductions_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->tips_by_pop || !io->imports || !io->into || !io->spectrum || !io->stats ||
                       !io->status || !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_introductions: ";
    io->passes = 0;
    io->pops = e->d.popNum;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    io->kernel_ms[0] = io->kernel_ms[1] = io->kernel_ms[2] = 0.0;
    // preconditions and refusals: those of vgx_get_tau_genealogies
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (walks tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, PH = P * H, mev_cap = e->tau_mev_cap;
    if (P < 1 || P > VGX_IN_POPS_MAX)
        return fail(e, VGX_ERR_ARG, me + "the model has " + std::to_string(P) + " populations (1 .. " + std::to_string(VGX_IN_POPS_MAX) + ": a row holds popNum^2 cells)");
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
    const int64_t cells = vgx_in_row_cells(P), row_bytes = 8 * (cells + 2);
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
                           nodes * (16 + VGX_IN_NODE_BYTES) + mut_need(i) * 20 + mig_need(i) * 16 +
                           (int64_t)(sizeof(VgxGtDesc) + sizeof(VgxGtCanonDesc) + sizeof(VgxGtCanonStat) + sizeof(VgxInDesc)) + row_bytes + 2048;
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

        // ---- walk, lineages: the walk's [desc | res | rng | key | cnt | base | len | lcap | arena | fresh | node x3 | mut x5 | mig x4],
        // then [tree descs | kids, got, n, ln | tips_by_pop | imports | into | spectrum | stats | status]
        t_host = std::chrono::steady_clock::now();
        std::vector<VgxGtDesc> dp((size_t)m);
        std::vector<VgxInDesc> md((size_t)m);
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
            md[(size_t)j] = VgxInDesc{N, nodes_of(gi)};
            T += d.tsize; A += d.arena_cap; N += nodes_of(gi); M += d.mut_cap; G += d.mig_cap;
        }
        io->ms[1] += since(t_host);
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGtDesc)), o_rng = o_res + up8(m * 40), o_key = o_rng + up8(m * 48),
                      o_cnt2 = o_key + up8(T * 8), o_base = o_cnt2 + up8(T * 8), o_len = o_base + up8(T * 4), o_lcap = o_len + up8(T * 4),
                      o_arena = o_lcap + up8(T * 4), o_fresh = o_arena + up8(A * 4), o_out = o_fresh + up8(N * 4),
                      o_md = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_w32 = o_md + up8(m * (int64_t)sizeof(VgxInDesc)),
                      o_tp = o_w32 + up8(4 * N * 4), o_imp = o_tp + up8(m * P * 8), o_into = o_imp + up8(m * P * P * 8),
                      o_sp = o_into + up8(m * P * VGX_IN_INTO * 8), o_stats = o_sp + up8(m * P * VGX_IN_BINS * 8),
                      o_status = o_stats + up8(m * VGX_IN_STATS * 8), total = o_status + up8(m * 16);
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
        VgxInLaunch b{};
        b.n = m;
        b.desc = (const VgxInDesc *)(ws + o_md);
        b.res = a.res;
        b.tree = a.tree; b.pop = a.tree_pop;
        b.P = P;
        int32_t *w32 = (int32_t *)(ws + o_w32);
        b.w = VgxInWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N};
        b.tips_by_pop = (int64_t *)(ws + o_tp); b.imports = (int64_t *)(ws + o_imp); b.into = (int64_t *)(ws + o_into);
        b.spectrum = (int64_t *)(ws + o_sp); b.stats = (int64_t *)(ws + o_stats); b.status = (int64_t *)(ws + o_status);
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGtDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_md, md.data(), (size_t)m * sizeof(VgxInDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipMemsetAsync(ws + o_tp, 0, (size_t)(o_stats - o_tp), e->stream));   // the rows: counted in place
        // walk and lineages with no host step between them
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_tg_walk(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        HIPCHECK(e, vgxi_in_lineages(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        std::vector<int64_t> st2((size_t)m * 2);
        HIPCHECK(e, hipMemcpyAsync(io->tips_by_pop + i0 * P, b.tips_by_pop, (size_t)(m * P) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->imports + i0 * P * P, b.imports, (size_t)(m * P * P) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->into + i0 * P * VGX_IN_INTO, b.into, (size_t)(m * P * VGX_IN_INTO) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->spectrum + i0 * P * VGX_IN_BINS, b.spectrum, (size_t)(m * P * VGX_IN_BINS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->stats + i0 * VGX_IN_STATS, b.stats, (size_t)m * VGX_IN_STATS * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(st2.data(), b.status, (size_t)m * 16, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 6, a.rng_out, (size_t)m * 48, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // before anything reads the rows
            return fail(e, VGX_ERR_HIP, me + "walk or lineage kernel failed: " + hipGetErrorString(er));
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

// ---- test hook: given trees and labels through the kernel (no engine) ------------------------------------------------------------------
extern "C" int vgx_test_introductions_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int32_t *pop, int64_t pops,
                                             const int64_t *walk_status, int64_t *tips_by_pop, int64_t *imports, int64_t *into, int64_t *spectrum,
                                             int64_t *stats, int64_t *status, char *errbuf, int64_t errcap) {
    auto fail_ = [&](int code, const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return code;
    };
    const std::string me = "vgx_test_introductions_device: ";
    if (n < 0 || (n > 0 && (!node_off || !tree || !pop || !tips_by_pop || !imports || !into || !spectrum || !stats || !status))) return fail_(VGX_ERR_ARG, me + "null argument");
    if (pops < 1 || pops > VGX_IN_POPS_MAX) return fail_(VGX_ERR_ARG, me + "populations = " + std::to_string(pops) + " (1 .. " + std::to_string(VGX_IN_POPS_MAX) + ")");
    if (n == 0) return VGX_OK;
    if (node_off[0] != 0) return fail_(VGX_ERR_ARG, me + "node_off[0] must be 0");
    // every array the kernel indexes is bounded here: the tree by its parents; a label is compared on the device before it is used
    std::vector<VgxInDesc> dp((size_t)n);
    std::vector<int64_t> res;
    if (walk_status) res.assign((size_t)n * 5, 0);
    for (int64_t t = 0; t < n; t++) {
        const int64_t N = node_off[t + 1] - node_off[t];
        if (N < 0) return fail_(VGX_ERR_ARG, me + "node_off must not decrease");
        const int64_t bad = vgx_ts_check_parents(tree + node_off[t], N);
        if (bad == N) return fail_(VGX_ERR_ARG, me + "tree " + std::to_string(t) + " has " + std::to_string(N) + " nodes: an odd number, at least 3");
        if (bad >= 0)
            return fail_(VGX_ERR_ARG, me + "tree " + std::to_string(t) + ": the parent of node " + std::to_string(bad) + " is " +
                                          std::to_string(tree[node_off[t] + bad]) + " (a higher id inside the tree, -1 at the last node)");
        dp[(size_t)t] = VgxInDesc{node_off[t], N};
        if (walk_status) {
            res[(size_t)(t * 5)] = walk_status[2 * t]; res[(size_t)(t * 5 + 1)] = walk_status[2 * t + 1];
            res[(size_t)(t * 5 + 2)] = N;
        }
    }
    const int64_t T = node_off[n], P = pops;
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t o_desc = 0, o_res = o_desc + up(n * (int64_t)sizeof(VgxInDesc)), o_tree = o_res + up(n * 40), o_pop = o_tree + up(T * 4),
                  o_w32 = o_pop + up(T * 4), o_tp = o_w32 + up(4 * T * 4), o_imp = o_tp + up(n * P * 8), o_into = o_imp + up(n * P * P * 8),
                  o_sp = o_into + up(n * P * VGX_IN_INTO * 8), o_stats = o_sp + up(n * P * VGX_IN_BINS * 8), o_status = o_stats + up(n * VGX_IN_STATS * 8),
                  total = o_status + up(n * 16);
    char *ws = nullptr;
    hipError_t er = hipMalloc((void **)&ws, (size_t)total);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
    VgxInLaunch a{};
    a.n = n;
    a.desc = (const VgxInDesc *)(ws + o_desc);
    a.res = walk_status ? (const int64_t *)(ws + o_res) : nullptr;
    a.tree = (const int32_t *)(ws + o_tree); a.pop = (const int32_t *)(ws + o_pop);
    a.P = P;
    int32_t *w32 = (int32_t *)(ws + o_w32);
    a.w = VgxInWork{w32, w32 + T, w32 + 2 * T, w32 + 3 * T};
    a.tips_by_pop = (int64_t *)(ws + o_tp); a.imports = (int64_t *)(ws + o_imp); a.into = (int64_t *)(ws + o_into);
    a.spectrum = (int64_t *)(ws + o_sp); a.stats = (int64_t *)(ws + o_stats); a.status = (int64_t *)(ws + o_status);
    er = hipMemcpy(ws + o_desc, dp.data(), (size_t)n * sizeof(VgxInDesc), hipMemcpyHostToDevice);
    if (er == hipSuccess && walk_status) er = hipMemcpy(ws + o_res, res.data(), (size_t)n * 40, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_tree, tree, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_pop, pop, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemset(ws + o_tp, 0, (size_t)(o_stats - o_tp));   // the rows: counted in place
    if (er == hipSuccess) er = vgxi_in_lineages(&a, nullptr);
    if (er == hipSuccess) er = hipStreamSynchronize(nullptr);
    if (er == hipSuccess) er = hipMemcpy(tips_by_pop, a.tips_by_pop, (size_t)(n * P) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(imports, a.imports, (size_t)(n * P * P) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(into, a.into, (size_t)(n * P * VGX_IN_INTO) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(spectrum, a.spectrum, (size_t)(n * P * VGX_IN_BINS) * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(stats, a.stats, (size_t)n * VGX_IN_STATS * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(status, a.status, (size_t)n * 16, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (er != hipSuccess) return fail_(VGX_ERR_HIP, me + hipGetErrorString(er));
    return VGX_OK;
}
