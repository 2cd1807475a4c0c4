// vgx_tree_shapes.hip — the shape kernel of vgx_get_tree_shapes: every tree the walk of vgx_gwalk.h left on the device reduced where
// it lies to the row of vgx_tree_shape.h (12 integer statistics, 7 lengths).  DESIGN.md §29.
//
// One wavefront per tree, four trees per workgroup of 256 threads, no LDS.  The per-node accumulators (n, h, lad, tipkids, minkid,
// kids, got as int32, A and B as int64) live in the pass's global workspace and the kernel initialises them.  A first parallel pass
// checks every parent (i < tree[i] < N: nothing below indexes outside the tree) and counts the children, kids[tree[i]] += 1.  The
// sweep then takes 64 consecutive nodes per round in ascending id: a lane is ready when got[i] == kids[i] (all its children have
// pushed), ready lanes finalise their node, add it to their own partial statistics and push into the parent with atomics, and the
// round repeats under a ballot until its 64 lanes are done.  The lowest unfinished node of a round has all its children in earlier
// rounds or in lower lanes, which have pushed: every iteration finishes at least one lane, a round takes at most 64 iterations (a
// caterpillar tree: the sequential case) and the loop is bounded by that.  The branch terms have no dependencies: a lane adds its
// node's when it finalises it.  The partials are reduced across the wavefront at the end and lane 0 writes the row.
//
// Memory order inside the wavefront: the pushes are relaxed atomics, performed at the L2; VGXS_SYNC waits for every vector-memory
// operation of the wavefront (s_waitcnt vmcnt(0): the atomics have been acknowledged) before the next iteration issues, and the
// accumulators are read back with atomic loads that go to the L2 and not to the vector L1, which may hold the line from before.
// No other wavefront touches a tree's accumulators.  (Lane 0 running vgx_ts_sweep, the host's loop, on the same workspace was
// measured at 7 times the rounds' time on 4096 trees of 2800 tips and is not kept: DESIGN.md §29.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_tree_shape.h"
#include "vgx_wave.h"

namespace {

#define VGXS_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   \
        __builtin_amdgcn_wave_barrier();                         \
    } while (0)

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
__device__ __forceinline__ double wave_max(double v) {
    for (int d = 32; d > 0; d >>= 1) { const double o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v, int lane) { return bcast_i64(iscan(v, lane), 63); }
__device__ __forceinline__ double wave_sum(double v) { return bcast(fscan(v), 63); }

// The 64-lane rounds over one tree (all 64 lanes, wave-uniform control flow).  Returns -1 and the two blocks (wave-uniform), or the
// first node that breaks the precondition.
__device__ int64_t shape_rounds(const int32_t *tree, const int32_t *node_ev, const double *times, const int32_t N, const VgxTsWork &w,
                                const int lane, int64_t *st, double *ln) {
    int32_t bad = INT32_MAX;
    for (int32_t i = lane; i < N; i += 64) {
        const int32_t p = tree[i];
        if (i == N - 1 ? p != -1 : (p <= i || p >= N)) bad = i < bad ? i : bad;
        w.n[i] = 0; w.h[i] = 0; w.lad[i] = 0; w.tipkids[i] = 0; w.minkid[i] = INT32_MAX; w.kids[i] = 0; w.got[i] = 0;
        w.A[i] = 0; w.B[i] = 0;
    }
    bad = wave_min(bad);
    if (bad != INT32_MAX) return bad;
    VGXS_SYNC();
    for (int32_t i = lane; i < N - 1; i += 64) atomicAdd(&w.kids[tree[i]], 1);
    VGXS_SYNC();
    const double t_root = times[N - 1];
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
                VgxTsNode v;
                if (tip) { v.n = 1; v.h = 0; v.lad = 0; v.tipkids = 0; v.minkid = 0; v.A = 0; v.B = 0; }
                else {
                    v.n = ld32(&w.n[i]); v.h = ld32(&w.h[i]); v.tipkids = ld32(&w.tipkids[i]); v.minkid = ld32(&w.minkid[i]);
                    v.A = ld64(&w.A[i]); v.B = ld64(&w.B[i]);
                    v.lad = v.tipkids == 1 ? ld32(&w.lad[i]) : 0;
                }
                vgx_ts_count(v, tip, st);
                if (i == N - 1) {
                    st[VGX_TS_SACKIN] = v.A; st[VGX_TS_MAX_DEPTH] = v.h; st[VGX_TS_DEPTH_SUMSQ] = v.B;
                } else {
                    const int32_t p = tree[i];
                    atomicAdd(&w.n[p], v.n);
                    atomicAdd((unsigned long long *)&w.A[p], (unsigned long long)v.A + (unsigned long long)v.n);
                    atomicAdd((unsigned long long *)&w.B[p], (unsigned long long)v.B + 2 * (unsigned long long)v.A + (unsigned long long)v.n);
                    atomicMax(&w.h[p], v.h + 1);
                    if (tip) atomicAdd(&w.tipkids[p], 1);
                    atomicMin(&w.minkid[p], v.n);
                    atomicMax(&w.lad[p], v.lad + 1);
                    atomicAdd(&w.got[p], 1);
                    vgx_ts_branch(times[i], times[p], t_root, tip, ln);
                }
                todo = false;
            }
            VGXS_SYNC();
            if (!__ballot(todo)) break;
        }
        if (__ballot(todo)) return wave_min(todo ? i : INT32_MAX);   // (not with the child counts checked above: the loop's bound)
    }
    // the partials of the 64 lanes: sums, and the two maxima
    const int sums[9] = {VGX_TS_TIPS, VGX_TS_INTERNAL, VGX_TS_CHERRIES, VGX_TS_PITCHFORKS, VGX_TS_SACKIN, VGX_TS_COLLESS, VGX_TS_MAX_DEPTH,
                         VGX_TS_DEPTH_SUMSQ, VGX_TS_LADDER_NODES};   // (sackin, max_depth, depth_sumsq: the root's lane alone holds them)
#pragma unroll
    for (int k = 0; k < 9; k++) st[sums[k]] = wave_sum(st[sums[k]], lane);
    st[VGX_TS_MAX_LADDER] = wave_max((int32_t)st[VGX_TS_MAX_LADDER]);
    st[VGX_TS_ROOT_EVENT] = node_ev[N - 1];
    st[VGX_TS_LAST_TIP_EVENT] = node_ev[0];
    ln[VGX_TS_LENGTH] = wave_sum(ln[VGX_TS_LENGTH]);
    ln[VGX_TS_EXTERNAL_LENGTH] = wave_sum(ln[VGX_TS_EXTERNAL_LENGTH]);
    ln[VGX_TS_LENGTH_SUMSQ] = wave_sum(ln[VGX_TS_LENGTH_SUMSQ]);
    ln[VGX_TS_TIP_HEIGHT_SUM] = wave_sum(ln[VGX_TS_TIP_HEIGHT_SUM]);
    ln[VGX_TS_MAX_BRANCH] = wave_max(ln[VGX_TS_MAX_BRANCH]);
    ln[VGX_TS_ROOT_TIME] = t_root;
    ln[VGX_TS_LAST_TIP_TIME] = times[0];
    return -1;
}

__global__ void __launch_bounds__(256) vgxs_shape_kernel(VgxTsLaunch a) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= a.n) return;   // (the whole wavefront)
    const VgxTsDesc d = a.desc[row];
    int64_t status = a.res ? a.res[row * 5] : 0, arg = a.res ? a.res[row * 5 + 1] : 0;
    int64_t st[VGX_TS_K];
    double ln[VGX_TS_L];
    for (int k = 0; k < VGX_TS_K; k++) st[k] = 0;
    for (int k = 0; k < VGX_TS_L; k++) ln[k] = 0.0;
    if (status == 0) {
        const int64_t o = d.node_off;
        const VgxTsWork w{a.w.n + o, a.w.h + o, a.w.lad + o, a.w.tipkids + o, a.w.minkid + o, a.w.kids + o, a.w.got + o, a.w.A + o, a.w.B + o};
        int64_t bad = d.nodes;   // a node count that is even or below 3
        if (d.nodes >= 3 && (d.nodes & 1) && d.nodes <= INT32_MAX)
            bad = shape_rounds(a.tree + o, a.node_ev + o, a.times + o, (int32_t)d.nodes, w, lane, st, ln);
        if (bad >= 0) { status = VGX_GW_BAD_TREE; arg = bad; }
    }
    if (lane == 0) {
        const bool ok = status == 0;
        for (int k = 0; k < VGX_TS_K; k++) a.stats[row * VGX_TS_K + k] = ok ? st[k] : 0;
        for (int k = 0; k < VGX_TS_L; k++) a.lengths[row * VGX_TS_L + k] = ok ? ln[k] : NAN;
        a.status[row * 2] = status;
        a.status[row * 2 + 1] = arg;
    }
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_ts_shape(const VgxTsLaunch *a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxs_shape_kernel, dim3((unsigned)((a->n + 3) / 4)), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// ---- test hook: given trees through the kernel (no engine) ----------------------------------------------------------------------
extern "C" int vgx_test_tree_shape_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int32_t *node_ev, const double *times,
                                          int64_t *stats, double *lengths, int64_t *status, char *errbuf, int64_t errcap) {
    auto fail = [&](int code, const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return code;
    };
    const std::string me = "vgx_test_tree_shape_device: ";
    if (n < 0 || (n > 0 && (!node_off || !tree || !node_ev || !times || !stats || !lengths || !status))) return fail(VGX_ERR_ARG, me + "null argument");
    if (n == 0) return VGX_OK;
    if (node_off[0] != 0) return fail(VGX_ERR_ARG, me + "node_off[0] must be 0");
    std::vector<VgxTsDesc> dp((size_t)n);
    for (int64_t t = 0; t < n; t++) {
        const int64_t N = node_off[t + 1] - node_off[t];
        if (N < 0) return fail(VGX_ERR_ARG, me + "node_off must not decrease");
        const int64_t bad = vgx_ts_check_parents(tree + node_off[t], N);
        if (bad == N) return fail(VGX_ERR_ARG, me + "tree " + std::to_string(t) + " has " + std::to_string(N) + " nodes: an odd number, at least 3");
        if (bad >= 0)
            return fail(VGX_ERR_ARG, me + "tree " + std::to_string(t) + ": the parent of node " + std::to_string(bad) + " is " +
                                         std::to_string(tree[node_off[t] + bad]) + " (a higher id inside the tree, -1 at the last node)");
        dp[(size_t)t] = VgxTsDesc{node_off[t], N};
    }
    const int64_t T = node_off[n];
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t o_desc = 0, o_tree = o_desc + up(n * (int64_t)sizeof(VgxTsDesc)), o_nev = o_tree + up(T * 4), o_times = o_nev + up(T * 4),
                  o_w64 = o_times + up(T * 8), o_w32 = o_w64 + up(2 * T * 8), o_stats = o_w32 + up(7 * T * 4),
                  o_len = o_stats + up(n * VGX_TS_K * 8), o_status = o_len + up(n * VGX_TS_L * 8), total = o_status + up(n * 16);
    char *ws = nullptr;
    hipError_t er = hipMalloc((void **)&ws, (size_t)total);
    if (er != hipSuccess) return fail(VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
    VgxTsLaunch a{};
    a.n = n;
    a.desc = (const VgxTsDesc *)(ws + o_desc);
    a.res = nullptr;
    a.tree = (const int32_t *)(ws + o_tree); a.node_ev = (const int32_t *)(ws + o_nev); a.times = (const double *)(ws + o_times);
    int32_t *w32 = (int32_t *)(ws + o_w32);
    int64_t *w64 = (int64_t *)(ws + o_w64);
    a.w = VgxTsWork{w32, w32 + T, w32 + 2 * T, w32 + 3 * T, w32 + 4 * T, w32 + 5 * T, w32 + 6 * T, w64, w64 + T};
    a.stats = (int64_t *)(ws + o_stats); a.lengths = (double *)(ws + o_len); a.status = (int64_t *)(ws + o_status);
    er = hipMemcpy(ws + o_desc, dp.data(), (size_t)n * sizeof(VgxTsDesc), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_tree, tree, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_nev, node_ev, (size_t)T * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(ws + o_times, times, (size_t)T * 8, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = vgxi_ts_shape(&a, nullptr);
    if (er == hipSuccess) er = hipStreamSynchronize(nullptr);
    if (er == hipSuccess) er = hipMemcpy(stats, a.stats, (size_t)n * VGX_TS_K * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(lengths, a.lengths, (size_t)n * VGX_TS_L * 8, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(status, a.status, (size_t)n * 16, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (er != hipSuccess) return fail(VGX_ERR_HIP, me + hipGetErrorString(er));
    return VGX_OK;
}
