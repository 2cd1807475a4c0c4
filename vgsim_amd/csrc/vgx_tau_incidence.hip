// vgx_tau_incidence.hip — event counts per time bin, population and channel of every selected replicate of a TAU ensemble on
// the device (vgx_get_tau_incidence), the host side of that call, and the same rule and tile walk compiled for the host
// (vgx_test_tau_incidence).  The rule is vgx_tau_incidence.h; DESIGN.md §17.
//
// COUNTING kernel.  A workgroup of 256 threads takes one chain (a selected replicate's own rows in its block of t_mev, or the
// flattened prefix) and a TILE of consecutive rows, so that one long chain spreads over the whole device.  Consecutive lanes read
// consecutive rows (three 16-byte loads per lane: every byte of a fetched line is used).  The tile is clipped to the window
// [cut[0], cut[T]); its first bin comes from a search in the chain's cuts, read where they lie; bin by bin `num` is added to an
// int64 histogram of P * 7 cells in LDS with 64-bit LDS atomics, and at every bin change and at the tile's end the nonzero cells
// go to the block in device memory with 64-bit integer atomics and are cleared.  Rows outside the window are not skipped: every
// thread sums their positive num, and at the end a wave sum and one global atomic per wavefront feed the chain's two `outside`
// counters.  All arithmetic is integer: the block does not depend on the tile size or the launch geometry.
// The tile size (VGX_INCIDENCE_TILE_EVENTS, rows here; default 4096) is the one DESIGN.md §16 reasons out for the direct kernel
// (16 rows per thread amortise the search and the flush, a chain of 10^6 rows still gives 244 workgroups); it is not the result
// of a sweep.
// The prefix is counted ONCE per call as a chain of its own; an init kernel then starts the block of every selected replicate
// that did not restart from the prefix block, and the replicates' own rows are added on top.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_tau_incidence.h"
#include "vgx_tau_replay.h"   // the frame: selection, cuts, workspace, prefix pass, chunks, summary, the hook's chain split

namespace {

__global__ void __launch_bounds__(256) vgxti_count_kernel(VgxTauIncLaunch a) {
    extern __shared__ __attribute__((aligned(16))) long long hist[];   // [P][7]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_rows[row], T = a.T, P = a.P, cells = P * VGX_INC_CHANNELS;
    const int32_t *cut = a.cut + row * (int64_t)(T + 1);   // (uniform addresses: every thread reads the same cuts)
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *rows = (const longlong2 *)(a.rows + (a.rep ? a.rep[row] * a.stride * 6 : 0));
    long long *out = (long long *)a.counts + row * (int64_t)T * cells, *outside = (long long *)a.outside + 2 * row;
    long long before = 0, after = 0;       // this thread's share of the rows outside the window
    bool clean = false;                    // the histogram is zeroed before the first tile that counts
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e0 = (int32_t)t0, e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t b1, a0;
        vgx_tau_inc_outside(cut, T, e0, e1, b1, a0);
        for (int64_t e = (int64_t)e0 + tid; e < b1; e += 256) {   // (only num is needed: the row's first 16 bytes)
            const long long w = rows[e * 3].x;
            if (w > 0) before += w;
        }
        for (int64_t e = (int64_t)a0 + tid; e < e1; e += 256) {
            const long long w = rows[e * 3].x;
            if (w > 0) after += w;
        }
        int32_t pos, hi;
        vgx_inc_clip(cut, T, e0, e1, pos, hi);
        if (pos >= hi) continue;           // (the whole workgroup: nothing of the tile lies inside the window)
        if (!clean) {
            for (int i = tid; i < cells; i += 256) hist[i] = 0;
            clean = true;
            __syncthreads();
        }
        while (pos < hi) {
            const int32_t b = vgx_inc_bin(cut, T, pos);
            const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
            for (int64_t e = (int64_t)pos + tid; e < end; e += 256) {
                const longlong2 r0 = rows[e * 3], r1 = rows[e * 3 + 1], r2 = rows[e * 3 + 2];
                int32_t cell[2];
                int k;
                const long long w = vgx_tau_inc_row(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, P, a.hapNum, a.mask, cell, k);
                if (k > 0) add64(&hist[cell[0]], w);
                if (k > 1) add64(&hist[cell[1]], w);
            }
            __syncthreads();
            long long *dst = out + (int64_t)b * cells;
            for (int i = tid; i < cells; i += 256) {
                const long long v = hist[i];
                if (v) { add64(&dst[i], v); hist[i] = 0; }
            }
            __syncthreads();
            pos = end;
        }
    }
    before = wave_sum(before);
    after = wave_sum(after);
    if (lane == 0) {
        if (before) add64(&outside[0], before);
        if (after) add64(&outside[1], after);
    }
}

hipError_t launch_count(const VgxTauIncLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    const int64_t lds = vgx_tau_inc_lds_bytes(a->P);
    if (lds > VGX_INC_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxti_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxti_count_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a);
    return hipGetLastError();
}

// what both the call and the hook check about the grid and the dimensions; "" or why not
std::string check_grid(const double *edges, int64_t T, int64_t P) {
    if (T < 1 || T >= VGX_INC_MAX_BINS || !edges) return "T = " + std::to_string(T) + " bins: at least 1, below 2^24, with edges";
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(edges[k])) return "edges[" + std::to_string(k) + "] is not finite";
        if (k > 0 && !(edges[k - 1] < edges[k])) return "edges must increase strictly (edges[" + std::to_string(k) + "])";
    }
    if (vgx_tau_inc_lds_bytes(P) > VGX_INC_LDS_MAX)
        return std::to_string(P) + " populations need " + std::to_string(vgx_tau_inc_lds_bytes(P)) + " bytes of counters, above the " +
               std::to_string((int64_t)VGX_INC_LDS_MAX) + " bytes of LDS a counting workgroup may use";
    return "";
}

}  // namespace

extern "C" int vgx_get_tau_incidence(vgx_engine *e, vgx_tau_incidence_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_incidence: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, cells = P * VGX_INC_CHANNELS, tc = T * cells, mev_cap = e->tau_mev_cap;
    TauSel sel;
    if (const int rc = tau_select(e, me, "counts", [&]() { return check_grid(io->edges, T, P); }, n, io->replicates, prefix, false, tau_every, sel)) return rc;
    const int64_t pre_rows = sel.pre_rows;
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    int64_t tile = VGX_INC_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_INCIDENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_INC_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    // what stays for the whole call: [rep | n_own | with | mask | prefix: rows, cut, n_rows, block, outside | counts | outside | narrow | min, max]
    const int64_t mask_words = (H + 31) / 32, block_bytes = n * tc * 8, narrow_bytes = io->summary ? n * tc * 4 : 0;
    DevLayout lay;
    const int64_t o_rep = lay.take(n * 8), o_nown = lay.take(n * 4), o_with = lay.take(n * 4), o_mask = lay.take(mask_words * 4),
                  o_prow = lay.take(pre_rows * 48 + 8), o_pcut = lay.take((T + 1) * 4), o_pn = lay.take(4), o_pcnt = lay.take(tc * 8), o_pout = lay.take(16),
                  o_cnt = lay.take(block_bytes), o_out = lay.take(n * 16), o_nar = lay.take(narrow_bytes + 8), o_mm = lay.take(16), keep_total = lay.total;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x 7 counts of 8 bytes, the prefix rows and " +
                                        (io->summary ? "the summary's 4-byte copy take " : "their counters take ") + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    DevHold khold;
    if (const int rc = dev_alloc(e, me, keep_total, khold)) return rc;
    char *const kws = khold.get();
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, sel.n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_with, sel.with_prefix.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    if (io->hap_mask) HIPCHECK(e, hipMemcpyAsync(kws + o_mask, io->hap_mask, (size_t)mask_words * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_pcnt, 0, (size_t)(o_cnt - o_pcnt), e->stream));   // the prefix block and its outside counters
    VgxTauIncLaunch base{};   // what every launch of the call shares
    base.T = (int32_t)T; base.P = (int32_t)P; base.hapNum = (int32_t)H; base.tile = (int32_t)tile;
    base.mask = io->hap_mask ? (const uint32_t *)(kws + o_mask) : nullptr;

    // the prefix, once: flattened rows uploaded, its cuts, counted as a chain of its own
    int64_t point0 = 0;
    int rc = tau_prefix_pass<VgxIncCutter, 0>(e, me, io->ms, sel, prefix ? prefix->ev_times : nullptr, io->edges, T, kws + o_prow, kws + o_pcut, kws + o_pn, point0, [&]() -> int {
        VgxTauIncLaunch a = base;
        a.m = 1;
        a.rows = (const int64_t *)(kws + o_prow); a.stride = 0; a.rep = nullptr;
        a.n_rows = (const int32_t *)(kws + o_pn); a.cut = (const int32_t *)(kws + o_pcut);
        a.max_n = pre_rows;
        a.counts = (int64_t *)(kws + o_pcnt); a.outside = (int64_t *)(kws + o_pout);
        HIPCHECK(e, launch_count(&a, e->stream));
        if (pre_rows > 0) io->passes += 1;
        return VGX_OK;
    });
    if (rc) return rc;
    // chunks of replicates: their blocks start from the prefix's or from zero, their own rows are counted on top
    rc = tau_chunks<VgxIncCutter, 0>(e, me, me + "counting kernel failed: ", io->ms, sel, n, io->replicates, io->edges, T, point0, (int64_t)(free_b / 2) - keep_total,
                                     [&](int64_t i0, int64_t m, int64_t max_n, const int32_t *cuts) -> int {
        VgxTauIncLaunch a = base;
        a.m = m;
        a.rows = (const int64_t *)e->t_mev.p; a.stride = mev_cap;
        a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_rows = (const int32_t *)(kws + o_nown) + i0;
        a.cut = cuts;
        a.max_n = max_n;
        a.counts = (int64_t *)(kws + o_cnt) + i0 * tc; a.outside = (int64_t *)(kws + o_out) + 2 * i0;
        HIPCHECK(e, vgxi_tau_block_init(m, tc, 0, (const int32_t *)(kws + o_with) + i0, (const int64_t *)(kws + o_pcnt), nullptr, (const int64_t *)(kws + o_pout),
                                        a.counts, nullptr, a.outside, e->stream));
        HIPCHECK(e, launch_count(&a, e->stream));
        if (max_n > 0) io->passes += 1;
        return VGX_OK;
    });
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(io->outside, kws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (io->counts) HIPCHECK(e, hipMemcpy(io->counts, kws + o_cnt, (size_t)block_bytes, hipMemcpyDeviceToHost));
    if (io->summary)
        if ((rc = tau_summary(e, me, true, (const int64_t *)(kws + o_cnt), n, tc, (int32_t *)(kws + o_nar), (uint64_t *)(kws + o_mm), io->summary, io->ms))) return rc;
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, cuts, cells and tile walk on a chain given as arrays (no device, no engine).  The
// last n_own_events events play the replicate's own steps, everything before them the prefix, which is counted once as a chain
// of its own and added, as on the device (tau_hook_split, tau_hook_count).
extern "C" int vgx_test_tau_incidence(vgx_tau_incidence_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_incidence: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->counts || !io->outside) return fail_("null argument");
    const int64_t T = io->T, P = io->popNum, H = io->hapNum;
    if (P < 1 || H < 1 || P > INT32_MAX / VGX_INC_CHANNELS || H > INT32_MAX) return fail_("bad dimensions");
    std::string why = check_grid(io->edges, T, P);
    if (!why.empty()) return fail_(why);
    const int64_t cells = P * VGX_INC_CHANNELS;
    TauHookChain c;
    why = tau_hook_split(io, VGX_INC_TILE_DEFAULT, T * cells, c);
    if (!why.empty()) return fail_(why);
    std::vector<int32_t> pcut, ocut;
    tau_hook_marks<VgxIncCutter, 0>(c, io->ev_times, io->edges, T, pcut, ocut);
    std::vector<int64_t> hist((size_t)cells, 0);
    int64_t *const dst[2] = {io->counts, io->outside};
    const int64_t len[2] = {T * cells, 2};
    tau_hook_count(c, pcut.data(), ocut.data(), dst, len, [&](const int64_t *rows, const int32_t *cut, int32_t t0, int32_t t1, int64_t *const *b) {
        vgx_tau_inc_tile_host(rows, cut, (int32_t)T, (int32_t)P, (int32_t)H, io->hap_mask, t0, t1, hist.data(), b[0], b[1]);
    });
    return VGX_OK;
}
