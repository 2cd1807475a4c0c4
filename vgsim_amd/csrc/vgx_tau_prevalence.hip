// vgx_tau_prevalence.hip — infectious hosts per population and variant class of every selected replicate of a TAU ensemble at the
// times of one grid, on the device (vgx_get_tau_prevalence), the host side of that call, and the same rule, tile walk and scan
// compiled for the host (vgx_test_tau_prevalence).  The rule is vgx_tau_prevalence.h; DESIGN.md §19.
//
// COUNTING kernel.  As in vgx_prevalence.hip the stock is formed as the NET change of every (interval, population, class),
// tile-parallel, and summed up per column afterwards.  A workgroup of 256 threads takes one chain (a selected replicate's own rows
// in its block of t_mev, or the flattened prefix) and a TILE of consecutive rows; consecutive lanes read consecutive rows (three
// 16-byte loads per lane).  The tile's first interval comes from a search in the chain's bounds, read where they lie; interval by
// interval the signed num goes into P * V int64 cells in LDS with 64-bit LDS atomics, and at every interval change and at the
// tile's end the nonzero cells go to the net block in device memory with 64-bit atomics and are cleared.  variant_of is staged in
// LDS behind the cells when it fits.  Rows outside [cut[0], cut[T-1]) count like any other (interval 0 or the tail); every thread
// also sums their positive num, and at the end a wave sum and one global atomic per wavefront feed the chain's two `outside`
// counters.  All arithmetic is integer: the block does not depend on the tile size or the launch geometry.
// The prefix is counted ONCE per call as a chain of its own; an INIT kernel starts the net block (value intervals, tail, outside)
// of every selected replicate that did not restart from the prefix's, the replicates' own rows are added on top, and the SCAN
// kernel (one thread per (chain, population, class) column, consecutive threads consecutive classes) turns the net block into
// running sums from the `start` block.  The tile size is VGX_PREVALENCE_TILE_EVENTS (rows here; default 4096, the value DESIGN.md
// §16 reasons out; not the result of a sweep).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_tau_prevalence.h"
#include "vgx_tau_replay.h"   // the frame: selection, bounds, workspace, prefix pass, chunks, summary, the hook's chain split

namespace {

__global__ void __launch_bounds__(256) vgxtp_count_kernel(VgxTauPrevLaunch a, int stage) {
    extern __shared__ __attribute__((aligned(16))) long long hist[];   // [P][V] cells, then (stage) variant_of [hapNum]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_rows[row], T = a.T, P = a.P, V = a.V, cells = P * V;
    if ((int64_t)blockIdx.y * a.tile >= n) return;         // (the whole workgroup: the chain ends before its first tile)
    const int32_t *bound = a.bound + row * (int64_t)(T + 2);   // (uniform addresses: every thread reads the same bounds)
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *rows = (const longlong2 *)(a.rows + (a.rep ? a.rep[row] * a.stride * 6 : 0));
    long long *val = (long long *)a.val, *fin = (long long *)a.fin, *outside = (long long *)a.outside + 2 * row;
    const int32_t *vo = a.variant_of;
    for (int i = tid; i < cells; i += 256) hist[i] = 0;
    if (stage) {
        int32_t *map = (int32_t *)(hist + cells);
        for (int i = tid; i < a.hapNum; i += 256) map[i] = vo[i];
        vo = map;
    }
    __syncthreads();
    const int32_t first = bound[1], last = bound[T];       // rows before `first` / from `last` on are outside the grid
    long long before = 0, after = 0;                       // this thread's share of their positive num
    for (int64_t t0 = (int64_t)blockIdx.y * a.tile; t0 < n; t0 += (int64_t)gridDim.y * a.tile) {
        const int32_t e1 = (int32_t)(t0 + a.tile < n ? t0 + a.tile : n);
        int32_t pos = (int32_t)t0;
        while (pos < e1) {
            const int32_t j = vgx_inc_bin(bound, T + 1, pos);
            const int32_t end = e1 < bound[j + 1] ? e1 : bound[j + 1];
            for (int64_t e = (int64_t)pos + tid; e < end; e += 256) {
                const longlong2 r0 = rows[e * 3], r1 = rows[e * 3 + 1], r2 = rows[e * 3 + 2];
                if (r0.x > 0) {
                    if (e < first) before += r0.x;
                    else if (e >= last) after += r0.x;
                }
                int32_t cell[2], sign[2];
                int k;
                const long long w = vgx_tau_prev_row(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, P, a.hapNum, V, vo, cell, sign, k);
                if (k > 0) add64(&hist[cell[0]], sign[0] < 0 ? -w : w);
                if (k > 1) add64(&hist[cell[1]], sign[1] < 0 ? -w : w);
            }
            __syncthreads();
            long long *dst = (long long *)vgx_tau_prev_net((int64_t *)val, (int64_t *)fin, row, T, cells, j);
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

// one thread per (chain, population, class) column, consecutive threads consecutive classes: every step of the running sum reads
// and writes whole lines
__global__ void __launch_bounds__(256) vgxtp_scan_kernel(VgxTauPrevLaunch a) {
    const int64_t cells = (int64_t)a.P * a.V, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.m * cells) return;
    const int64_t row = idx / cells, cell = idx % cells;
    vgx_tau_prev_scan_column(a.val + row * a.T * cells + cell, a.fin + idx, a.start[idx], a.T, cells);
}

// int64 block -> int32 for the column summary (clamped: a block with a value that does not fit is refused), and the block's
// smallest and largest value: mm[0] = min, mm[1] = max, both with the sign bit flipped so that unsigned order is signed order
// (the caller sets ~0 and 0)
__global__ void __launch_bounds__(256) vgxtp_minmax_kernel(int64_t total, const long long *src, int32_t *dst, unsigned long long *mm) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    long long lo = LLONG_MAX, hi = LLONG_MIN;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long v = src[i];
        dst[i] = (int32_t)(v < INT32_MIN ? INT32_MIN : v > INT32_MAX ? INT32_MAX : v);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&mm[0], (unsigned long long)lo ^ 0x8000000000000000ull);
        atomicMax(&mm[1], (unsigned long long)hi ^ 0x8000000000000000ull);
    }
}

hipError_t launch_count(const VgxTauPrevLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if (vgx_tau_prev_lds_bytes(a->P, a->V) > VGX_PREV_LDS_MAX || a->tile < 1) return hipErrorInvalidValue;
    const bool stage = vgx_tau_prev_stage_map(a->P, a->V, a->hapNum);
    const int64_t lds = vgx_tau_prev_lds_bytes(a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxtp_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtp_count_kernel, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_scan(const VgxTauPrevLaunch *a, hipStream_t s) {
    const int64_t cols = a->m * a->P * a->V;
    if (cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxtp_scan_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// what both the call and the hook check about the grid, the map and the dimensions; "" or why not
std::string check_request(const double *grid, int64_t T, int64_t V, const int32_t *variant_of, int64_t P, int64_t H) {
    if (T < 1 || T >= VGX_PREV_MAX_POINTS || !grid) return "T = " + std::to_string(T) + " grid points: at least 1, below 2^24, with grid";
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(grid[k])) return "grid[" + std::to_string(k) + "] is not finite";
        if (k > 0 && !(grid[k - 1] < grid[k])) return "grid must increase strictly (grid[" + std::to_string(k) + "])";
    }
    if (V < 1 || V > INT32_MAX || !variant_of) return "V = " + std::to_string(V) + " classes: at least 1, with variant_of";
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")";
    if (vgx_tau_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return std::to_string(P) + " populations x " + std::to_string(V) + " classes need " + std::to_string(vgx_tau_prev_lds_bytes(P, V)) +
               " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use";
    return "";
}

}  // namespace

// the count, scan and min/max launches as vgx_tau_susceptible.hip, vgx_tau_milestones.hip and the frame's summary tail share them
// (declared in vgx_engine.h)
extern "C" hipError_t vgxi_tau_prev_count(const VgxTauPrevLaunch *a, hipStream_t s) { return launch_count(a, s); }

extern "C" hipError_t vgxi_tau_prev_scan(const VgxTauPrevLaunch *a, hipStream_t s) { return launch_scan(a, s); }

extern "C" hipError_t vgxi_tau_prev_minmax(int64_t total, const int64_t *src, int32_t *dst, uint64_t *mm, hipStream_t s) {
    hipLaunchKernelGGL(vgxtp_minmax_kernel, dim3(flat_grid(total)), dim3(256), 0, s, total, (const long long *)src, dst, (unsigned long long *)mm);
    return hipGetLastError();
}

extern "C" int vgx_get_tau_prevalence(vgx_engine *e, vgx_tau_prevalence_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_prevalence: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V, mev_cap = e->tau_mev_cap;
    TauSel sel;
    if (const int rc = tau_select(e, me, "counts", [&]() { return check_request(io->grid, T, V, io->variant_of, P, H); }, n, io->replicates, prefix, false, tau_every, sel))
        return rc;
    const int64_t cells = P * V, tc = T * cells, pre_rows = sel.pre_rows;
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    // the state every chain starts from, folded through variant_of: the initial state for a chain that starts at the beginning of
    // the model's history (a restarted replicate, or one that carries a prefix), else the state the call started from
    std::vector<int64_t> start((size_t)(n * cells));
    {
        const std::vector<int64_t> fold[2] = {tau_fold_state(e->hs.infectious, P, H, V, io->variant_of), tau_fold_state(e->hs.initial_infectious, P, H, V, io->variant_of)};
        for (int64_t i = 0; i < n; i++) {
            const std::vector<int64_t> &f = fold[e->sc_host[(size_t)io->replicates[i]].restarts > 0 || sel.pre_ev > 0 ? 1 : 0];
            std::copy(f.begin(), f.end(), start.begin() + i * cells);
        }
    }
    int64_t tile = VGX_PREV_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_PREVALENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    // what stays for the whole call:
    // [rep | n_own | with | variant_of | prefix: rows, bound, n_rows, val, fin, outside | start | val | fin | outside | narrow | min, max]
    const int64_t val_bytes = n * tc * 8, fin_bytes = n * cells * 8, narrow_bytes = io->summary ? n * tc * 4 : 0;
    DevLayout lay;
    const int64_t o_rep = lay.take(n * 8), o_nown = lay.take(n * 4), o_with = lay.take(n * 4), o_map = lay.take(H * 4), o_prow = lay.take(pre_rows * 48 + 8),
                  o_pbnd = lay.take((T + 2) * 4), o_pn = lay.take(4), o_pval = lay.take(tc * 8), o_pfin = lay.take(cells * 8), o_pout = lay.take(16),
                  o_start = lay.take(fin_bytes), o_val = lay.take(val_bytes), o_fin = lay.take(fin_bytes), o_out = lay.take(n * 16),
                  o_nar = lay.take(narrow_bytes + 8), o_mm = lay.take(16), keep_total = lay.total;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(V) +
                                        " values of 8 bytes (" + std::to_string(val_bytes + fin_bytes) + " bytes), the prefix rows, the start and " +
                                        (io->summary ? "the summary's 4-byte copy take " : "the bounds take ") + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    DevHold khold;
    if (const int rc = dev_alloc(e, me, keep_total, khold)) return rc;
    char *const kws = khold.get();
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, sel.n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_with, sel.with_prefix.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)fin_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_pval, 0, (size_t)(o_start - o_pval), e->stream));   // the prefix's net block and its outside counters
    VgxTauPrevLaunch base{};   // what every launch of the call shares
    base.T = (int32_t)T; base.P = (int32_t)P; base.hapNum = (int32_t)H; base.V = (int32_t)V; base.variant_of = (const int32_t *)(kws + o_map);
    base.tile = (int32_t)tile;

    // the prefix, once: flattened rows uploaded, its bounds, counted as a chain of its own
    int64_t point0 = 0;
    int rc = tau_prefix_pass<VgxPrevCutter, 1>(e, me, io->ms, sel, prefix ? prefix->ev_times : nullptr, io->grid, T, kws + o_prow, kws + o_pbnd, kws + o_pn, point0, [&]() -> int {
        VgxTauPrevLaunch a = base;
        a.m = 1;
        a.rows = (const int64_t *)(kws + o_prow); a.stride = 0; a.rep = nullptr;
        a.n_rows = (const int32_t *)(kws + o_pn); a.bound = (const int32_t *)(kws + o_pbnd);
        a.max_n = pre_rows;
        a.val = (int64_t *)(kws + o_pval); a.fin = (int64_t *)(kws + o_pfin); a.outside = (int64_t *)(kws + o_pout);
        HIPCHECK(e, launch_count(&a, e->stream));
        if (pre_rows > 0) io->passes += 1;
        return VGX_OK;
    });
    if (rc) return rc;
    // chunks of replicates: their net blocks start from the prefix's or from zero, their own rows are counted on top, the columns summed up
    rc = tau_chunks<VgxPrevCutter, 1>(e, me, me + "counting or scan kernel failed: ", io->ms, sel, n, io->replicates, io->grid, T, point0,
                                      (int64_t)(free_b / 2) - keep_total, [&](int64_t i0, int64_t m, int64_t max_n, const int32_t *bounds) -> int {
        VgxTauPrevLaunch a = base;
        a.m = m;
        a.rows = (const int64_t *)e->t_mev.p; a.stride = mev_cap;
        a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_rows = (const int32_t *)(kws + o_nown) + i0;
        a.bound = bounds;
        a.max_n = max_n;
        a.val = (int64_t *)(kws + o_val) + i0 * tc; a.fin = (int64_t *)(kws + o_fin) + i0 * cells; a.outside = (int64_t *)(kws + o_out) + 2 * i0;
        a.start = (const int64_t *)(kws + o_start) + i0 * cells;
        HIPCHECK(e, vgxi_tau_block_init(m, tc, cells, (const int32_t *)(kws + o_with) + i0, (const int64_t *)(kws + o_pval), (const int64_t *)(kws + o_pfin),
                                        (const int64_t *)(kws + o_pout), a.val, a.fin, a.outside, e->stream));
        HIPCHECK(e, launch_count(&a, e->stream));
        if (max_n > 0) io->passes += 1;
        HIPCHECK(e, launch_scan(&a, e->stream));
        return VGX_OK;
    });
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(io->outside, kws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (io->final) HIPCHECK(e, hipMemcpy(io->final, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary)
        if ((rc = tau_summary(e, me, false, (const int64_t *)(kws + o_val), n, tc, (int32_t *)(kws + o_nar), (uint64_t *)(kws + o_mm), io->summary, io->ms))) return rc;
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, bounds, cells, tile walk, prefix-plus-own sum and scan on a chain given as arrays (no
// device, no engine).  The last n_own_events events play the replicate's own steps, everything before them the prefix, which is
// counted once as a chain of its own; the chain's net block starts from the prefix's, as on the device (tau_hook_split,
// tau_hook_count).
extern "C" int vgx_test_tau_prevalence(vgx_tau_prevalence_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_prevalence: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->values || !io->final || !io->outside || !io->start) return fail_("null argument");
    const int64_t T = io->T, P = io->popNum, H = io->hapNum, V = io->V;
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail_("bad dimensions");
    std::string why = check_request(io->grid, T, V, io->variant_of, P, H);
    if (!why.empty()) return fail_(why);
    const int64_t cells = P * V;
    TauHookChain c;
    why = tau_hook_split(io, VGX_PREV_TILE_DEFAULT, T * cells, c);
    if (!why.empty()) return fail_(why);
    std::vector<int32_t> pbound, obound;
    tau_hook_marks<VgxPrevCutter, 1>(c, io->ev_times, io->grid, T, pbound, obound);
    std::vector<int64_t> hist((size_t)cells, 0);
    int64_t *const dst[3] = {io->values, io->final, io->outside};
    const int64_t len[3] = {T * cells, cells, 2};
    tau_hook_count(c, pbound.data(), obound.data(), dst, len, [&](const int64_t *rows, const int32_t *bound, int32_t t0, int32_t t1, int64_t *const *b) {
        vgx_tau_prev_tile_host(rows, bound, (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, t0, t1, hist.data(), b[0], b[1], b[2]);
    });
    for (int64_t i = 0; i < cells; i++) vgx_tau_prev_scan_column(io->values + i, io->final + i, io->start[i], (int32_t)T, cells);
    return VGX_OK;
}
