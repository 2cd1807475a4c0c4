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
#include "vgx_engine.h"
#include "vgx_tau_prevalence.h"
#include "vgx_tau_rows.h"   // EventCols, RowCols, FlatChain, flatten

namespace {

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void add64(long long *p, long long v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);   // two's complement: the sum is the signed one
}

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

// the net blocks (tc value cells and `cells` tail cells per chain) and `outside` counters of m chains start from the prefix's
// (with[i] != 0) or from zero
__global__ void __launch_bounds__(256) vgxtp_init_kernel(int64_t m, int64_t tc, int64_t cells, const int32_t *with, const long long *pre_val,
                                                         const long long *pre_fin, const long long *pre_out, long long *val, long long *fin,
                                                         long long *outside) {
    const int64_t stride = (int64_t)gridDim.x * 256, i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = i0; i < m * tc; i += stride) {
        const int64_t c = i / tc;
        val[i] = with[c] ? pre_val[i - c * tc] : 0;
    }
    for (int64_t i = i0; i < m * cells; i += stride) {
        const int64_t c = i / cells;
        fin[i] = with[c] ? pre_fin[i - c * cells] : 0;
    }
    for (int64_t i = i0; i < 2 * m; i += stride) outside[i] = with[i >> 1] ? pre_out[i & 1] : 0;
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

unsigned flat_grid(int64_t total) { return (unsigned)std::min<int64_t>(std::max<int64_t>((total + 255) / 256, 1), 1 << 16); }

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

// The prefix as a chain of its own: its bounds (0, the cuts the literal loop consumes over its events, then its row count) and
// where the loop stands after it.  bound: [T + 2].
int64_t prefix_bounds(const FlatChain &f, int64_t n_ev, const double *times, const double *grid, int64_t T, int32_t *bound) {
    VgxPrevCutter ct{grid, T, bound};
    for (int64_t i = 0; i < n_ev; i++) ct.event(f.ev_row[(size_t)i], times[i]);
    const int64_t point0 = ct.point;
    ct.finish(f.ev_row[(size_t)n_ev]);
    return point0;
}

// A chain's own events after a prefix that left the loop at point0: bounds relative to the chain's first own row
template <class OwnTime, class OwnRow>
void own_bounds(const double *grid, int64_t T, int64_t point0, int64_t n_own, OwnTime own_time, OwnRow own_m0, int64_t n_rows, int32_t *bound) {
    for (int64_t k = 1; k <= point0; k++) bound[k] = 0;   // these cuts lie inside the prefix: before the first own row
    VgxPrevCutter ct{grid, T, bound};
    ct.point = point0;
    for (int64_t k = 0; k < n_own; k++) ct.event(own_m0(k), own_time(k));
    ct.finish(n_rows);
}

// a state [P][H] folded through variant_of: [P][V]
std::vector<int64_t> fold_state(const std::vector<int64_t> &src, int64_t P, int64_t H, int64_t V, const int32_t *variant_of) {
    std::vector<int64_t> out((size_t)(P * V), 0);
    for (int64_t pn = 0; pn < P; pn++)
        for (int64_t h = 0; h < H; h++)
            if (variant_of[h] >= 0) out[(size_t)(pn * V + variant_of[h])] += src[(size_t)(pn * H + h)];
    return out;
}

}  // namespace

// the init, scan and min/max launches as vgx_tau_susceptible.hip shares them (declared in vgx_engine.h)
extern "C" hipError_t vgxi_tau_prev_init(int64_t m, int64_t tc, int64_t cells, const int32_t *with, const int64_t *pre_val, const int64_t *pre_fin,
                                         const int64_t *pre_out, int64_t *val, int64_t *fin, int64_t *outside, hipStream_t s) {
    hipLaunchKernelGGL(vgxtp_init_kernel, dim3(flat_grid(m * tc)), dim3(256), 0, s, m, tc, cells, with, (const long long *)pre_val,
                       (const long long *)pre_fin, (const long long *)pre_out, (long long *)val, (long long *)fin, (long long *)outside);
    return hipGetLastError();
}

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
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (counts tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V, mev_cap = e->tau_mev_cap;
    {
        const std::string why = check_request(io->grid, T, V, io->variant_of, P, H);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + why);
    }
    const int64_t cells = P * V, tc = T * cells;
    // the prefix: what the model held when the call started
    const int64_t pre_ev = prefix ? prefix->ev_ptr : 0;
    if (pre_ev < 0 || (pre_ev > 0 && (!prefix->ev_times || !prefix->ev_types || !prefix->ev_haplotypes || !prefix->ev_populations ||
                                      !prefix->ev_newHaplotypes || !prefix->ev_newPopulations)))
        return fail(e, VGX_ERR_ARG, me + "null prefix column");
    std::vector<int32_t> n_own((size_t)n), with_prefix((size_t)n, 0);
    bool any_prefix = false;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : e->ev_ptr0;   // vgx_counters.ev_first_new
            if (s.restarts == 0 && first != pre_ev)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain continues a log of " + std::to_string(first) +
                                                " events, the prefix holds " + std::to_string(pre_ev));
            with_prefix[(size_t)i] = s.restarts == 0 && pre_ev > 0;
            any_prefix = any_prefix || with_prefix[(size_t)i];
            const auto &lg = e->tau_log[(size_t)r];
            for (size_t k = 0; k < lg.size(); k++)   // the steps' row ranges tile the replicate's block
                if (lg[k].m0 != (k ? lg[k - 1].m1 : 0) || lg[k].m1 < lg[k].m0)
                    return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": row ranges of its steps are not contiguous");
            if (!lg.empty() && lg.back().m1 > mev_cap) return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " logged more rows than its block holds");
        }
    }
    FlatChain pre;
    pre.ev_row.assign(1, 0);
    if (any_prefix) {
        const EventCols ev{pre_ev, prefix->ev_times, prefix->ev_types, prefix->ev_haplotypes, prefix->ev_populations, prefix->ev_newHaplotypes, prefix->ev_newPopulations};
        const RowCols mv{prefix->mev_rows, prefix->mev_num, prefix->mev_types, prefix->mev_haplotypes, prefix->mev_populations, prefix->mev_newHaplotypes,
                         prefix->mev_newPopulations};
        if (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np)) return fail(e, VGX_ERR_ARG, me + "null prefix multievent column");
        const std::string why = flatten(ev, pre_ev, mv, pre);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + "prefix: " + why);
    }
    const int64_t pre_rows = pre.n_rows();
    for (int64_t i = 0; i < n; i++) {
        const auto &lg = e->tau_log[(size_t)io->replicates[i]];
        const int64_t own = lg.empty() ? 0 : lg.back().m1, total = (with_prefix[(size_t)i] ? pre_rows : 0) + own;
        if (total >= ((int64_t)1 << 31))
            return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(io->replicates[i]) + ": prefix and own rows reach 2^31 (" + std::to_string(total) + ")");
        n_own[(size_t)i] = (int32_t)own;
    }
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    // the state every chain starts from, folded through variant_of: the initial state for a chain that starts at the beginning of
    // the model's history (a restarted replicate, or one that carries a prefix), else the state the call started from
    std::vector<int64_t> start((size_t)(n * cells));
    {
        const std::vector<int64_t> fold[2] = {fold_state(e->hs.infectious, P, H, V, io->variant_of), fold_state(e->hs.initial_infectious, P, H, V, io->variant_of)};
        for (int64_t i = 0; i < n; i++) {
            const std::vector<int64_t> &f = fold[e->sc_host[(size_t)io->replicates[i]].restarts > 0 || pre_ev > 0 ? 1 : 0];
            std::copy(f.begin(), f.end(), start.begin() + i * cells);
        }
    }
    int64_t tile = VGX_PREV_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_PREVALENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call:
    // [rep | n_own | with | variant_of | prefix: rows, bound, n_rows, val, fin, outside | start | val | fin | outside | narrow | min, max]
    const int64_t val_bytes = n * tc * 8, fin_bytes = n * cells * 8, narrow_bytes = io->summary ? n * tc * 4 : 0;
    const int64_t o_rep = 0, o_nown = o_rep + up8(n * 8), o_with = o_nown + up8(n * 4), o_map = o_with + up8(n * 4), o_prow = o_map + up8(H * 4),
                  o_pbnd = o_prow + up8(pre_rows * 48 + 8), o_pn = o_pbnd + up8((T + 2) * 4), o_pval = o_pn + up8(4), o_pfin = o_pval + up8(tc * 8),
                  o_pout = o_pfin + up8(cells * 8), o_start = o_pout + up8(16), o_val = o_start + up8(fin_bytes), o_fin = o_val + up8(val_bytes),
                  o_out = o_fin + up8(fin_bytes), o_nar = o_out + up8(n * 16), o_mm = o_nar + up8(narrow_bytes + 8), keep_total = o_mm + up8(16);
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(V) +
                                        " values of 8 bytes (" + std::to_string(val_bytes + fin_bytes) + " bytes), the prefix rows, the start and " +
                                        (io->summary ? "the summary's 4-byte copy take " : "the bounds take ") + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_with, with_prefix.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)fin_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_pval, 0, (size_t)(o_start - o_pval), e->stream));   // the prefix's net block and its outside counters
    const int32_t *d_map = (const int32_t *)(kws + o_map);

    // the prefix, once: flattened rows uploaded, its bounds, counted as a chain of its own
    int64_t point0 = 0;
    std::vector<int32_t> pbound((size_t)(T + 2), 0);
    const int32_t pn = (int32_t)pre_rows;
    if (any_prefix) {
        const auto t_cuts = std::chrono::steady_clock::now();
        point0 = prefix_bounds(pre, pre_ev, prefix->ev_times, io->grid, T, pbound.data());
        io->ms[1] += since(t_cuts);
        if (pre_rows > 0) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 48, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_pbnd, pbound.data(), (size_t)(T + 2) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_pn, &pn, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        VgxTauPrevLaunch a{};
        a.m = 1;
        a.rows = (const int64_t *)(kws + o_prow); a.stride = 0; a.rep = nullptr;
        a.n_rows = (const int32_t *)(kws + o_pn); a.bound = (const int32_t *)(kws + o_pbnd);
        a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V; a.variant_of = d_map;
        a.tile = (int32_t)tile; a.max_n = pre_rows;
        a.val = (int64_t *)(kws + o_pval); a.fin = (int64_t *)(kws + o_pfin); a.outside = (int64_t *)(kws + o_pout);
        HIPCHECK(e, launch_count(&a, e->stream));
        if (pre_rows > 0) io->passes += 1;
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting kernel failed on the prefix: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
    }

    // chunks of replicates: the bounds of a chunk fit `share` bytes of device memory
    int64_t share = std::min<int64_t>((int64_t)(free_b / 2) - keep_total + 4096, (int64_t)1 << 30);
    if (const char *cb = getenv("VGX_TIMELINES_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    const int64_t per_rep = (T + 2) * 4 + 64;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(share / per_rep, (int64_t)1 << 20));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t i1 = std::min(n, i0 + chunk), m = i1 - i0;
        char *ws = nullptr;
        const int64_t total = up8(m * (T + 2) * 4);
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, dev_free);
        // host: every replicate's bounds in the row index space of its own block (the loop continued where the prefix left it)
        const auto t_cuts = std::chrono::steady_clock::now();
        std::vector<int32_t> bounds((size_t)(m * (T + 2)));
        int64_t steps_all = 0, max_n = 0;
        for (int64_t j = 0; j < m; j++) {
            steps_all += (int64_t)e->tau_log[(size_t)io->replicates[i0 + j]].size();
            max_n = std::max<int64_t>(max_n, n_own[(size_t)(i0 + j)]);
        }
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j;
                const auto &lg = e->tau_log[(size_t)io->replicates[gi]];
                own_bounds(io->grid, T, with_prefix[(size_t)gi] ? point0 : 0, (int64_t)lg.size(), [&](int64_t k) { return lg[(size_t)k].time; },
                           [&](int64_t k) { return lg[(size_t)k].m0; }, n_own[(size_t)gi], bounds.data() + j * (T + 2));
            }
        }, std::max<int64_t>(steps_all / std::max<int64_t>(m, 1), 1) + T);
        io->ms[1] += since(t_cuts);
        HIPCHECK(e, hipMemcpyAsync(ws, bounds.data(), (size_t)(m * (T + 2)) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        VgxTauPrevLaunch a{};
        a.m = m;
        a.rows = (const int64_t *)e->t_mev.p; a.stride = mev_cap;
        a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_rows = (const int32_t *)(kws + o_nown) + i0;
        a.bound = (const int32_t *)ws;
        a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V; a.variant_of = d_map;
        a.tile = (int32_t)tile; a.max_n = max_n;
        a.val = (int64_t *)(kws + o_val) + i0 * tc; a.fin = (int64_t *)(kws + o_fin) + i0 * cells; a.outside = (int64_t *)(kws + o_out) + 2 * i0;
        a.start = (const int64_t *)(kws + o_start) + i0 * cells;
        hipLaunchKernelGGL(vgxtp_init_kernel, dim3(flat_grid(m * tc)), dim3(256), 0, e->stream, m, tc, cells, (const int32_t *)(kws + o_with) + i0,
                           (const long long *)(kws + o_pval), (const long long *)(kws + o_pfin), (const long long *)(kws + o_pout), (long long *)a.val,
                           (long long *)a.fin, (long long *)a.outside);
        HIPCHECK(e, hipGetLastError());
        HIPCHECK(e, launch_count(&a, e->stream));
        if (max_n > 0) io->passes += 1;
        HIPCHECK(e, launch_scan(&a, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting or scan kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
    }
    HIPCHECK(e, hipMemcpy(io->outside, kws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (io->final) HIPCHECK(e, hipMemcpy(io->final, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        // the column summary sorts 32-bit keys of whole numbers in [0, 2^31): narrow the block, and find its extremes on the way
        const uint64_t init[2] = {~(uint64_t)0, 0};
        uint64_t mm[2] = {0, 0};
        HIPCHECK(e, hipMemcpyAsync(kws + o_mm, init, sizeof init, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        hipLaunchKernelGGL(vgxtp_minmax_kernel, dim3(flat_grid(n * tc)), dim3(256), 0, e->stream, n * tc, (const long long *)(kws + o_val),
                           (int32_t *)(kws + o_nar), (unsigned long long *)(kws + o_mm));
        HIPCHECK(e, hipGetLastError());
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "min/max kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        const int64_t lo = (int64_t)(mm[0] ^ 0x8000000000000000ull), hi = (int64_t)(mm[1] ^ 0x8000000000000000ull);
        if (lo <= hi && (lo < 0 || hi >= ((int64_t)1 << 31)))
            return fail(e, VGX_ERR_ARG, me + "summary: a value of " + std::to_string(lo < 0 ? lo : hi) +
                                            " is not a whole number in [0, 2^31) (summarise the int64 values on the host)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_tau_prevalence: summary", (const int32_t *)(kws + o_nar), n, tc, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, bounds, cells, tile walk, prefix-plus-own sum and scan on a chain given as arrays (no
// device, no engine).  The last n_own_events events play the replicate's own steps (their rows are taken as they are, as the device
// reads t_mev), everything before them the prefix, which is flattened and counted once as a chain of its own; the chain's net block
// starts from the prefix's, as on the device.
extern "C" int vgx_test_tau_prevalence(vgx_tau_prevalence_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_prevalence: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->values || !io->final || !io->outside || !io->start) return fail_("null argument");
    const int64_t n = io->ev_ptr, T = io->T, P = io->popNum, H = io->hapNum, V = io->V;
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail_("bad dimensions");
    {
        const std::string why = check_request(io->grid, T, V, io->variant_of, P, H);
        if (!why.empty()) return fail_(why);
    }
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail_("chain too long");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail_("null event column");
    if (io->mev_rows < 0 || (io->mev_rows > 0 && (!io->mev_num || !io->mev_types || !io->mev_haplotypes || !io->mev_populations ||
                                                  !io->mev_newHaplotypes || !io->mev_newPopulations)))
        return fail_("null multievent column");
    int64_t tile = io->tile;
    if (tile < 0) return fail_("tile must not be negative");
    if (tile == 0) tile = VGX_PREV_TILE_DEFAULT;
    const int64_t cells = P * V;
    if (T * cells >= ((int64_t)1 << 40)) return fail_("block too large");
    int64_t n_own_ev = io->n_own_events;
    if (n_own_ev < -1 || n_own_ev > n) return fail_("n_own_events must be -1 or lie in [0, ev_ptr]");
    if (n_own_ev < 0) {   // the chain's trailing MULTITYPE events
        n_own_ev = 0;
        while (n_own_ev < n && io->ev_types[n - 1 - n_own_ev] == VGX_TL_MULTITYPE) n_own_ev++;
    }
    const int64_t n_pre_ev = n - n_own_ev;
    const EventCols ev{n, io->ev_times, io->ev_types, io->ev_haplotypes, io->ev_populations, io->ev_newHaplotypes, io->ev_newPopulations};
    const RowCols mv{io->mev_rows, io->mev_num, io->mev_types, io->mev_haplotypes, io->mev_populations, io->mev_newHaplotypes, io->mev_newPopulations};
    FlatChain pre;
    {
        const std::string why = flatten(ev, n_pre_ev, mv, pre);
        if (!why.empty()) return fail_(why);
    }
    // the own rows as a block of their own, unjudged, with every own event's first row
    std::vector<int64_t> own, own_m0((size_t)n_own_ev);
    for (int64_t k = 0; k < n_own_ev; k++) {
        const int64_t i = n_pre_ev + k, t = ev.types[i];
        own_m0[(size_t)k] = (int64_t)own.size() / 6;
        if (t == VGX_TL_MULTITYPE) {
            const int64_t j0 = ev.hap[i], j1 = ev.pop[i];
            if (j1 <= j0) continue;
            if (j0 < 0 || j1 > mv.n) return fail_("event " + std::to_string(i) + ": MULTITYPE row range outside the multievent log");
            for (int64_t j = j0; j < j1; j++) {
                const int64_t v[6] = {mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]};
                own.insert(own.end(), v, v + 6);
            }
        } else {
            const int64_t v[6] = {1, t, ev.hap[i], ev.pop[i], ev.nh[i], ev.np[i]};
            own.insert(own.end(), v, v + 6);
        }
        if (pre.n_rows() + (int64_t)own.size() / 6 >= ((int64_t)1 << 31)) return fail_("the chain has 2^31 rows or more");
    }
    const int64_t pre_rows = pre.n_rows(), own_rows = (int64_t)own.size() / 6;
    std::vector<int32_t> pbound((size_t)(T + 2)), obound((size_t)(T + 2));
    const int64_t point0 = prefix_bounds(pre, n_pre_ev, io->ev_times, io->grid, T, pbound.data());
    own_bounds(io->grid, T, point0, n_own_ev, [&](int64_t k) { return io->ev_times[n_pre_ev + k]; }, [&](int64_t k) { return own_m0[(size_t)k]; }, own_rows,
               obound.data());
    // the prefix's net block, counted once ...
    std::vector<int64_t> pval((size_t)(T * cells), 0), pfin((size_t)cells, 0), hist((size_t)cells, 0);
    int64_t pout[2] = {0, 0};
    for (int64_t t0 = 0; t0 < pre_rows; t0 += tile)
        vgx_tau_prev_tile_host(pre.rows.data(), pbound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, (int32_t)t0,
                               (int32_t)std::min<int64_t>(t0 + tile, pre_rows), hist.data(), pval.data(), pfin.data(), pout);
    // ... is what the chain's net block starts from; its own rows are added on top, and the columns are summed up
    for (int64_t i = 0; i < T * cells; i++) io->values[i] = pval[(size_t)i];
    for (int64_t i = 0; i < cells; i++) io->final[i] = pfin[(size_t)i];
    io->outside[0] = pout[0];
    io->outside[1] = pout[1];
    for (int64_t t0 = 0; t0 < own_rows; t0 += tile)
        vgx_tau_prev_tile_host(own.data(), obound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, (int32_t)t0,
                               (int32_t)std::min<int64_t>(t0 + tile, own_rows), hist.data(), io->values, io->final, io->outside);
    for (int64_t i = 0; i < cells; i++) vgx_tau_prev_scan_column(io->values + i, io->final + i, io->start[i], (int32_t)T, cells);
    return VGX_OK;
}
