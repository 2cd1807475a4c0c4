// vgx_tau_milestones.hip — peaks, first passages and last positive events per population (and all populations together) and
// variant class of every selected replicate of a TAU ensemble, on the device (vgx_get_tau_milestones), the host side of that
// call, and the same rule, tile walk and merge compiled for the host (vgx_test_tau_milestones).  The rule is
// vgx_tau_milestones.h; DESIGN.md §22.
//
// A tau event is a step of many weighted rows that apply together, and values move by num: the ballots of vgx_milestones.hip do
// not apply.  Pass A (vgx_tau_prevalence.hip's int64 counting and scan kernels with the tile edges in row space as bounds) gives
// every tile of whole events its base.  The WALK kernel takes one workgroup per (chain, tile): the events of the tile run in
// order; for each, the threads stride over its rows (three 16-byte loads per row, consecutive threads consecutive rows), add the
// signed num to the per-cell net change in LDS with 64-bit LDS atomics and put a cell on a touched list the first time it is
// hit; behind a barrier they stride over the touched population cells, settle each (vgx_tau_ms_settle), clear its net change and
// pass it on to the cell of row P; behind another barrier the touched cells of row P are settled.  Row P's net change is formed
// from the touched cells, not from every row: otherwise all rows of a step would add to the same V addresses.  At the tile's end
// event indices go to the chain's block with 32-bit atomic extrema and the tile's peak to a slot of its own; the REDUCE kernel
// takes the slots in tile order.  The prefix is walked once per call as a chain of its own.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_tau_milestones.h"
#include "vgx_tau_replay.h"   // the frame: selection, workspace, timed sections, the hook's chain split

namespace {

__device__ __forceinline__ void lds_add64(int64_t *p, int64_t v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);   // two's complement: the sum is the signed one
}

// put `cell` on the list that starts at list[at] unless it is there (count: the list's length)
__device__ __forceinline__ void note(const VgxTauMsRecords &rec, int32_t cell, int32_t at, int which) {
    if (atomicExch(&rec.mark[cell], 1) == 0) rec.list[at + atomicAdd(&rec.count[which], 1)] = cell;
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) vgxtm_walk_kernel(VgxTauMsLaunch g) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const VgxTauPrevLaunch &a = g.a;
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int32_t nt = g.n_tiles[row], P = a.P, V = a.V, pv = P * V, cells = pv + V, K = g.K, T = a.T;
    if ((int32_t)blockIdx.y >= nt) return;                 // (the whole workgroup: the chain ends before its first tile)
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *rows = (const longlong2 *)(a.rows + (a.rep ? a.rep[row] * a.stride * 6 : 0));
    const int32_t *ev_row = g.ev_row + g.ev_off[row], *tile_ev = g.tile_ev + row * (int64_t)(T + 1);
    const int32_t ev0 = g.ev0[row];
    const VgxTauMsRecords rec = vgx_tau_ms_records(lds, cells, K);
    int32_t *blast = g.last_pos + row * cells, *bfirst = g.first + row * (int64_t)K * cells;
    for (int32_t t = (int32_t)blockIdx.y; t < nt; t += (int32_t)gridDim.y) {
        for (int32_t i = tid; i < cells; i += THREADS) {
            int64_t v = 0;
            if (i < pv) v = vgx_tau_ms_base(a.start, a.val, row, T, pv, t, i);
            else for (int32_t p = 0; p < P; p++) v = vgx_tau_prev_add(v, vgx_tau_ms_base(a.start, a.val, row, T, pv, t, p * V + (i - pv)));
            vgx_tau_ms_record_init(rec, i, cells, K, v);
        }
        if (tid == 0) rec.count[0] = rec.count[1] = 0;
        __syncthreads();
        const int32_t e1 = tile_ev[t + 1];
        int32_t r1 = ev_row[tile_ev[t]];                    // (uniform addresses: every thread reads the same entries)
        for (int32_t e = tile_ev[t]; e < e1; e++) {
            const int32_t r0 = r1;
            r1 = ev_row[e + 1];
            if (r1 <= r0) continue;                         // (the whole workgroup: an event without rows changes nothing)
            // (i) the rows of the event into the net changes of their cells
            for (int64_t r = (int64_t)r0 + tid; r < r1; r += THREADS) {
                const longlong2 q0 = rows[r * 3], q1 = rows[r * 3 + 1], q2 = rows[r * 3 + 2];
                int32_t cell[2], sign[2];
                int k;
                const int64_t w = vgx_tau_prev_row(q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, P, a.hapNum, V, a.variant_of, cell, sign, k);
                if (k > 0) { lds_add64(&rec.delta[cell[0]], sign[0] < 0 ? -w : w); note(rec, cell[0], 0, 0); }
                if (k > 1) { lds_add64(&rec.delta[cell[1]], sign[1] < 0 ? -w : w); note(rec, cell[1], 0, 0); }
            }
            __syncthreads();
            // (ii) the touched population cells, one per thread; their net changes on to row P
            const int32_t n0 = rec.count[0], ev = ev0 + e;
            for (int32_t i = tid; i < n0; i += THREADS) {
                const int32_t cell = rec.list[i];
                const int64_t d = rec.delta[cell];
                rec.delta[cell] = 0;
                rec.mark[cell] = 0;
                if (d) {
                    vgx_tau_ms_settle(rec, cell, cells, d, ev, g.theta, K);
                    const int32_t all = pv + cell % V;
                    lds_add64(&rec.delta[all], d);
                    note(rec, all, pv, 1);
                }
            }
            __syncthreads();
            const int32_t n1 = rec.count[1];
            if (tid == 0) rec.count[0] = 0;                 // (every thread has read it before the barrier above)
            for (int32_t i = tid; i < n1; i += THREADS) {
                const int32_t cell = rec.list[pv + i];
                const int64_t d = rec.delta[cell];
                rec.delta[cell] = 0;
                rec.mark[cell] = 0;
                vgx_tau_ms_settle(rec, cell, cells, d, ev, g.theta, K);
            }
            __syncthreads();
            if (tid == 0) rec.count[1] = 0;                 // (read before the barrier above, added to behind the next one)
        }
        // the tile's records: event indices into the block, the peak into the tile's slot
        int64_t *speak = g.slot_peak + (row * T + t) * cells;
        int32_t *sevent = g.slot_event + (row * T + t) * cells;
        for (int32_t i = tid; i < cells; i += THREADS) {
            speak[i] = rec.peak[i];
            sevent[i] = rec.peak_event[i];
            if (rec.last_pos[i] != VGX_MS_NONE) atomicMax(&blast[i], rec.last_pos[i]);
            for (int32_t k = 0; k < K; k++) {
                const int32_t fe = rec.first[(int64_t)k * cells + i];
                if (fe != VGX_MS_NEVER) atomicMin(&bfirst[(int64_t)k * cells + i], fe);
            }
        }
        __syncthreads();
    }
}

// one thread per (chain, cell): the peaks of the chain's tiles offered to the block's in tile order
__global__ void __launch_bounds__(256) vgxtm_reduce_kernel(VgxTauMsLaunch g) {
    const int64_t cells = ((int64_t)g.a.P + 1) * g.a.V, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.a.m * cells) return;
    const int64_t row = idx / cells, cell = idx % cells;
    int64_t peak = g.peak[idx];
    int32_t peak_event = g.peak_event[idx];
    const int32_t nt = g.n_tiles[row];
    for (int32_t t = 0; t < nt; t++) {
        const int64_t at = (row * g.a.T + t) * cells + cell;
        vgx_tau_ms_offer_peak(peak, peak_event, g.slot_peak[at], g.slot_event[at]);
    }
    g.peak[idx] = peak;
    g.peak_event[idx] = peak_event;
}

template <int THREADS>
hipError_t launch_walk_shape(const VgxTauMsLaunch *g, unsigned tiles, int64_t lds, hipStream_t s) {
    hipError_t err = hipFuncSetAttribute((const void *)vgxtm_walk_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtm_walk_kernel<THREADS>, dim3((unsigned)g->a.m, tiles), dim3(THREADS), (size_t)lds, s, *g);
    return hipGetLastError();
}

// the walk of every (chain, tile) and the reduction of the peaks.  waves: wavefronts of a workgroup, 1 or 4
hipError_t launch_walk(const VgxTauMsLaunch *g, int waves, hipStream_t s) {
    const VgxTauPrevLaunch &a = g->a;
    if (a.m <= 0 || g->max_tiles <= 0) return hipSuccess;
    const int64_t lds = vgx_tau_ms_lds_bytes(a.P, a.V, g->K);
    if (lds > VGX_MS_LDS_MAX || g->K < 0 || g->K > VGX_MS_MAX_K || g->max_tiles > a.T || (waves != 1 && waves != 4)) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)(g->max_tiles < 65535 ? g->max_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = waves == 1 ? launch_walk_shape<64>(g, tiles, lds, s) : launch_walk_shape<256>(g, tiles, lds, s);
    if (err != hipSuccess) return err;
    const int64_t cols = a.m * ((int64_t)a.P + 1) * a.V;
    hipLaunchKernelGGL(vgxtm_reduce_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, *g);
    return hipGetLastError();
}

// what both the call and the hook check about the map, the thresholds and the dimensions; "" or why not
std::string check_request(int64_t V, const int32_t *variant_of, int64_t K, const int64_t *thresholds, int64_t P, int64_t H) {
    if (V < 1 || V > INT32_MAX || !variant_of) return "V = " + std::to_string(V) + " classes: at least 1, with variant_of";
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")";
    if (K < 0 || K > VGX_MS_MAX_K || (K > 0 && !thresholds)) return "K = " + std::to_string(K) + " thresholds: at most 16, with thresholds";
    if (vgx_tau_ms_lds_bytes(P, V, K) > VGX_MS_LDS_MAX)
        return std::to_string(P) + " populations (and their total) x " + std::to_string(V) + " classes x " + std::to_string(K) + " thresholds need " +
               std::to_string(vgx_tau_ms_lds_bytes(P, V, K)) + " bytes of records, above the " + std::to_string((int64_t)VGX_MS_LDS_MAX) +
               " bytes of LDS a walking workgroup may use";
    return "";
}

// The tables of m chains of one launch: tile edges in events and in rows (pass A's bounds), the first row of every event
struct ChainTables {
    int64_t T = 1, max_tiles = 0;          // T: allocation stride in tiles (at least 1)
    std::vector<int32_t> ev_row, tile_ev, bound, n_tiles;
    std::vector<int64_t> ev_off;
};
// edges[j]: the tile edges of chain j in events (vgx_tau_ms_tiles); row_of(j, e): first row of its event e (e = events: its rows)
template <class RowOf>
void fill_tables(ChainTables &ct, int64_t m, const std::vector<int32_t> *const *edges, const int64_t *n_ev, RowOf row_of) {
    ct.T = 1; ct.max_tiles = 0;
    int64_t total = 0;
    for (int64_t j = 0; j < m; j++) {
        const int64_t nt = (int64_t)edges[j]->size() - 1;
        ct.max_tiles = std::max(ct.max_tiles, nt);
        total += n_ev[j] + 1;
    }
    ct.T = std::max<int64_t>(ct.max_tiles, 1);
    const int64_t T = ct.T;
    ct.ev_row.resize((size_t)total);
    ct.ev_off.resize((size_t)m);
    ct.n_tiles.resize((size_t)m);
    ct.tile_ev.resize((size_t)(m * (T + 1)));
    ct.bound.resize((size_t)(m * (T + 2)));
    int64_t off = 0;
    for (int64_t j = 0; j < m; j++) {
        const std::vector<int32_t> &ed = *edges[j];
        const int64_t nt = (int64_t)ed.size() - 1;
        ct.ev_off[(size_t)j] = off;
        ct.n_tiles[(size_t)j] = (int32_t)nt;
        for (int64_t k = 0; k <= n_ev[j]; k++) ct.ev_row[(size_t)(off + k)] = (int32_t)row_of(j, k);
        off += n_ev[j] + 1;
        for (int64_t k = 0; k <= T; k++) ct.tile_ev[(size_t)(j * (T + 1) + k)] = ed[(size_t)std::min(k, nt)];
        for (int64_t k = 0; k <= T + 1; k++) ct.bound[(size_t)(j * (T + 2) + k)] = (int32_t)row_of(j, ed[(size_t)std::min(k, nt)]);
    }
}

// host blocks of n chains
struct HostBlocks {
    int64_t cells, K;
    std::vector<int64_t> peak;
    std::vector<int32_t> peak_event, last_pos, first;
    HostBlocks(int64_t n, int64_t cells_, int64_t K_) : cells(cells_), K(K_), peak((size_t)(n * cells_)), peak_event((size_t)(n * cells_)),
                                                         last_pos((size_t)(n * cells_)), first((size_t)(n * std::max<int64_t>(K_, 1) * cells_)) {}
    VgxTauMsBlock at(int64_t i) { return VgxTauMsBlock{peak.data() + i * cells, peak_event.data() + i * cells, last_pos.data() + i * cells, first.data() + i * K * cells}; }
    // the block of chain i from the start of its population rows (pv values)
    void init(int64_t i, const int64_t *start, int64_t P, int64_t V, const int64_t *theta) {
        const VgxTauMsBlock b = at(i);
        for (int64_t c = 0; c < cells; c++) {
            int64_t v = 0;
            if (c < P * V) v = start[c];
            else for (int64_t p = 0; p < P; p++) v = vgx_tau_prev_add(v, start[p * V + (c - P * V)]);
            vgx_tau_ms_init_cell(b, (int32_t)c, (int32_t)cells, v, theta, (int32_t)K);
        }
    }
    void copy(int64_t i, HostBlocks &src, int64_t j) {
        std::copy_n(src.peak.data() + j * cells, cells, peak.data() + i * cells);
        std::copy_n(src.peak_event.data() + j * cells, cells, peak_event.data() + i * cells);
        std::copy_n(src.last_pos.data() + j * cells, cells, last_pos.data() + i * cells);
        std::copy_n(src.first.data() + j * K * cells, K * cells, first.data() + i * K * cells);
    }
};

}  // namespace

extern "C" int vgx_get_tau_milestones(vgx_engine *e, vgx_tau_milestones_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && !io->replicates)) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_milestones: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, V = io->V, K = io->K, mev_cap = e->tau_mev_cap;
    TauSel sel;
    if (const int rc = tau_select(e, me, "walks", [&]() { return check_request(V, io->variant_of, K, io->thresholds, P, H); }, n, io->replicates, prefix, false,
                                  [&](int64_t, int64_t r, bool with) -> std::string {
                                      const int64_t events = (with ? sel.pre_ev : 0) + (int64_t)e->tau_log[(size_t)r].size();
                                      if (events < VGX_MS_MAX_EVENTS) return "";
                                      return "replicate " + std::to_string(r) + " holds a chain of " + std::to_string(events) + " events (2^30 or more)";
                                  }, sel))
        return rc;
    const FlatChain &pre = sel.pre;
    const std::vector<int32_t> &n_own = sel.n_own, &with_prefix = sel.with_prefix;
    const bool any_prefix = sel.any_prefix;
    const int64_t pv = P * V, cells = pv + V, pre_ev = sel.pre_ev, pre_rows = sel.pre_rows;
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    int64_t tile = VGX_TAU_MS_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_TAU_MILESTONES_TILE_ROWS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), (int64_t)1 << 30);
    const char *wv = getenv("VGX_TAU_MILESTONES_WAVES");      // diagnostic: the other workgroup shape
    const int waves = wv && atoi(wv) == 4 ? 4 : 1;
    // host: the tiles of every chain
    const auto t_tables = std::chrono::steady_clock::now();
    std::vector<int32_t> pre_edges;
    if (any_prefix) vgx_tau_ms_tiles([&](int64_t k) { return pre.ev_row[(size_t)k]; }, pre_ev, tile, pre_edges);
    std::vector<std::vector<int32_t>> edges((size_t)n);
    std::vector<int64_t> steps((size_t)n);
    for_parts(n, [&](int64_t j0, int64_t j1, unsigned) {
        for (int64_t i = j0; i < j1; i++) {
            const auto &lg = e->tau_log[(size_t)io->replicates[i]];
            const int64_t ns = (int64_t)lg.size();
            steps[(size_t)i] = ns;
            vgx_tau_ms_tiles([&](int64_t k) { return k < ns ? lg[(size_t)k].m0 : (int64_t)n_own[(size_t)i]; }, ns, tile, edges[(size_t)i]);
        }
    }, 1 << 12);
    io->ms[1] += since(t_tables);

    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    // what stays for the whole call: [rep | n_own | ev0 | variant_of | prefix rows | start | peak | peak_event | last_pos | first]
    DevLayout lay;
    const int64_t o_rep = lay.take(n * 8), o_nown = lay.take(n * 4), o_ev0 = lay.take(n * 4), o_map = lay.take(H * 4), o_prow = lay.take(pre_rows * 48 + 8),
                  o_start = lay.take(n * pv * 8), o_peak = lay.take(n * cells * 8), o_pev = lay.take(n * cells * 4), o_last = lay.take(n * cells * 4),
                  o_first = lay.take(n * K * cells * 4), keep_total = lay.total + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(P + 1) + " x " + std::to_string(V) + " records of " +
                                        std::to_string(K) + " thresholds, the prefix rows and the start take " + std::to_string(keep_total) +
                                        " bytes, above half of the " + std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    const int64_t share = tau_chunk_share((int64_t)(free_b / 2) - keep_total + 4096);
    // device bytes of m chains of at most T tiles with `events` events in all: the first row of every event, pass A's bounds, the
    // tile edges, the tile bases (val, fin), the peak slots
    const int64_t tile_bytes = pv * 8 + cells * 12 + 8;
    auto chunk_bytes = [&](int64_t m, int64_t T, int64_t events) { return (events + m) * 4 + m * (T * tile_bytes + pv * 8 + 64) + 2048; };
    for (int64_t i = 0; i < n; i++) {
        const int64_t tiles = std::max<int64_t>((int64_t)edges[(size_t)i].size() - 1, 1), need = chunk_bytes(1, tiles, steps[(size_t)i]);
        if (need > share)
            return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(io->replicates[i]) + ": the bases and peak slots of its " + std::to_string(tiles) +
                                            " tiles of " + std::to_string(tile) + " rows (" + std::to_string(tiles * tile_bytes) + " bytes) and its event table take " +
                                            std::to_string(need) + " bytes, above the " + std::to_string(share) +
                                            " bytes of device memory the call may use: raise VGX_TAU_MILESTONES_TILE_ROWS");
    }
    DevHold khold;
    if (const int rc = dev_alloc(e, me, keep_total, khold)) return rc;
    char *const kws = khold.get();
    const int32_t *d_map = (const int32_t *)(kws + o_map);
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));

    // One launch sequence over m chains: tables up, pass A (count, scan), walk, reduce; the blocks and the final rows come back.
    // blocks / fin: host arrays of the m chains; d_*: where their device copies lie.
    auto run = [&](int64_t m, const ChainTables &ct, const int64_t *d_rows, int64_t stride, const int64_t *d_rep, const int32_t *d_nrows, int64_t max_rows,
                   const int32_t *d_ev0, const int64_t *d_start, char *d_peak, char *d_pev, char *d_last, char *d_first, HostBlocks &blocks, int64_t b0,
                   int64_t *fin) -> int {
        const int64_t T = ct.T;
        DevLayout cl;
        const int64_t c_evrow = cl.take((int64_t)ct.ev_row.size() * 4), c_evoff = cl.take(m * 8), c_tev = cl.take(m * (T + 1) * 4), c_nt = cl.take(m * 4),
                      c_bnd = cl.take(m * (T + 2) * 4), c_val = cl.take(m * T * pv * 8), c_fin = cl.take(m * pv * 8), c_out = cl.take(m * 16),
                      c_speak = cl.take(m * T * cells * 8), c_sev = cl.take(m * T * cells * 4);
        DevHold chold;
        if (const int rc = dev_alloc(e, me, cl.total, chold)) return rc;
        char *const cws = chold.get();
        HIPCHECK(e, hipMemcpyAsync(cws + c_evrow, ct.ev_row.data(), ct.ev_row.size() * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_evoff, ct.ev_off.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_tev, ct.tile_ev.data(), ct.tile_ev.size() * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_nt, ct.n_tiles.data(), (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + c_bnd, ct.bound.data(), ct.bound.size() * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemsetAsync(cws + c_val, 0, (size_t)(c_speak - c_val), e->stream));   // val, fin and pass A's outside counters
        VgxTauMsLaunch g{};
        VgxTauPrevLaunch &a = g.a;
        a.m = m;
        a.rows = d_rows; a.stride = stride; a.rep = d_rep; a.n_rows = d_nrows;
        a.bound = (const int32_t *)(cws + c_bnd);
        a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V; a.variant_of = d_map;
        a.tile = VGX_PREV_TILE_DEFAULT; a.max_n = max_rows;
        a.val = (int64_t *)(cws + c_val); a.fin = (int64_t *)(cws + c_fin); a.outside = (int64_t *)(cws + c_out);
        a.start = d_start;
        g.K = (int32_t)K;
        for (int64_t k = 0; k < K; k++) g.theta[k] = io->thresholds[k];
        g.ev_row = (const int32_t *)(cws + c_evrow); g.ev_off = (const int64_t *)(cws + c_evoff);
        g.tile_ev = (const int32_t *)(cws + c_tev); g.n_tiles = (const int32_t *)(cws + c_nt); g.ev0 = d_ev0;
        g.max_tiles = ct.max_tiles;
        g.peak = (int64_t *)d_peak; g.peak_event = (int32_t *)d_pev; g.last_pos = (int32_t *)d_last; g.first = (int32_t *)d_first;
        g.slot_peak = (int64_t *)(cws + c_speak); g.slot_event = (int32_t *)(cws + c_sev);
        return tau_timed(e, io->ms, me + "counting, scan, walk or reduce kernel failed: ", [&]() -> int {
            HIPCHECK(e, vgxi_tau_prev_count(&a, e->stream));
            HIPCHECK(e, vgxi_tau_prev_scan(&a, e->stream));
            HIPCHECK(e, launch_walk(&g, waves, e->stream));
            if (ct.max_tiles > 0) io->passes += 1;
            return VGX_OK;
        }, [&]() -> int {
            HIPCHECK(e, hipMemcpyAsync(fin, cws + c_fin, (size_t)(m * pv) * 8, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync(blocks.peak.data() + b0 * cells, d_peak, (size_t)(m * cells) * 8, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync(blocks.peak_event.data() + b0 * cells, d_pev, (size_t)(m * cells) * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync(blocks.last_pos.data() + b0 * cells, d_last, (size_t)(m * cells) * 4, hipMemcpyDeviceToHost, e->stream));
            if (K > 0) HIPCHECK(e, hipMemcpyAsync(blocks.first.data() + b0 * K * cells, d_first, (size_t)(m * K * cells) * 4, hipMemcpyDeviceToHost, e->stream));
            return VGX_OK;
        });
    };
    auto up_blocks = [&](HostBlocks &b, int64_t m, char *d_peak, char *d_pev, char *d_last, char *d_first) -> int {
        HIPCHECK(e, hipMemcpyAsync(d_peak, b.peak.data(), (size_t)(m * cells) * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(d_pev, b.peak_event.data(), (size_t)(m * cells) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(d_last, b.last_pos.data(), (size_t)(m * cells) * 4, hipMemcpyHostToDevice, e->stream));
        if (K > 0) HIPCHECK(e, hipMemcpyAsync(d_first, b.first.data(), (size_t)(m * K * cells) * 4, hipMemcpyHostToDevice, e->stream));
        return VGX_OK;
    };

    // the state every chain starts from, folded through variant_of: the initial state for a chain that starts at the beginning of
    // the model's history (a restarted replicate, or one that carries a prefix), else the state the call started from
    const std::vector<int64_t> fold[2] = {tau_fold_state(e->hs.infectious, P, H, V, io->variant_of), tau_fold_state(e->hs.initial_infectious, P, H, V, io->variant_of)};

    // the prefix, once: a chain of its own from the initial state.  Its block and its final row use the places of chain 0, which
    // are written again below.
    HostBlocks pblock(1, cells, K);
    std::vector<int64_t> pfin(fold[1]);
    if (any_prefix) {
        pblock.init(0, fold[1].data(), P, V, io->thresholds);
        const auto t_tab = std::chrono::steady_clock::now();
        ChainTables ct;
        const std::vector<int32_t> *pe = &pre_edges;
        fill_tables(ct, 1, &pe, &pre_ev, [&](int64_t, int64_t k) { return pre.ev_row[(size_t)k]; });
        io->ms[1] += since(t_tab);
        const int32_t pn = (int32_t)pre_rows, zero = 0;
        if (pre_rows > 0) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 48, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_nown, &pn, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_ev0, &zero, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(kws + o_start, fold[1].data(), (size_t)pv * 8, hipMemcpyHostToDevice, e->stream));
        if (const int rc = up_blocks(pblock, 1, kws + o_peak, kws + o_pev, kws + o_last, kws + o_first)) return rc;
        if (const int rc = run(1, ct, (const int64_t *)(kws + o_prow), 0, nullptr, (const int32_t *)(kws + o_nown), pre_rows, (const int32_t *)(kws + o_ev0),
                               (const int64_t *)(kws + o_start), kws + o_peak, kws + o_pev, kws + o_last, kws + o_first, pblock, 0, pfin.data()))
            return rc;
    }

    // every replicate's start, block and first event index: from the prefix's final values and block where it carries the prefix
    HostBlocks blocks(n, cells, K);
    std::vector<int64_t> start((size_t)(n * pv)), reps_all(io->replicates, io->replicates + n);
    std::vector<int32_t> ev0((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (with_prefix[(size_t)i]) {
            std::copy(pfin.begin(), pfin.end(), start.begin() + i * pv);
            blocks.copy(i, pblock, 0);
        } else {
            const std::vector<int64_t> &f = fold[e->sc_host[(size_t)io->replicates[i]].restarts > 0 || pre_ev > 0 ? 1 : 0];
            std::copy(f.begin(), f.end(), start.begin() + i * pv);
            blocks.init(i, f.data(), P, V, io->thresholds);
        }
        ev0[(size_t)i] = with_prefix[(size_t)i] ? (int32_t)pre_ev : 0;
    }
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_ev0, ev0.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)(n * pv) * 8, hipMemcpyHostToDevice, e->stream));
    if (const int rc = up_blocks(blocks, n, kws + o_peak, kws + o_pev, kws + o_last, kws + o_first)) return rc;
    HIPCHECK(e, hipStreamSynchronize(e->stream));

    // chunks of replicates whose tables, bases and slots fit the share
    std::vector<int64_t> fin((size_t)(n * pv));
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0, T = 1, events = 0, max_rows = 0;
        while (i1 < n) {
            const int64_t T2 = std::max<int64_t>(T, (int64_t)edges[(size_t)i1].size() - 1), ev2 = events + steps[(size_t)i1];
            if (i1 > i0 && chunk_bytes(i1 + 1 - i0, T2, ev2) > share) break;
            T = T2; events = ev2;
            max_rows = std::max<int64_t>(max_rows, n_own[(size_t)i1]);
            i1++;
        }
        const int64_t m = i1 - i0;
        const auto t_tab = std::chrono::steady_clock::now();
        ChainTables ct;
        std::vector<const std::vector<int32_t> *> ed((size_t)m);
        for (int64_t j = 0; j < m; j++) ed[(size_t)j] = &edges[(size_t)(i0 + j)];
        fill_tables(ct, m, ed.data(), steps.data() + i0, [&](int64_t j, int64_t k) {
            const auto &lg = e->tau_log[(size_t)io->replicates[i0 + j]];
            return k < (int64_t)lg.size() ? lg[(size_t)k].m0 : (int64_t)n_own[(size_t)(i0 + j)];
        });
        io->ms[1] += since(t_tab);
        if (const int rc = run(m, ct, (const int64_t *)e->t_mev.p, mev_cap, (const int64_t *)(kws + o_rep) + i0, (const int32_t *)(kws + o_nown) + i0, max_rows,
                               (const int32_t *)(kws + o_ev0) + i0, (const int64_t *)(kws + o_start) + i0 * pv, kws + o_peak + i0 * cells * 8,
                               kws + o_pev + i0 * cells * 4, kws + o_last + i0 * cells * 4, kws + o_first + i0 * K * cells * 4, blocks, i0, fin.data() + i0 * pv))
            return rc;
        i0 = i1;
    }
    // host: indices -> results and times
    for (int64_t i = 0; i < n; i++) {
        const int64_t r = io->replicates[i], pn = with_prefix[(size_t)i] ? pre_ev : 0;
        const auto &lg = e->tau_log[(size_t)r];
        auto at = [&](auto *p, int64_t per) { return p ? p + i * per : p; };
        const VgxTauMsOut out{at(io->final, cells), at(io->peak, cells), at(io->peak_event, cells), at(io->last_positive_event, cells),
                              at(io->first_event, K * cells), at(io->peak_time, cells), at(io->extinction_time, cells), at(io->first_time, K * cells)};
        // index -1: a chain that starts at the beginning of the model's history starts at 0.0, else where the call started
        const double t_start = e->sc_host[(size_t)r].restarts > 0 || pre_ev > 0 ? 0.0 : e->hs.currentTime;
        vgx_tau_ms_outputs(blocks.at(i), fin.data() + i * pv, (int32_t)P, (int32_t)V, (int32_t)K, pn + (int64_t)lg.size(),
                           [&](int64_t k) { return k < pn ? prefix->ev_times[k] : lg[(size_t)(k - pn)].time; }, t_start, out);
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- the host instance: the same flattening, tile edges, pass A, walk, merge and outputs on a chain given as arrays (no device,
// no engine).  The last n_own_events events play the replicate's own steps (their rows are taken as they are, as the device reads
// t_mev), everything before them the prefix, which is flattened and walked once as a chain of its own; the own events start from
// its block and its final values, as on the device.
extern "C" int vgx_test_tau_milestones(vgx_tau_milestones_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_milestones: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->start) return fail_("null argument");
    const int64_t n = io->ev_ptr, P = io->popNum, H = io->hapNum, V = io->V, K = io->K;
    if (P < 1 || H < 1 || P >= INT32_MAX || H > INT32_MAX) return fail_("bad dimensions");
    {
        const std::string why = check_request(V, io->variant_of, K, io->thresholds, P, H);
        if (!why.empty()) return fail_(why);
    }
    if (n < 0 || n >= VGX_MS_MAX_EVENTS) return fail_("a chain of " + std::to_string(n) + " events (2^30 or more)");
    TauHookChain c;
    {
        const std::string why = tau_hook_split(io, VGX_TAU_MS_TILE_DEFAULT, 0, c);
        if (!why.empty()) return fail_(why);
    }
    const int64_t tile = c.tile, n_pre_ev = c.n_pre_ev, n_own_ev = c.n_own_ev, pv = P * V, cells = pv + V;
    const FlatChain &pre = c.pre;
    const std::vector<int64_t> &own = c.own, &own_row = c.own_m0;
    const int32_t Pi = (int32_t)P, Hi = (int32_t)H, Vi = (int32_t)V, Ki = (int32_t)K;
    HostBlocks block(1, cells, K);
    const VgxTauMsBlock blk = block.at(0);
    std::vector<char> lds((size_t)vgx_tau_ms_lds_bytes(P, V, K) + 8);
    const VgxTauMsRecords rec = vgx_tau_ms_records((void *)(((uintptr_t)lds.data() + 7) & ~(uintptr_t)7), (int32_t)cells, Ki);
    rec.count[0] = rec.count[1] = 0;
    // one chain: its tiles, pass A over the tile edges as bounds, then every tile from its base, event after event, and the merge
    auto walk = [&](const int64_t *rows, const std::vector<int64_t> &ev_row, int64_t n_ev, int32_t ev0, const int64_t *start, int64_t *fin) {
        std::vector<int32_t> edges;
        vgx_tau_ms_tiles([&](int64_t k) { return ev_row[(size_t)k]; }, n_ev, tile, edges);
        const int64_t nt = (int64_t)edges.size() - 1, T = std::max<int64_t>(nt, 1), n_rows = ev_row[(size_t)n_ev];
        std::vector<int32_t> bound((size_t)(T + 2));
        for (int64_t k = 0; k <= T + 1; k++) bound[(size_t)k] = (int32_t)ev_row[(size_t)edges[(size_t)std::min(k, nt)]];
        std::vector<int64_t> val((size_t)(T * pv), 0), hist((size_t)pv, 0);
        int64_t outside[2] = {0, 0};
        for (int64_t i = 0; i < pv; i++) fin[i] = 0;
        for (int64_t t0 = 0; t0 < n_rows; t0 += VGX_PREV_TILE_DEFAULT)
            vgx_tau_prev_tile_host(rows, bound.data(), (int32_t)T, Pi, Hi, Vi, io->variant_of, (int32_t)t0,
                                   (int32_t)std::min<int64_t>(t0 + VGX_PREV_TILE_DEFAULT, n_rows), hist.data(), val.data(), fin, outside);
        for (int64_t i = 0; i < pv; i++) vgx_tau_prev_scan_column(val.data() + i, fin + i, start[i], (int32_t)T, pv);
        for (int64_t t = 0; t < nt; t++) {
            for (int32_t i = 0; i < cells; i++) {
                int64_t v = 0;
                if (i < pv) v = vgx_tau_ms_base(start, val.data(), 0, (int32_t)T, (int32_t)pv, t, i);
                else for (int32_t p = 0; p < Pi; p++) v = vgx_tau_prev_add(v, vgx_tau_ms_base(start, val.data(), 0, (int32_t)T, (int32_t)pv, t, p * Vi + (i - (int32_t)pv)));
                vgx_tau_ms_record_init(rec, i, (int32_t)cells, Ki, v);
            }
            for (int64_t k = edges[(size_t)t]; k < edges[(size_t)t + 1]; k++)
                if (ev_row[(size_t)k + 1] > ev_row[(size_t)k])
                    vgx_tau_ms_event_host(rec, rows + ev_row[(size_t)k] * 6, ev_row[(size_t)k + 1] - ev_row[(size_t)k], ev0 + (int32_t)k, Pi, Hi, Vi, io->variant_of,
                                          io->thresholds, Ki);
            vgx_tau_ms_merge_host(rec, blk, (int32_t)cells, Ki);
        }
    };
    block.init(0, io->start, P, V, io->thresholds);
    std::vector<int64_t> pfin(io->start, io->start + pv), fin((size_t)pv);
    if (n_pre_ev > 0) walk(pre.rows.data(), pre.ev_row, n_pre_ev, 0, io->start, pfin.data());
    walk(own.data(), own_row, n_own_ev, (int32_t)n_pre_ev, pfin.data(), fin.data());
    const VgxTauMsOut out{io->final, io->peak, io->peak_event, io->last_positive_event, io->first_event, io->peak_time, io->extinction_time, io->first_time};
    vgx_tau_ms_outputs(blk, fin.data(), Pi, Vi, Ki, n, [&](int64_t k) { return io->ev_times[k]; }, io->t_start, out);
    return VGX_OK;
}
