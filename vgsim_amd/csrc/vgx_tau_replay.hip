// vgx_tau_replay.hip — what the frame of the tau replays (vgx_tau_replay.h) compiles once: the chain split of
// the CPU test hooks, the workspace allocation, the chunk share, the summary tail, and the init kernel that starts the blocks of a
// chunk's chains from the prefix's.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "vgx_tau_replay.h"

namespace {

__global__ void __launch_bounds__(256) vgxtr_init_kernel(int64_t m, int64_t tc, int64_t cells, const int32_t *with, const long long *pre_val,
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

}  // namespace

extern "C" hipError_t vgxi_tau_block_init(int64_t m, int64_t tc, int64_t cells, const int32_t *with, const int64_t *pre_val, const int64_t *pre_fin,
                                          const int64_t *pre_out, int64_t *val, int64_t *fin, int64_t *outside, hipStream_t s) {
    hipLaunchKernelGGL(vgxtr_init_kernel, dim3(flat_grid(m * tc)), dim3(256), 0, s, m, tc, cells, with, (const long long *)pre_val,
                       (const long long *)pre_fin, (const long long *)pre_out, (long long *)val, (long long *)fin, (long long *)outside);
    return hipGetLastError();
}

std::string tau_hook_split(const EventCols &ev, const RowCols &mv, int64_t tile, int64_t tile_default, int64_t block, int64_t n_own_events, TauHookChain &c) {
    const int64_t n = ev.n;
    if (n < 0 || n >= ((int64_t)1 << 31)) return "chain too long";
    if (n > 0 && (!ev.times || !ev.types || !ev.hap || !ev.pop || !ev.nh || !ev.np)) return "null event column";
    if (mv.n < 0 || (mv.n > 0 && (!mv.num || !mv.types || !mv.hap || !mv.pop || !mv.nh || !mv.np))) return "null multievent column";
    if (tile < 0) return "tile must not be negative";
    c.tile = tile == 0 ? tile_default : tile;
    if (block >= ((int64_t)1 << 40)) return "block too large";
    int64_t n_own_ev = n_own_events;
    if (n_own_ev < -1 || n_own_ev > n) return "n_own_events must be -1 or lie in [0, ev_ptr]";
    if (n_own_ev < 0) {   // the chain's trailing MULTITYPE events
        n_own_ev = 0;
        while (n_own_ev < n && ev.types[n - 1 - n_own_ev] == VGX_TL_MULTITYPE) n_own_ev++;
    }
    const int64_t n_pre_ev = n - n_own_ev;
    c.n_pre_ev = n_pre_ev;
    c.n_own_ev = n_own_ev;
    {
        const std::string why = flatten(ev, n_pre_ev, mv, c.pre);
        if (!why.empty()) return why;
    }
    // the own rows as a block of their own, unjudged, with every own event's first row
    std::vector<int64_t> &own = c.own;
    own.clear();
    c.own_m0.assign((size_t)n_own_ev + 1, 0);
    for (int64_t k = 0; k < n_own_ev; k++) {
        const int64_t i = n_pre_ev + k, t = ev.types[i];
        c.own_m0[(size_t)k] = (int64_t)own.size() / 6;
        if (t == VGX_TL_MULTITYPE) {
            const int64_t j0 = ev.hap[i], j1 = ev.pop[i];
            if (j1 <= j0) continue;
            if (j0 < 0 || j1 > mv.n) return "event " + std::to_string(i) + ": MULTITYPE row range outside the multievent log";
            for (int64_t j = j0; j < j1; j++) {
                const int64_t v[6] = {mv.num[j], mv.types[j], mv.hap[j], mv.pop[j], mv.nh[j], mv.np[j]};
                own.insert(own.end(), v, v + 6);
            }
        } else {
            const int64_t v[6] = {1, t, ev.hap[i], ev.pop[i], ev.nh[i], ev.np[i]};
            own.insert(own.end(), v, v + 6);
        }
        if (c.pre.n_rows() + (int64_t)own.size() / 6 >= ((int64_t)1 << 31)) return "the chain has 2^31 rows or more";
    }
    c.own_m0[(size_t)n_own_ev] = (int64_t)own.size() / 6;
    return "";
}

std::vector<int64_t> tau_fold_state(const std::vector<int64_t> &src, int64_t P, int64_t H, int64_t V, const int32_t *variant_of) {
    std::vector<int64_t> out((size_t)(P * V), 0);
    for (int64_t pn = 0; pn < P; pn++)
        for (int64_t h = 0; h < H; h++)
            if (variant_of[h] >= 0) out[(size_t)(pn * V + variant_of[h])] += src[(size_t)(pn * H + h)];
    return out;
}

int dev_alloc(vgx_engine *e, const std::string &me, int64_t bytes, DevHold &hold) {
    char *p = nullptr;
    const hipError_t er = hipMalloc((void **)&p, (size_t)bytes);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(er));
    hold.reset(p);
    return VGX_OK;
}

int64_t tau_chunk_share(int64_t room) {
    int64_t share = std::min<int64_t>(room, (int64_t)1 << 30);
    if (const char *cb = getenv("VGX_TIMELINES_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    return share;
}

int tau_summary(vgx_engine *e, const std::string &me, bool counts, const int64_t *block, int64_t n, int64_t tc, int32_t *narrow, uint64_t *mm,
                vgx_traj_summary_io *summary, double *ms) {
    // the column summary sorts 32-bit keys of whole numbers in [0, 2^31): narrow the block, and find its extremes on the way
    const uint64_t init[2] = {~(uint64_t)0, 0};
    uint64_t h_mm[2] = {0, 0};
    HIPCHECK(e, hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, e->stream));
    const int rc = tau_timed(e, ms, me + (counts ? "narrowing kernel failed: " : "min/max kernel failed: "),
                             [&]() -> int { HIPCHECK(e, vgxi_tau_prev_minmax(n * tc, block, narrow, mm, e->stream)); return VGX_OK; },
                             [&]() -> int { HIPCHECK(e, hipMemcpyAsync(h_mm, mm, sizeof h_mm, hipMemcpyDeviceToHost, e->stream)); return VGX_OK; });
    if (rc) return rc;
    const int64_t lo = (int64_t)(h_mm[0] ^ 0x8000000000000000ull), hi = (int64_t)(h_mm[1] ^ 0x8000000000000000ull);
    if (counts && lo <= hi && hi >= ((int64_t)1 << 31))
        return fail(e, VGX_ERR_ARG, me + "summary: the largest count is " + std::to_string(hi) + ", the column summary takes whole numbers below 2^31 (use narrower bins, or summarise the int64 counts on the host)");
    if (!counts && lo <= hi && (lo < 0 || hi >= ((int64_t)1 << 31)))
        return fail(e, VGX_ERR_ARG, me + "summary: a value of " + std::to_string(lo < 0 ? lo : hi) +
                                        " is not a whole number in [0, 2^31) (summarise the int64 values on the host)");
    char msg[512] = "";
    const int rcs = vgxi_column_summary_i32((me + "summary").c_str(), narrow, n, tc, summary, e->stream, msg, sizeof msg);
    return rcs ? fail(e, rcs, msg) : VGX_OK;
}
