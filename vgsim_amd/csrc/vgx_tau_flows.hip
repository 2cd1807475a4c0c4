// vgx_tau_flows.hip — new infections per time bin, source population, destination population and variant class of every selected
// replicate of a TAU ensemble on the device (vgx_get_tau_flows), the host side of that call, and the same rule and tile walk
// compiled for the host (vgx_test_tau_flows).  The rule is vgx_tau_flows.h; DESIGN.md §24.
//
// COUNTING kernel.  The geometry and the row loads of vgx_tau_incidence.hip: a workgroup of 256 threads takes one chain (a
// selected replicate's own rows in its block of t_mev, or the flattened prefix) and a TILE of consecutive rows; consecutive lanes
// read consecutive rows (three 16-byte loads per lane).  The tile is clipped to the window [cut[0], cut[T]); its first bin comes
// from a search in the chain's cuts, read where they lie; bin by bin `num` is added with 64-bit LDS atomics to the int64 cells
// the form keeps (vgx_flows.h: all P * P * V, or the P * V of the diagonal, a row off the diagonal then adding num to its cell of
// the bin's block in device memory with one 64-bit atomic), and at every bin change and at the tile's end the nonzero cells go to
// the block in device memory with 64-bit integer atomics and are cleared.  variant_of is staged in LDS behind the cells when it
// fits.  Rows outside the window feed the chain's two `outside` counters: a per-thread sum, a wave sum, one atomic per wavefront.
// All arithmetic is integer: the block does not depend on the form, the tile size, the launch geometry or the chunking.
// The tile size is VGX_FLOWS_TILE_EVENTS (rows here; default 4096, DESIGN.md §16 for why).
// The prefix is counted ONCE per call as a chain of its own; an init kernel then starts the block of every selected replicate
// that did not restart from the prefix block, and the replicates' own rows are added on top.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "vgx_tau_flows.h"
#include "vgx_tau_replay.h"   // the frame: selection, cuts, workspace, prefix pass, chunks, summary, the hook's chain split

namespace {

template <int FORM>
__global__ void __launch_bounds__(256) vgxtf_count_kernel(VgxTauFlowLaunch a, int stage) {
    extern __shared__ __attribute__((aligned(16))) long long hist[];   // dense: [P][P][V] cells, split: [P][V]; then (stage) variant_of [hapNum]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const int32_t n = a.n_rows[row], T = a.T, P = a.P, V = a.V, cells = P * P * V;
    const int32_t kept = FORM == VGX_FLOW_DENSE ? cells : P * V;
    const int32_t *cut = a.cut + row * (int64_t)(T + 1);   // (uniform addresses: every thread reads the same cuts)
    // 16-byte aligned: 48-byte rows from 256-byte aligned bases
    const longlong2 *rows = (const longlong2 *)(a.rows + (a.rep ? a.rep[row] * a.stride * 6 : 0));
    long long *out = (long long *)a.counts + row * (int64_t)T * cells, *outside = (long long *)a.outside + 2 * row;
    const int32_t *vo = a.variant_of;
    long long before = 0, after = 0;       // this thread's share of the rows outside the window
    bool clean = false;                    // the cells are zeroed and the map staged before the first tile that counts
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
            for (int i = tid; i < kept; i += 256) hist[i] = 0;
            if (stage) {
                int32_t *map = (int32_t *)(hist + kept);
                for (int i = tid; i < a.hapNum; i += 256) map[i] = vo[i];
                vo = map;
            }
            clean = true;
            __syncthreads();
        }
        while (pos < hi) {
            const int32_t b = vgx_inc_bin(cut, T, pos);
            const int32_t end = hi < cut[b + 1] ? hi : cut[b + 1];
            long long *dstb = out + (int64_t)b * cells;
            for (int64_t e = (int64_t)pos + tid; e < end; e += 256) {
                const longlong2 r0 = rows[e * 3], r1 = rows[e * 3 + 1], r2 = rows[e * 3 + 2];
                int32_t src, dst, cls;
                const long long w = vgx_tau_flow_row(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, P, a.hapNum, vo, a.within, src, dst, cls);
                if (!w) continue;
                if (FORM == VGX_FLOW_DENSE) add64(&hist[vgx_flow_index(P, V, src, dst, cls)], w);
                else if (src == dst) add64(&hist[src * V + cls], w);
                else add64(&dstb[vgx_flow_index(P, V, src, dst, cls)], w);
            }
            __syncthreads();
            for (int i = tid; i < kept; i += 256) {
                const long long v = hist[i];
                if (v) { add64(&dstb[FORM == VGX_FLOW_DENSE ? i : vgx_flow_diag_index(P, V, i)], v); hist[i] = 0; }
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

template <int FORM>
hipError_t launch(const VgxTauFlowLaunch *a, hipStream_t s) {
    const bool stage = vgx_tau_flow_stage_map(FORM, a->P, a->V, a->hapNum);
    const int64_t lds = vgx_tau_flow_lds_bytes(FORM, a->P, a->V) + (stage ? 4 * (int64_t)a->hapNum : 0);
    const int64_t all_tiles = (a->max_n + a->tile - 1) / a->tile;
    const unsigned tiles = (unsigned)(all_tiles < 65535 ? all_tiles : 65535);   // (a workgroup takes several tiles beyond that)
    hipError_t err = hipFuncSetAttribute((const void *)vgxtf_count_kernel<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgxtf_count_kernel<FORM>, dim3((unsigned)a->m, tiles), dim3(256), (size_t)lds, s, *a, stage ? 1 : 0);
    return hipGetLastError();
}

// what both the call and the hook check about the grid, the map and the form; "" or why not.  `ran` gets the form that runs.
std::string check_request(const double *edges, int64_t T, int64_t V, const int32_t *variant_of, int64_t P, int64_t H, int asked, int &ran) {
    if (T < 1 || T >= VGX_FLOW_MAX_BINS || !edges) return "T = " + std::to_string(T) + " bins: at least 1, below 2^24, with edges";
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(edges[k])) return "edges[" + std::to_string(k) + "] is not finite";
        if (k > 0 && !(edges[k - 1] < edges[k])) return "edges must increase strictly (edges[" + std::to_string(k) + "])";
    }
    if (V < 1 || V > INT32_MAX || !variant_of) return "V = " + std::to_string(V) + " classes: at least 1, with variant_of";
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")";
    ran = vgx_tau_flow_form(asked, P, V);
    if (!ran) {
        char why[256];
        vgx_tau_flow_refusal(asked, P, V, why, sizeof why);
        return why;
    }
    return "";
}

}  // namespace

extern "C" hipError_t vgxi_tau_flow_count(const VgxTauFlowLaunch *a, hipStream_t s) {
    if (a->m <= 0 || a->max_n <= 0) return hipSuccess;
    if ((a->form != VGX_FLOW_DENSE && a->form != VGX_FLOW_SPLIT) || vgx_tau_flow_form(a->form, a->P, a->V) != a->form || a->tile < 1)
        return hipErrorInvalidValue;
    return a->form == VGX_FLOW_DENSE ? launch<VGX_FLOW_DENSE>(a, s) : launch<VGX_FLOW_SPLIT>(a, s);
}

// The frame of vgx_tau_replay.h around the block [n][T][P][P][V], with vgx_get_flows's variant_of, `within` and form.
extern "C" int vgx_get_tau_flows(vgx_engine *e, vgx_tau_flows_io *io, const vgx_timelines_prefix *prefix) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = "vgx_get_tau_flows: ";
    io->passes = 0;
    io->form = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V, mev_cap = e->tau_mev_cap;
    int form = 0;
    TauSel sel;
    auto request = [&]() -> std::string {
        int asked = VGX_FLOW_AUTO;
        if (const char *fm = getenv("VGX_FLOWS_FORM")) {
            if (!strcmp(fm, "dense")) asked = VGX_FLOW_DENSE;
            else if (!strcmp(fm, "split")) asked = VGX_FLOW_SPLIT;
            else if (*fm) return std::string("VGX_FLOWS_FORM=") + fm + " is neither dense nor split";
        }
        const std::string why = check_request(io->edges, T, V, io->variant_of, P, H, asked, form);
        if (why.empty()) io->form = form;
        return why;
    };
    if (const int rc = tau_select(e, me, "counts", request, n, io->replicates, prefix, false, tau_every, sel)) return rc;
    const int64_t cells = P * P * V, tc = T * cells, pre_rows = sel.pre_rows;   // (P * V <= 2^13 and P <= 2^13: cells below 2^26)
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    const std::string dims = std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x " + std::to_string(P) + " x " + std::to_string(V);
    if (tc >= ((int64_t)1 << 40) / n)
        return fail(e, VGX_ERR_ARG, me + "the block of " + dims + " counts holds 2^40 cells or more: select fewer replicates per call");
    int64_t tile = VGX_FLOW_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_FLOWS_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_FLOW_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    // what stays for the whole call: [rep | n_own | with | variant_of | prefix: rows, cut, n_rows, block, outside | counts | outside | narrow | min, max]
    const int64_t block_bytes = n * tc * 8, narrow_bytes = io->summary ? n * tc * 4 : 0;
    DevLayout lay;
    const int64_t o_rep = lay.take(n * 8), o_nown = lay.take(n * 4), o_with = lay.take(n * 4), o_map = lay.take(H * 4), o_prow = lay.take(pre_rows * 48 + 8),
                  o_pcut = lay.take((T + 1) * 4), o_pn = lay.take(4), o_pcnt = lay.take(tc * 8), o_pout = lay.take(16), o_cnt = lay.take(block_bytes),
                  o_out = lay.take(n * 16), o_nar = lay.take(narrow_bytes + 8), o_mm = lay.take(16), keep_total = lay.total;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + dims + " counts of 8 bytes, the prefix block, the prefix rows and " +
                                        (io->summary ? "the summary's 4-byte copy take " : "their counters take ") + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    DevHold khold;
    if (const int rc = dev_alloc(e, me, keep_total, khold)) return rc;
    char *const kws = khold.get();
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nown, sel.n_own.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_with, sel.with_prefix.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_pcnt, 0, (size_t)(o_cnt - o_pcnt), e->stream));   // the prefix block and its outside counters
    VgxTauFlowLaunch base{};   // what every launch of the call shares
    base.T = (int32_t)T; base.P = (int32_t)P; base.hapNum = (int32_t)H; base.V = (int32_t)V;
    base.variant_of = (const int32_t *)(kws + o_map);
    base.within = io->within ? 1 : 0; base.form = form; base.tile = (int32_t)tile;

    // the prefix, once: flattened rows uploaded, its cuts, counted as a chain of its own
    int64_t point0 = 0;
    int rc = tau_prefix_pass<VgxIncCutter, 0>(e, me, io->ms, sel, prefix ? prefix->ev_times : nullptr, io->edges, T, kws + o_prow, kws + o_pcut, kws + o_pn, point0, [&]() -> int {
        VgxTauFlowLaunch a = base;
        a.m = 1;
        a.rows = (const int64_t *)(kws + o_prow); a.stride = 0; a.rep = nullptr;
        a.n_rows = (const int32_t *)(kws + o_pn); a.cut = (const int32_t *)(kws + o_pcut);
        a.max_n = pre_rows;
        a.counts = (int64_t *)(kws + o_pcnt); a.outside = (int64_t *)(kws + o_pout);
        HIPCHECK(e, vgxi_tau_flow_count(&a, e->stream));
        if (pre_rows > 0) io->passes += 1;
        return VGX_OK;
    });
    if (rc) return rc;
    // chunks of replicates: their blocks start from the prefix's or from zero, their own rows are counted on top
    rc = tau_chunks<VgxIncCutter, 0>(e, me, me + "counting kernel failed: ", io->ms, sel, n, io->replicates, io->edges, T, point0, (int64_t)(free_b / 2) - keep_total,
                                     [&](int64_t i0, int64_t m, int64_t max_n, const int32_t *cuts) -> int {
        VgxTauFlowLaunch a = base;
        a.m = m;
        a.rows = (const int64_t *)e->t_mev.p; a.stride = mev_cap;
        a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_rows = (const int32_t *)(kws + o_nown) + i0;
        a.cut = cuts;
        a.max_n = max_n;
        a.counts = (int64_t *)(kws + o_cnt) + i0 * tc; a.outside = (int64_t *)(kws + o_out) + 2 * i0;
        HIPCHECK(e, vgxi_tau_block_init(m, tc, 0, (const int32_t *)(kws + o_with) + i0, (const int64_t *)(kws + o_pcnt), nullptr, (const int64_t *)(kws + o_pout),
                                        a.counts, nullptr, a.outside, e->stream));
        HIPCHECK(e, vgxi_tau_flow_count(&a, e->stream));
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

// ---- the host instance: the same flattening, cuts, cell and tile walk on a chain given as arrays (no device, no engine).  The
// last n_own_events events play the replicate's own steps, everything before them the prefix, which is counted once as a chain
// of its own and added, as on the device (tau_hook_split, tau_hook_count).
extern "C" int vgx_test_tau_flows(vgx_tau_flows_chain *io, char *errbuf, int64_t errcap) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "vgx_test_tau_flows: %s", m.c_str());
        return VGX_ERR_ARG;
    };
    if (!io || !io->counts || !io->outside) return fail_("null argument");
    const int64_t T = io->T, P = io->popNum, H = io->hapNum, V = io->V;
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail_("bad dimensions");
    if (io->form != VGX_FLOW_AUTO && io->form != VGX_FLOW_DENSE && io->form != VGX_FLOW_SPLIT)
        return fail_("form = " + std::to_string(io->form) + " is none of 0 (automatic), 1 (dense), 2 (split)");
    int ran = 0;
    std::string why = check_request(io->edges, T, V, io->variant_of, P, H, (int)io->form, ran);
    if (!why.empty()) return fail_(why);
    io->form_ran = ran;
    const int64_t cells = P * P * V;
    TauHookChain c;
    why = tau_hook_split(io, VGX_FLOW_TILE_DEFAULT, T * cells, c);
    if (!why.empty()) return fail_(why);
    std::vector<int32_t> pcut, ocut;
    tau_hook_marks<VgxIncCutter, 0>(c, io->ev_times, io->edges, T, pcut, ocut);
    const int32_t within = io->within ? 1 : 0;
    std::vector<int64_t> hist((size_t)(vgx_tau_flow_lds_bytes(ran, P, V) / 8), 0);
    int64_t *const dst[2] = {io->counts, io->outside};
    const int64_t len[2] = {T * cells, 2};
    tau_hook_count(c, pcut.data(), ocut.data(), dst, len, [&](const int64_t *rows, const int32_t *cut, int32_t t0, int32_t t1, int64_t *const *b) {
        vgx_tau_flow_tile_host(ran, rows, cut, (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, io->variant_of, within, t0, t1, hist.data(), b[0], b[1]);
    });
    return VGX_OK;
}
