// vgx_tau_lineages.hip — ancestral lineages per population and variant class of every selected replicate of a TAU ensemble at the
// times of one grid, on the device (vgx_get_tau_lineages), the host side of that call, and the same walk, tile walk and suffix sum
// compiled for the host (vgx_test_tau_lineages).  DESIGN.md §27.  Per pass, on one stream:
//   1. the canonicalise kernel of vgx_tau_genealogies.hip brings every own step's rows into the reference's order and granularity;
//   2. the walk kernel here: the tau walk of vgx_gwalk_tau.h with the logging observer of vgx_lineages.h, one replicate per wavefront,
//      lane 0 working, over the canonical rows and the shared flattened prefix.  It keeps the parents of the tree as workspace (the
//      closing pass reads them) and writes no tree, mutation or migration outputs: what leaves it is the lineage log, the result and
//      the six generator words;
//   3. the binning kernel and the suffix-sum kernel of vgx_lineages.hip, as they are, over bounds in EVENT-index space.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "vgx_engine.h"
#include "vgx_tau_lineages.h"
#include "vgx_tau_chain.h"

namespace {

__global__ void __launch_bounds__(64) vgxtl_walk_kernel(VgxTauLnLaunch a) {
    const int64_t i = (int64_t)blockIdx.x;
    if (threadIdx.x != 0 || i >= a.n) return;
    const VgxTauLnDesc d = a.desc[i];
    VgxGwRep w;
    w.n_ev = d.n_pre + d.n_steps; w.sCounter = d.sCounter; w.H = a.H; w.tsize = d.tsize;
    w.key = a.key + d.tab_off; w.cnt = a.cnt + d.tab_off;
    w.base = a.base + d.tab_off; w.len = a.len + d.tab_off; w.lcap = a.lcap + d.tab_off;
    w.arena = a.arena + d.arena_off; w.arena_cap = d.arena_cap;
    w.tree = a.tree + d.node_off; w.tree_pop = nullptr; w.node_ev = nullptr;   // (an observer without records: never touched)
    w.mut_cap = 0; w.mut_node = w.mut_AS = w.mut_DS = w.mut_site = w.mut_ev = nullptr;
    w.mig_cap = 0; w.mig_node = w.mig_old = w.mig_new = w.mig_ev = nullptr;
    const VgxGtChain c{a.pre, a.pre_off, d.n_pre, a.can + d.row_off, a.can_off + d.off_off, d.n_steps};
    VgxGtGen gen{{d.rng[0], d.rng[1], d.rng[2], d.rng[3]}, (int32_t)d.has32, (uint32_t)d.spare};
    VgxGwResult res{};
    VgxLnLog lg{a.rec + d.rec_off * 6, d.rec_cap, 0, 0};
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
        vgx_gt_walk(w, c, a.fresh + d.node_off, gen, res, VgxLnObserver{&lg});
        if (res.status == VGX_GW_OK && lg.dropped > 0) res.status = VGX_GW_WORKSPACE;   // a full lineage log
    }
    int64_t *r = a.res + i * 5;
    r[0] = res.status; r[1] = res.arg; r[2] = res.nodes_used; r[3] = res.mut_n; r[4] = res.mig_n;
    uint64_t *g = a.rng_out + i * 6;
    g[0] = gen.g.sh; g[1] = gen.g.sl; g[2] = gen.g.ih; g[3] = gen.g.il; g[4] = (uint64_t)gen.has32; g[5] = gen.spare;
    a.n_rec[i] = res.status == VGX_GW_OK ? lg.n : 0;
}

using namespace vgxtc;

// "" or why the grid, the classes or the LDS budget are refused (the wording of vgx_get_lineages)
std::string check_request(const double *grid, int64_t T, int64_t V, const int32_t *variant_of, int64_t P, int64_t H, bool events = false) {
    if (T < 1 || T >= VGX_PREV_MAX_POINTS || !grid) return "T = " + std::to_string(T) + " grid points: at least 1, below 2^24, with grid";
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(grid[k])) return "grid[" + std::to_string(k) + "] is not finite";
        if (k > 0 && !(grid[k - 1] < grid[k])) return "grid must increase strictly (grid[" + std::to_string(k) + "])";
    }
    if (V < 1 || V > INT32_MAX || !variant_of) return "V = " + std::to_string(V) + " classes: at least 1, with variant_of";
    for (int64_t h = 0; h < H; h++)
        if (variant_of[h] < -1 || variant_of[h] >= V)
            return "variant_of[" + std::to_string(h) + "] = " + std::to_string(variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")";
    if (vgx_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return std::to_string(P) + " populations x " + std::to_string(V) + " classes need " + std::to_string(vgx_prev_lds_bytes(P, V)) +
               " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use";
    if (events && vgx_te_lds_bytes(P, V) > VGX_PREV_LDS_MAX)   // (the tree events' cells: vgx_get_tree_events' wording)
        return std::to_string(P) + " populations x " + std::to_string(V) + " classes x " + std::to_string(VGX_TE_K) + " channels need " +
               std::to_string(vgx_te_lds_bytes(P, V)) + " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) +
               " bytes of LDS a counting workgroup may use";
    return "";
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t vgxi_tau_ln_walk(const VgxTauLnLaunch *a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vgxtl_walk_kernel, dim3((unsigned)a->n), dim3(64), 0, s, *a);
    return hipGetLastError();
}

// vgx_get_tau_lineages, and with `events` vgx_get_tau_tree_events: the block is then counts
// [n][T + 1][P][V][VGX_TE_K] behind io->values, binned by vgxi_te_bin, with no scan and no root.
static int tau_lineages_call(vgx_engine *e, vgx_tau_lineages_io *io, const vgx_tau_genealogy_prefix *prefix, const bool events, const char *name) {
    if (io->n < 0 || (io->n > 0 && (!io->replicates || !io->rng_state || !io->status || !io->status_arg || !io->records || !io->rng_out)))
        return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::string me = std::string(name) + ": ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    io->kernel_ms[0] = io->kernel_ms[1] = io->kernel_ms[2] = io->kernel_ms[3] = 0.0;
    if (!e->sc_host_valid || !e->last_was_tau || (int64_t)e->tau_log.size() < e->R)
        return fail(e, VGX_ERR_ARG, me + "the last call was not vgx_simulate_tau (walks tau chains only)");
    if (e->tau_mev_cap <= 0) return fail(e, VGX_ERR_ARG, me + "the last call recorded no multievent rows (record_events = 0)");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, PH = P * H, T = io->T, V = io->V, mev_cap = e->tau_mev_cap;
    {
        const std::string why = check_request(io->grid, T, V, io->variant_of, P, H, events);
        if (!why.empty()) return fail(e, VGX_ERR_ARG, me + why);
    }
    // the block: lineages' [n][T][cells] values and [n][cells] root, or the events' [n][T + 1][cells] counts with no root
    const int64_t cells = events ? P * V * VGX_TE_K : P * V, rows_out = events ? T + 1 : T;
    const int64_t pre_ev = prefix ? prefix->ev_ptr : 0;
    if (pre_ev >= VGX_PREV_MAX_EVENTS) return fail(e, VGX_ERR_ARG, me + "the prefix holds a chain of " + std::to_string(pre_ev) + " events (2^30 or more)");
    if (pre_ev < 0 ||
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
            const int64_t chain = (int64_t)lg.size() + (with_prefix[(size_t)i] ? pre_ev : 0);
            if (chain >= VGX_PREV_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " holds a chain of " + std::to_string(chain) + " events (2^30 or more)");
            if (rows >= ((int64_t)1 << 30) || 2 * s.sCounter > ((int64_t)1 << 31))
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
    int64_t tile = VGX_LN_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_LINEAGES_TILE_RECORDS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    typedef std::unique_ptr<char, void (*)(char *)> Hold;
    // what stays for the whole call: [rep | raw rows | sCounter | row sums | bound | variant_of | prefix rows | prefix offsets | val | fin | min, max]
    const int64_t val_bytes = n * rows_out * cells * 4, fin_bytes = events ? 0 : n * cells * 4;
    const int64_t o_rep = 0, o_raw = o_rep + up8(n * 8), o_sc = o_raw + up8(n * 8), o_cnt = o_sc + up8(n * 8), o_bnd = o_cnt + up8(n * 24),
                  o_map = o_bnd + up8(n * (T + 2) * 4), o_prow = o_map + up8(H * 4), o_poff = o_prow + up8(pre_rows * 32 + 32),
                  o_val = o_poff + up8((int64_t)pre.off.size() * 4), o_fin = o_val + up8(val_bytes), o_mm = o_fin + up8(fin_bytes), keep_total = o_mm + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(V) +
                                        " values (" + std::to_string(val_bytes + fin_bytes) + " bytes), its cuts and the prefix rows take " + std::to_string(keep_total) +
                                        " bytes, above half of the " + std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    Hold khold(kws, dev_free);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_raw, raw.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_sc, sC.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    if (pre_rows) HIPCHECK(e, hipMemcpyAsync(kws + o_prow, pre.rows.data(), (size_t)pre_rows * 32, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_poff, pre.off.data(), pre.off.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_val, 0, (size_t)(o_mm - o_val), e->stream));   // val and fin, zeroed once
    // raw sums of min(num, sCounter): MUTATION rows, MIGRATION rows, rows that can push a lineage
    std::vector<int64_t> cnt((size_t)n * 3);
    HIPCHECK(e, vgxi_tg_count((const int64_t *)e->t_mev.p, mev_cap, (const int64_t *)(kws + o_rep), (const int64_t *)(kws + o_raw),
                              (const int64_t *)(kws + o_sc), n, (int64_t *)(kws + o_cnt), e->stream));
    HIPCHECK(e, hipMemcpyAsync(cnt.data(), kws + o_cnt, (size_t)n * 24, hipMemcpyDeviceToHost, e->stream));
    if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));

    // host: the T + 2 bounds of every chain in event-index space.  The literal loop over the prefix's event times runs once; every
    // replicate that carries the prefix continues from its point over its own step times, a replicate that restarted starts at 0.
    const auto t_cuts = std::chrono::steady_clock::now();
    std::vector<int32_t> bounds((size_t)(n * (T + 2))), pbound((size_t)(T + 2), 0);
    int64_t point0 = 0;
    if (any_prefix) {
        VgxPrevCutter ct{io->grid, T, pbound.data()};
        for (int64_t i = 0; i < pre_ev; i++) ct.event(i, prefix->ev_times[i]);
        point0 = ct.point;
    }
    {
        int64_t steps_all = 0;
        for (int64_t i = 0; i < n; i++) steps_all += steps[(size_t)i];
        for_parts(n, [&](int64_t j0, int64_t j1, unsigned) {
            for (int64_t i = j0; i < j1; i++) {
                const auto &lg = e->tau_log[(size_t)io->replicates[i]];
                int32_t *bound = bounds.data() + i * (T + 2);
                VgxPrevCutter ct{io->grid, T, bound};
                const int64_t first = with_prefix[(size_t)i] ? pre_ev : 0;
                if (with_prefix[(size_t)i]) {
                    for (int64_t k = 1; k <= point0; k++) bound[k] = pbound[(size_t)k];
                    ct.point = point0;
                }
                for (size_t k = 0; k < lg.size(); k++) ct.event(first + (int64_t)k, lg[k].time);
                ct.finish(first + (int64_t)lg.size());
            }
        }, std::max<int64_t>(steps_all / n, 1) + T);
    }
    io->ms[1] += since(t_cuts);
    HIPCHECK(e, hipMemcpyAsync(kws + o_bnd, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, e->stream));

    // passes: what a replicate can need at most, from its raw rows
    auto nodes_of = [&](int64_t i) { return sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0; };
    auto table_of = [&](int64_t rows) { return vgx_gw_table_size(rows, PH); };
    auto arena_of = [&](int64_t i, int64_t tsize, int64_t pushes) {
        const int64_t all = pushes + (with_prefix[(size_t)i] ? pre_caps.direct_push + pre_caps.push(sC[(size_t)i]) : 0);
        return std::min(all, (tsize / 2) * sC[(size_t)i]);
    };
    std::vector<int64_t> bytes((size_t)n), rec_cap((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const bool wp = with_prefix[(size_t)i];
        const int64_t s = sC[(size_t)i], rows = raw[(size_t)i] + (wp ? pre_rows : 0), nodes = nodes_of(i);
        const int64_t tsize = nodes ? table_of(rows) : 0;
        rec_cap[(size_t)i] = vgx_ln_tau_capacity(s, cnt[(size_t)(3 * i)], cnt[(size_t)(3 * i + 1)], wp ? pre_caps.direct_mut + pre_caps.mut(s) : 0,
                                                 wp ? pre_caps.direct_mig + pre_caps.mig(s) : 0);
        bytes[(size_t)i] = raw[(size_t)i] * 32 + (steps[(size_t)i] + 1) * 8 + tsize * 28 + (nodes ? arena_of(i, tsize, cnt[(size_t)(3 * i + 2)]) : 0) * 4 +
                           nodes * 8 + rec_cap[(size_t)i] * 24 +
                           (int64_t)(sizeof(VgxTauLnDesc) + sizeof(VgxLnDesc) + sizeof(VgxGtCanonDesc) + sizeof(VgxGtCanonStat)) + 2048;
    }
    int64_t share = std::max<int64_t>((int64_t)(free_b / 2) - keep_total, 1);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // the stages of a pass, timed apart
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
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

        // ---- walk, binning, scan: [desc | bin desc | res | rng | n_rec | key | cnt | base | len | lcap | arena | fresh | parents | lineage logs]
        std::vector<VgxTauLnDesc> dp((size_t)m);
        std::vector<VgxLnDesc> bd((size_t)m);
        int64_t TB = 0, A = 0, N = 0, Rc = 0, max_rec = 0;
        for (int64_t j = 0; j < m; j++) {
            const int64_t gi = i0 + j;
            VgxTauLnDesc &d = dp[(size_t)j];
            const VgxGtCanonStat &st = stat[(size_t)j];
            d.rep = io->replicates[gi];
            d.n_pre = with_prefix[(size_t)gi] ? pre_ev : 0;
            d.n_steps = cd[(size_t)j].n_steps;
            d.sCounter = sC[(size_t)gi];
            d.status = st.status; d.arg = st.arg;
            const bool walk = d.sCounter >= 2 && st.status == VGX_GW_OK;
            d.tsize = walk ? table_of(st.n_rows + (with_prefix[(size_t)gi] ? pre_rows : 0)) : 0;
            d.arena_cap = walk ? arena_of(gi, d.tsize, st.pushes) : 0;
            d.rec_cap = walk ? rec_cap[(size_t)gi] : 0;
            d.row_off = cd[(size_t)j].row_off; d.off_off = cd[(size_t)j].off_off;
            for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[gi * 6 + k];
            d.has32 = io->rng_state[gi * 6 + 4] != 0; d.spare = (int64_t)(uint32_t)io->rng_state[gi * 6 + 5];
            d.tab_off = TB; d.arena_off = A; d.node_off = N; d.rec_off = Rc;
            TB += d.tsize; A += d.arena_cap; N += nodes_of(gi); Rc += d.rec_cap;
            max_rec = std::max<int64_t>(max_rec, d.rec_cap);
            VgxLnDesc &b = bd[(size_t)j];   // what the binning kernel reads of a replicate: where its log lies
            b = VgxLnDesc{};
            b.rep = d.rep; b.n_ev = d.n_pre + d.n_steps; b.sCounter = d.sCounter; b.rec_off = d.rec_off; b.rec_cap = d.rec_cap;
        }
        const int64_t o_desc = 0, o_bdesc = o_desc + up8(m * (int64_t)sizeof(VgxTauLnDesc)), o_res = o_bdesc + up8(m * (int64_t)sizeof(VgxLnDesc)),
                      o_rng = o_res + up8(m * 40), o_nrec = o_rng + up8(m * 48), o_key = o_nrec + up8(m * 8), o_tcnt = o_key + up8(TB * 8),
                      o_base = o_tcnt + up8(TB * 8), o_len = o_base + up8(TB * 4), o_lcap = o_len + up8(TB * 4), o_arena = o_lcap + up8(TB * 4),
                      o_fresh = o_arena + up8(A * 4), o_tree = o_fresh + up8(N * 4), o_rec = o_tree + up8(N * 4), total = o_rec + up8(Rc * 24);
        char *ws = nullptr;
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        Hold hold(ws, dev_free);
        VgxTauLnLaunch a{};
        a.n = m;
        a.desc = (const VgxTauLnDesc *)(ws + o_desc);
        a.pre = (const VgxGtRow *)(kws + o_prow); a.pre_off = (const int32_t *)(kws + o_poff);
        a.can = ca.can; a.can_off = ca.can_off;
        a.I = (const int32_t *)e->t_I.p;
        a.P = P; a.H = H;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_tcnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena); a.fresh = (int32_t *)(ws + o_fresh); a.tree = (int32_t *)(ws + o_tree);
        a.rec = (int32_t *)(ws + o_rec);
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        a.n_rec = (int64_t *)(ws + o_nrec);
        VgxLnLaunch b{};   // the binning and the scan of vgx_lineages.hip read these fields alone
        b.m = m;
        b.desc = (const VgxLnDesc *)(ws + o_bdesc);
        b.P = P; b.H = H;
        b.rec = a.rec; b.n_rec = a.n_rec;
        b.bound = (const int32_t *)(kws + o_bnd) + i0 * (T + 2);
        b.T = (int32_t)T; b.V = (int32_t)V;
        b.variant_of = (const int32_t *)(kws + o_map);
        b.tile = (int32_t)tile; b.max_rec = max_rec;
        b.val = (int32_t *)(kws + o_val) + i0 * rows_out * cells;
        b.fin = (int32_t *)(kws + o_fin) + i0 * cells;
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxTauLnDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_bdesc, bd.data(), (size_t)m * sizeof(VgxLnDesc), hipMemcpyHostToDevice, e->stream));
        if (TB > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)TB * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_tau_ln_walk(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        if (events) {
            const VgxTeLaunch te{m, b.desc, b.rec, b.n_rec, b.bound, b.T, (int32_t)P, (int32_t)H, b.V, b.variant_of, b.tile, max_rec, b.val};
            HIPCHECK(e, vgxi_te_bin(&te, e->stream));
        } else {
            HIPCHECK(e, vgxi_ln_bin(&b, e->stream));
        }
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        if (!events) HIPCHECK(e, vgxi_ln_scan(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[3], e->stream));
        std::vector<int64_t> res((size_t)m * 5), nrec((size_t)m);
        HIPCHECK(e, hipMemcpyAsync(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 6, a.rng_out, (size_t)m * 48, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(nrec.data(), a.n_rec, (size_t)m * 8, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // before anything reads the outputs
            return fail(e, VGX_ERR_HIP, me + "walk, binning or scan kernel failed: " + hipGetErrorString(er));
        for (int k = 0; k < 3; k++) {
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->kernel_ms[k + 1] += kms;
            io->ms[0] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            io->status[i0 + j] = res[(size_t)(j * 5)];
            io->status_arg[i0 + j] = res[(size_t)(j * 5 + 1)];
            io->records[i0 + j] = nrec[(size_t)j];
        }
        io->passes += 1;
        i0 = i1;
    }
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (!events) HIPCHECK(e, hipMemcpy(io->root, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        if (!io->summary->group_of) return fail(e, VGX_ERR_ARG, me + "summary: null group_of");
        int64_t failed = 0;
        for (int64_t i = 0; i < n; i++) failed += io->summary->group_of[i] >= 0 && io->status[i] != VGX_GW_OK;
        if (failed > 0)
            return fail(e, VGX_ERR_ARG, me + "summary: " + std::to_string(failed) + " replicate(s) of a group have a walk that failed (status is not 0): leave them out of the groups");
        // the column summary sorts 32-bit keys of whole numbers in [0, 2^31)
        int32_t mm[2] = {0, 0};
        HIPCHECK(e, vgxi_prev_minmax((const int32_t *)(kws + o_val), n * rows_out * cells, (int32_t *)(kws + o_mm), e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "min/max kernel failed: " + hipGetErrorString(er));
        if (mm[0] < 0) return fail(e, VGX_ERR_ARG, me + "summary: a value of " + std::to_string(mm[0]) + " is not a whole number in [0, 2^31)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32((me + "summary").c_str(), (const int32_t *)(kws + o_val), n, rows_out * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

extern "C" int vgx_get_tau_lineages(vgx_engine *e, vgx_tau_lineages_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io || (io->n > 0 && !io->root)) return VGX_ERR_ARG;
    return tau_lineages_call(e, io, prefix, false, "vgx_get_tau_lineages");
}

extern "C" int vgx_get_tau_tree_events(vgx_engine *e, vgx_tau_tree_events_io *io, const vgx_tau_genealogy_prefix *prefix) {
    if (!e || !io) return VGX_ERR_ARG;
    vgx_tau_lineages_io l{};
    l.n = io->n; l.replicates = io->replicates; l.rng_state = io->rng_state;
    l.T = io->T; l.grid = io->grid; l.V = io->V; l.variant_of = io->variant_of;
    l.values = io->counts;
    l.status = io->status; l.status_arg = io->status_arg; l.records = io->records; l.rng_out = io->rng_out;
    l.summary = io->summary;
    const int rc = tau_lineages_call(e, &l, prefix, true, "vgx_get_tau_tree_events");
    io->passes = l.passes;
    for (int k = 0; k < 3; k++) { io->ms[k] = l.ms[k]; io->kernel_ms[k] = l.kernel_ms[k]; }
    return rc;
}

// ---- the host instance: the chain handling of vgx_test_tau_genealogy_walk, the walk with the logging observer, the tile walk and the
// suffix sum on a chain given as arrays (no device, no engine)
// (with `events`, vgx_test_tau_tree_events: `values` is counts [T + 1][P][V][VGX_TE_K] by vgx_te_tile_host, no root, no suffix sum)
static int tau_lineages_hook(vgx_genealogy_io *io, int64_t sites, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                             int32_t *values, int32_t *root, int64_t *records, char *errbuf, int64_t errcap, const bool events, const char *name) {
    auto fail_ = [&](const std::string &m) {
        if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", m.c_str());
        return VGX_ERR_ARG;
    };
    auto message = [](int64_t status, int64_t arg) {
        char buf[512];
        vgx_genealogy_message(status, arg, buf, 512);
        return std::string(buf);
    };
    const std::string me = std::string(name) + ": ";
    if (!io || !io->infectious || !grid || !variant_of || !values || (!events && !root) || !records) return fail_(me + "null argument");
    const int64_t P = io->popNum, H = io->hapNum, PH = P * H, sC = io->sCounter, n = io->ev_ptr;
    if (P < 1 || H < 1 || P > INT32_MAX || H > INT32_MAX) return fail_(me + "bad dimensions");
    if (T < 1 || T >= VGX_PREV_MAX_POINTS) return fail_(me + "T = " + std::to_string(T) + " must be at least 1 and below 2^24");   // (vgx_test_lineages' words)
    if (V < 1 || V > INT32_MAX) return fail_(me + "V = " + std::to_string(V) + " must be at least 1");
    {
        const std::string why = check_request(grid, T, V, variant_of, P, H, events);
        if (!why.empty()) return fail_(me + why);
    }
    if (tile < 0) return fail_(me + "tile must not be negative");
    if (tile == 0) tile = VGX_LN_TILE_DEFAULT;
    if (sC < 2) return fail_(message(VGX_GW_FEW_SAMPLES, 0));
    if (n < 0 || n >= VGX_PREV_MAX_EVENTS) return fail_(me + "a chain of " + std::to_string(n) + " events (2^30 or more)");
    if (2 * sC > ((int64_t)1 << 31) || sites < 0) return fail_(me + "chain too long");
    if (n > 0 && (!io->ev_times || !io->ev_types || !io->ev_haplotypes || !io->ev_populations || !io->ev_newHaplotypes || !io->ev_newPopulations))
        return fail_(me + "null event column");
    if (io->mev_rows > 0 && (!io->mev_num || !io->mev_types || !io->mev_haplotypes || !io->mev_populations || !io->mev_newHaplotypes || !io->mev_newPopulations))
        return fail_(me + "null multievent column");
    HostChain hc;
    const std::string why = host_chain(io, sites, me, message, hc);
    if (!why.empty()) return fail_(why);
    const int64_t nodes = 2 * sC - 1, tsize = hc.tsize;
    // the capacity of the log from the canonical rows, which the device bounds from above by its raw rows
    int64_t own_mut = 0, own_mig = 0;
    for (const VgxGtRow &r : hc.can) {
        own_mut += r.type == VGX_GW_MUTATION ? std::min<int64_t>(std::max<int64_t>(r.num, 0), sC) : 0;
        own_mig += r.type == VGX_GW_MIGRATION ? std::min<int64_t>(std::max<int64_t>(r.num, 0), sC) : 0;
    }
    const int64_t rec_cap = vgx_ln_tau_capacity(sC, own_mut, own_mig, hc.caps.direct_mut + hc.caps.mut(sC), hc.caps.direct_mig + hc.caps.mig(sC));
    std::vector<int64_t> key((size_t)tsize, -1), cnt((size_t)tsize);
    std::unique_ptr<int32_t[]> base(new int32_t[(size_t)tsize]), len(new int32_t[(size_t)tsize]), lcap(new int32_t[(size_t)tsize]);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(hc.arena_cap, 1)), fresh((size_t)nodes), tree((size_t)nodes), rec((size_t)rec_cap * 6);
    VgxGwRep w{};
    w.n_ev = n; w.sCounter = sC; w.H = H; w.tsize = tsize;
    w.key = key.data(); w.cnt = cnt.data(); w.base = base.get(); w.len = len.get(); w.lcap = lcap.get();
    w.arena = arena.data(); w.arena_cap = hc.arena_cap;
    w.tree = tree.data();   // (the observer keeps no records: the other outputs are never touched)
    const VgxGtChain c = hc.chain(n);
    VgxGwResult res{};
    res.status = vgx_gt_prepass(w, c);
    if (res.status != VGX_GW_OK) return fail_(message(res.status, res.arg));
    for (int64_t s = 0; s < tsize; s++)
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) cnt[(size_t)s] = io->infectious[key[(size_t)s]];
    VgxGtGen gen{{io->rng_state[0], io->rng_state[1], io->rng_state[2], io->rng_state[3]}, io->rng_has_uint32 != 0, (uint32_t)io->rng_uinteger};
    VgxLnLog lg{rec.data(), rec_cap, 0, 0};
    vgx_gt_walk(w, c, fresh.data(), gen, res, VgxLnObserver{&lg});
    if (res.status == VGX_GW_OK && lg.dropped > 0) res.status = VGX_GW_WORKSPACE;
    for (int64_t s = 0; s < tsize; s++)   // walked back in place, as the host pass does
        if (key[(size_t)s] >= 0 && key[(size_t)s] < PH) io->infectious[key[(size_t)s]] = cnt[(size_t)s];
    if (res.status != VGX_GW_OK) return fail_(message(res.status, res.arg));
    io->nodes_used = res.nodes_used;
    io->rng_state[0] = gen.g.sh; io->rng_state[1] = gen.g.sl; io->rng_state[2] = gen.g.ih; io->rng_state[3] = gen.g.il;
    io->rng_has_uint32 = gen.has32 ? 1 : 0;
    io->rng_uinteger = gen.spare;
    *records = lg.n;
    // the bounds in event-index space from the chain's event times, the tile walk over the lineage log, the suffix sum
    std::vector<int32_t> bound((size_t)(T + 2));
    VgxPrevCutter ct{grid, T, bound.data()};
    for (int64_t e = 0; e < n; e++) ct.event(e, io->ev_times[e]);
    ct.finish(n);
    if (events) {
        const int64_t cells = P * V * VGX_TE_K;
        for (int64_t i = 0; i < (T + 1) * cells; i++) values[i] = 0;
        std::vector<int32_t> hist((size_t)cells, 0);
        for (int64_t r0 = 0; r0 < lg.n; r0 += tile)
            vgx_te_tile_host(rec.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, variant_of, r0, std::min<int64_t>(r0 + tile, lg.n),
                             hist.data(), values);
        return VGX_OK;
    }
    const int64_t cells = P * V;
    for (int64_t i = 0; i < T * cells; i++) values[i] = 0;
    for (int64_t i = 0; i < cells; i++) root[i] = 0;
    std::vector<int32_t> hist((size_t)cells, 0);
    for (int64_t r0 = 0; r0 < lg.n; r0 += tile)
        vgx_ln_tile_host(rec.data(), bound.data(), (int32_t)T, (int32_t)P, (int32_t)H, (int32_t)V, variant_of, r0, std::min<int64_t>(r0 + tile, lg.n),
                         hist.data(), values, root);
    for (int64_t i = 0; i < cells; i++) vgx_ln_scan_column(values + i, root + i, (int32_t)T, cells);
    return VGX_OK;
}

extern "C" int vgx_test_tau_lineages(vgx_genealogy_io *io, int64_t sites, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                                     int32_t *values, int32_t *root, int64_t *records, char *errbuf, int64_t errcap) {
    return tau_lineages_hook(io, sites, grid, T, variant_of, V, tile, values, root, records, errbuf, errcap, false, "vgx_test_tau_lineages");
}

extern "C" int vgx_test_tau_tree_events(vgx_genealogy_io *io, int64_t sites, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                                        int32_t *counts, int64_t *records, char *errbuf, int64_t errcap) {
    return tau_lineages_hook(io, sites, grid, T, variant_of, V, tile, counts, nullptr, records, errbuf, errcap, true, "vgx_test_tau_tree_events");
}
