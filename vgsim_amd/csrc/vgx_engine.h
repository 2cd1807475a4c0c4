// vgx_engine.h — the engine behind the C ABI of include/vgx.h, as the host drivers of libvgx.so share it: the engine structure,
// its device buffers and error helpers, the launchers defined next to their kernels.  Host-only; included by the host drivers
// (vgx_api.hip, vgx_direct_run.hip, vgx_tau_run.hip, vgx_tau_timelines.hip, vgx_tau_genealogies.hip, vgx_tau_lineages.hip; the tau replays through their frame, vgx_tau_replay.h) alone. Helpers that several of them use are `inline` here; direct_core and the
// choice of its kernel have their one definition in vgx_direct_run.hip, host_clock in vgx_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <chrono>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../include/vgx.h"
#include "vgx_dev.h"
#include "vgx_quadg.h"
#include "vgx_taus.h"
#include "vgx_solo.h"
#include "vgx_lone.h"
#include "vgx_gwalk.h"
#include "vgx_tline.h"
#include "vgx_timelines.h"
#include "vgx_incidence.h"
#include "vgx_prevalence.h"
#include "vgx_milestones.h"
#include "vgx_flows.h"
#include "vgx_lineages.h"
#include "vgx_tree_events.h"   // (declares its launcher, vgxi_te_bin, itself)
#include "vgx_tree_shape.h"    // (likewise: vgxi_ts_shape)
#include "vgx_tau_tree_shape.h"   // (likewise: vgxi_tts_times)

#pragma GCC visibility push(hidden)   // nothing here is part of the exported C ABI

// launchers defined next to their kernels (vgx_direct.hip)
extern "C" hipError_t vgxi_launch_direct(const VgxDirectArgs *a, size_t lds, hipStream_t stream);
extern "C" hipError_t vgxi_launch_direct_sets(const VgxDirectArgs *a, const VgxDevParams *psets, const int32_t *set_of, size_t lds, hipStream_t stream);
extern "C" int vgxi_tau_inc_shards(int64_t H, int64_t P);
extern "C" int64_t vgxi_tau_queue_shards(int64_t H, int64_t P);
extern "C" int64_t vgxi_tau_queue_shard_max(int64_t H);
extern "C" int vgxi_tau_drift_blocks(const VgxTauArgs *a);
extern "C" hipError_t vgxi_tau_sieve(const VgxTauArgs *a, hipStream_t s);
extern "C" hipError_t vgxi_launch_lanes(const VgxDirectArgs *a, const VgxLaneWs *w, hipStream_t stream);
extern "C" hipError_t vgxi_launch_quad(const VgxDirectArgs *a, const double *cd, double *effMig, double *maxEBM, int32_t *has_mig, int long_lists,
                                       int plain_div, hipStream_t stream);
extern "C" size_t vgxi_direct_lds_bytes(int P, int S, int C, int CB);
extern "C" hipError_t vgxi_launch_counts64(const int32_t *c32, int64_t *c64, int64_t n, hipStream_t stream);
extern "C" hipError_t vgxi_launch_quad_prep(const VgxDevParams *p, const double *cd, double *effMig, double *maxEBM, int32_t *has_mig, hipStream_t stream);
extern "C" hipError_t vgxi_launch_quadf(const VgxDirectArgs *a, const double *cd, double *effMig, double *maxEBM, int32_t *has_mig, hipStream_t stream);
extern "C" hipError_t vgxi_launch_taus(const VgxTausArgs *a, hipStream_t s);
extern "C" hipError_t vgxi_launch_taus_sets(const VgxTausSetsArgs *sa, int max_C, int max_CB, hipStream_t s);
extern "C" hipError_t vgxi_launch_quadg(const VgxDirectArgs *a, const VgxQuadgArgs *qa, hipStream_t stream);
extern "C" hipError_t vgxi_launch_solo(const VgxDirectArgs *a, const VgxSoloArgs *sa, int clock, hipStream_t stream);
extern "C" hipError_t vgxi_launch_lone(const VgxDirectArgs *a, const VgxLoneArgs *la, int clock, hipStream_t stream);
extern "C" hipError_t vgxi_gw_count(const int32_t *log, int64_t evcap, const int64_t *reps, const int64_t *n_ev, int64_t n, int64_t *out,
                                    hipStream_t s);
extern "C" hipError_t vgxi_gw_walk(const VgxGwLaunch *a, int wave, hipStream_t s);
extern "C" hipError_t vgxi_tl_pack(const int32_t *log, const double *evrate, int64_t evcap, const int64_t *rep, const int32_t *n_ev,
                                   const int64_t *off, int64_t m, int64_t max_n, int32_t *iter_out, double *rate_out, hipStream_t s);
extern "C" hipError_t vgxi_tl_replay(const VgxTlLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_inc_count(const VgxIncLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_prev_count(const VgxPrevLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_prev_scan(const VgxPrevLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_prev_minmax(const int32_t *x, int64_t n, int32_t *out, hipStream_t s);   // out[0] = min, out[1] = max of x[0 .. n)
extern "C" hipError_t vgxi_ms_walk(const VgxMsLaunch *g, int waves, hipStream_t s);   // vgx_milestones.hip: the ordered walk over the bases of pass A
extern "C" hipError_t vgxi_sus_count(const VgxPrevLaunch *a, hipStream_t s);   // vgx_susceptible.hip: hapNum := susNum, V := G, variant_of := class_of
// vgx_lineages.hip: the walk with the logging observer, the binning of the lineage logs, the suffix sum (one pass, one stream)
extern "C" hipError_t vgxi_ln_walk(const VgxLnLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_ln_bin(const VgxLnLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_ln_scan(const VgxLnLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_flow_count(const VgxFlowLaunch *a, hipStream_t s);   // vgx_flows.hip: a->form is the form that runs (dense or split)
// the launchers of vgx_tau_prevalence.hip that vgx_tau_susceptible.hip and the frame of the tau replays (vgx_tau_replay.h) share
// (the 64-bit running sums, the narrowing min/max pass)
struct VgxTauPrevLaunch;
extern "C" hipError_t vgxi_tau_prev_count(const VgxTauPrevLaunch *a, hipStream_t s);   // (vgx_tau_milestones.hip: pass A over tile edges)
extern "C" hipError_t vgxi_tau_prev_scan(const VgxTauPrevLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_tau_prev_minmax(int64_t total, const int64_t *src, int32_t *dst, uint64_t *mm, hipStream_t s);
// vgx_tau_flows.hip: the weighted-row count (a->form is the form that runs)
struct VgxTauFlowLaunch;
extern "C" hipError_t vgxi_tau_flow_count(const VgxTauFlowLaunch *a, hipStream_t s);
// the column summary of vgx_colsummary.hip on a device int32 matrix x[R][N] of values in [0, 2^31) (a refusal's message goes to errbuf)
extern "C" int vgxi_column_summary_i32(const char *what, const int32_t *x, int64_t R, int64_t N, vgx_traj_summary_io *io, hipStream_t stream,
                                       char *errbuf, int64_t errcap);
extern "C" hipError_t vgxi_launch_counts32(const int64_t *c64, int32_t *c32, int64_t n, hipStream_t stream);
extern "C" hipError_t vgxi_launch_init_reps(const VgxDevRep *r, int P, int S, int64_t R, const int32_t *s_nocc,
                                            const int32_t *s_hap, const int32_t *s_cls, const int64_t *s_cnt,
                                            int64_t s_cap, const int64_t *s_sus, const double *s_cd,
                                            const int64_t *s_tot, hipStream_t stream);
extern "C" hipError_t vgxi_launch_init_reps_sets(const VgxDevRep *r, int P, int64_t R, const VgxDevParams *psets, const int32_t *set_of,
                                                 hipStream_t stream);

#define TAU_DECL(name) extern "C" hipError_t vgxi_##name(const VgxTauArgs *a, hipStream_t s);
TAU_DECL(tau_eff) TAU_DECL(tau_scatter) TAU_DECL(tau_prep) TAU_DECL(tau_drift) TAU_DECL(tau_choose) TAU_DECL(tau_draw)
TAU_DECL(tau_conv8) TAU_DECL(tau_sync8) TAU_DECL(tau_arrivals) TAU_DECL(tau_verdict) TAU_DECL(tau_apply) TAU_DECL(tau_check) TAU_DECL(tau_decide) TAU_DECL(tau_commit) TAU_DECL(tau_finish) TAU_DECL(tau_draw_big) TAU_DECL(tau_suspect)
extern "C" hipError_t vgxi_tau_traj(const VgxTauArgs *a, int64_t rep0, int64_t n, int fill, hipStream_t s);

// vgx_direct_plan.kernel
enum { VGX_K_WAVE = 1, VGX_K_LANES = 2, VGX_K_QUAD = 3, VGX_K_QUADG = 4, VGX_K_SOLO = 5, VGX_K_LONE = 6, VGX_K_QUADF = 7 };

struct HostState {
    std::vector<int64_t> susceptible, infectious, initial_susceptible, initial_infectious;
    std::vector<int64_t> totalSusceptible, totalInfectious, lockdownON;
    std::vector<double> contactDensity;
    int64_t first_simulation = 0, globalInfectious = 0;
    int64_t bCounter = 0, dCounter = 0, sCounter = 0, mCounter = 0, iCounter = 0, swapLockdown = 0, migPlus = 0,
            migNonPlus = 0, good_attempt = 0;
    double currentTime = 0, totalRate = 0, totalMigrationRate = 0, tau_l = 0.01;
    int64_t ev_ptr = 0, ev_size = 0;
};

// What the start of a tau call reads of one parameter set on the host (the engine's h_class_pos, suscepCumul, h_mut_uniform and
// h_mutp hold set 0's): filled for every set by vgx_set_param_sets
struct TauSetTables {
    std::vector<int32_t> cls;            // [H] rate class of a haplotype
    std::vector<char> class_pos;         // [C] the class has a positive recovery, sampling, mutation or transmission rate
    std::vector<double> suscepCumul;     // [S]
    bool mut_uniform = false;
    double mutp[16][3] = {};             // mRate[s] * w[s][i] / (w[s][0] + w[s][1] + w[s][2]) of haplotype 0's rows
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct vgx_engine {
    vgx_dims d{};
    int64_t R = 1;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    bool have_params = false, have_state = false, dev_state_valid = false;
    bool call_philox = false;      // the last direct call drew from the counter-based stream (the host clock must too)
    int64_t start_max_nocc = 0;    // longest occupancy list of the state last uploaded
    int64_t start_lone_rows = 0;   // heap rows of vgx_lone.hip that state (and the Restart snapshot) needs at least
    void *pin[2] = {nullptr, nullptr};   // pinned staging buffers of large uploads (VGX_PIN_BYTES each), allocated on first use
    void *pin_tl = nullptr;               // pinned staging of vgx_get_timelines (packed iteration and rate logs), kept between calls
    size_t pin_tl_bytes = 0;
    void *pin_tau = nullptr;              // pinned mirror of what the tau step loop reads after every try and step (flags, the finish kernel's record)
    size_t pin_tau_bytes = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool counts32_valid = false;   // r_lcnt32 mirrors r_lcnt (vgx_quad.hip keeps it; other kernels do not)
    bool counts64_valid = true;    // r_lcnt is current (vgx_quadf.hip and the long-list kernel of vgx_quad.hip keep the 4-byte counts only)
    int C = 0, CB = 0;
    // host copies of what the host needs again
    std::vector<int32_t> cls;
    std::vector<int64_t> sizes, seeds;
    std::vector<double> suscepCumul, mig, actualSizes;
    std::vector<char> h_class_pos;       // [C] the class has a positive recovery, sampling, mutation or transmission rate
    HostState hs;
    // device
    std::vector<DevBuf *> all;
    DevBuf p_cls, p_suscType, p_mRate, p_hapMutType, p_bRate, p_susc, p_cd, p_cs, p_ctm, p_cbidx, p_cstype, p_cbb, p_cbsig,
        p_sizes, p_cdBefore, p_cdAfter, p_startLD, p_endLD, p_sampMult, p_actualSizes, p_mig, p_suscTrans,
        p_suscCumul, p_sitesPos;
    // scenario ensembles (vgx_set_param_sets): n_sets parameter sets, replicate r runs under set set_of[r].  1: none installed
    // (vgx_set_params).  Everything above is set 0's then; the wavefront kernel reads block set_of[r] of ps_blocks instead.
    int64_t n_sets = 1;
    int sets_C = 0, sets_CB = 0;         // largest C and CB over the sets
    std::vector<double> sets_startLD;    // [n_sets][P]
    std::vector<VgxDevParams> h_psets;   // [n_sets] the blocks as uploaded: pointers into ps_blob
    DevBuf ps_blob, ps_blocks, ps_setof;
    std::vector<int32_t> h_setof;        // [R] the map as installed
    std::vector<TauSetTables> h_sets;    // [n_sets] what the start of a tau call reads of every set (vgx_tau_run.hip)
    DevBuf ps_taurec;                    // [n_sets] VgxTausSetRec of the last tau call
    int max_C() const { return n_sets > 1 ? sets_C : C; }
    int max_CB() const { return n_sets > 1 ? sets_CB : CB; }
    double recombination = 0.0;          // pyx:93, 1422-1426
    int64_t genome_length = 1000000, rec_cap = 0;
    DevBuf r_rec;
    DevBuf r_popD, r_popI, r_sus, r_immSrc, r_birthC, r_xC, r_effMig, r_nocc, r_lhap, r_lcls, r_lcnt, r_lcnt32, r_ltsum, r_lanews, r_sc, r_seeds,
        r_evrate, r_evcols, r_locrec, r_loctime, r_lociter, r_farate, r_fakey, r_traj, r_prof, r_qeff, r_qmebm, r_qflag;
    // tau-leaping (dense compartments)
    DevBuf t_I, t_S, t_dChk, t_dApp, t_dSi, t_dTot, t_totInf, t_gI, t_cd, t_lock, t_F, t_eff, t_Aeff, t_Gout, t_dS,
        t_taubits, t_tau, t_time, t_flags, t_counters, t_cnttry, t_cntpop, t_front, t_frontn, t_occ, t_occn, t_occpop, t_tIpt, t_d8spk, t_d8sbc, t_d8stile, t_d8sovf, t_d8smax, t_mev, t_mevn, t_mevbase, t_locn, t_mutcum, t_migcdf, t_migIn, t_mutHi, t_colT, t_colTW, t_inc, t_incn, t_sieve, t_sievepop, t_sieveskip, t_big, t_bign, t_res, t_susp, t_suspn, t_stkey, t_stval, t_dChkTot, t_q, t_qn, t_hist, t_I8, t_dSpart, t_tmax8, t_iI, t_iS, t_slog, t_sres, t_trajpre, t_trajn;
    std::vector<int64_t> tau_sieve_skipped;   // [R] tries left out by the sieve in the last tau call
    bool last_was_tau = false;
    bool tau_staged = false;              // vgx_stage_tau put the current start state on the device in the tau kernels' layout
    int64_t tau_occupied = 0;             // ... and counted its occupied compartments
    bool direct_logs_valid = false;   // the rate / iteration logs of the last direct call are on the device (host_clock can run)
    int64_t tau_mev_cap = 0;
    struct TauStep { double time; int64_t m0, m1; int32_t tries; };   // tries: rejected tries of the step's halving loop (pyx:2316-2321)
    std::vector<std::vector<TauStep>> tau_log;      // [R] MULTITYPE records of the last tau call
    std::vector<std::vector<double>> tau_loc_time;  // [R] lockdown log of the last tau call
    std::vector<std::vector<int64_t>> tau_loc_state, tau_loc_pop;
    std::vector<int64_t> tau_ev_ptr0;
    std::vector<VgxRepScalars> tau_sc;
    std::vector<double> h_startLD, h_endLD, h_cdBefore, h_cdAfter;
    bool h_has_mig = false, h_mut_uniform = false, h_mig_uniform = false;
    double h_mig_b = 0.0, h_mig_d = 1.0;
    double h_mutp[16][3] = {}, h_mut_total = 0.0;
    DevBuf i_nocc, i_hap, i_cls, i_cnt, i_sus;          // initial state (Restart)
    DevBuf s_nocc, s_hap, s_cls, s_cnt, s_sus, s_cd, s_tot;  // state at the start of the call
    VgxDevParams dp{};
    VgxDevRep dr{};
    int64_t cap = 0, evcap = 0, ev_base = 0, ev_ptr0 = 0, traj_points = 0;
    std::vector<int64_t> call_ev0;        // [R] events.ptr of every replicate at the start of the last call (they differ once replicates of a
                                          // continued ensemble stopped at different places)
    // host clock of the last direct call (host_clock below)
    int64_t loc_cap = 1, fa_cap = 0;
    bool call_recorded = false, call_has_tlimit = false;
    double call_tlimit = 0.0;
    std::vector<double> call_t0;          // [R] currentTime at the start of the call
    struct HostClock {
        int64_t rep = -1, e0 = 0;         // replicate; first event index of the reconstructed range
        bool exact = false;               // false: no rate log (record_events = 0), device clock reported
        std::vector<double> times;        // [ev_ptr - e0] event times
        double final_time = 0.0;          // currentTime after the call
        std::vector<double> loc_times;    // lockdown records
        bool limit_mismatch = false;      // device and host clock disagreed on a time-limit stop (see host_clock)
    } hc;
    int64_t clock_mismatches = 0;
    int64_t last_kernel = VGX_K_WAVE;   // vgx_direct_plan.kernel of the last direct call
    // BirthRate program of the general row kernel (vgx_quadg.h)
    std::vector<int32_t> h_seg_par, h_seg_sn, h_cb_seg;
    std::vector<double> h_seg_sig;
    DevBuf q_segpar, q_segsn, q_segsig, q_cbseg, r_cold;
    // BirthRate segments of the single-trajectory kernel (vgx_solo.h): distinct (group, non-zero susceptibility) pairs by group
    std::vector<int32_t> h_so_sn, h_so_hapcls, h_so_nnz, h_so_tsn;
    std::vector<double> h_so_sig, h_so_tsig, h_so_clssig;
    int h_so_ncls = 0, h_so_maxnnz = 0;
    DevBuf so_sn, so_sig, so_rcp, so_hapcls, so_nnz, so_tsn, so_tsig, so_clssig, so_pass;
    std::vector<int32_t> h_so_pass;
    int h_so_npass0 = 0, h_so_npass1 = 0;
    int64_t lone_fallbacks = 0;       // calls that ran again on the row kernel because the LDS heap of vgx_lone.hip was full
    bool dev_clock_stale = false;     // the last direct call ran without the device clock (vgx_solo.hip, CLOCK = false): r_sc[].currentTime is the
                                      // time at that call's START; a continued call must take the host clock's final time instead
    int64_t last_ev_size = 0;
    std::vector<VgxRepScalars> sc_host;
    bool sc_host_valid = false;
    float last_ms = 0.f;
    int64_t last_launches = 0;
    size_t dev_bytes = 0;
};

#define HIPCHECK(e_, call)                                                                             \
    do {                                                                                               \
        hipError_t err__ = (call);                                                                     \
        if (err__ != hipSuccess) {                                                                     \
            (e_)->err = std::string(#call) + ": " + hipGetErrorString(err__);                          \
            return VGX_ERR_HIP;                                                                        \
        }                                                                                              \
    } while (0)

inline int fail(vgx_engine *e, int code, const std::string &msg) {
    e->err = msg;
    return code;
}

// Host-side loops over all compartments of a large state (2^28 at BASELINE config 4): f(first, last, part) on up to 16 threads
// (n items of `weight` elementary operations each; small jobs stay on the calling thread)
template <class F>
inline void for_parts(int64_t n, F f, int64_t weight = 1) {
    unsigned nt = (unsigned)std::min<int64_t>(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u), std::max<int64_t>(n, 1));
    if (n * weight < ((int64_t)1 << 22)) nt = 1;
    if (nt == 1) { f((int64_t)0, n, 0u); return; }
    std::vector<std::thread> th;
    const int64_t step = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const int64_t b = std::min<int64_t>(n, (int64_t)t * step), en = std::min<int64_t>(n, b + step);
        th.emplace_back([=]() { f(b, en, t); });
    }
    for (auto &x : th) x.join();
}

inline int ensure(vgx_engine *e, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 8;
    if (b.bytes >= bytes) return VGX_OK;
    if (b.p) {
        HIPCHECK(e, hipFree(b.p));
        e->dev_bytes -= b.bytes;
        b.p = nullptr;
        b.bytes = 0;
    }
    HIPCHECK(e, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    e->dev_bytes += bytes;
    if (std::find(e->all.begin(), e->all.end(), &b) == e->all.end()) e->all.push_back(&b);
    return VGX_OK;
}

template <typename T>
inline int upload(vgx_engine *e, DevBuf &b, const T *src, size_t n) {
    int rc = ensure(e, b, n * sizeof(T));
    if (rc) return rc;
    if (n) HIPCHECK(e, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
    return VGX_OK;
}

inline bool sites_ok16(const vgx_engine *e) { return e->d.sites <= 16; }

template <typename T>
inline int dl(vgx_engine *e, std::vector<T> &dst, const DevBuf &b, size_t n) {
    dst.resize(n);
    HIPCHECK(e, hipMemcpy(dst.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return VGX_OK;
}
template <typename T>
inline int ul(vgx_engine *e, const DevBuf &b, const std::vector<T> &src) {
    HIPCHECK(e, hipMemcpy(b.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return VGX_OK;
}

// PrepareParameters' first-call part (pyx:435-448) + FirstInfection (pyx:234-242) on the host state
inline void prepare_first(vgx_engine *e) {
    HostState &h = e->hs;
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
    if (!h.first_simulation) {
        if (h.globalInfectious == 0) {
            for (int64_t sn = 0; sn < S; sn++) {
                if (h.susceptible[(size_t)sn] == 0) continue;
                h.susceptible[(size_t)sn] -= 1;
                h.totalSusceptible[0] -= 1;
                h.infectious[0] += 1;
                h.totalInfectious[0] += 1;
                h.globalInfectious += 1;
                break;
            }
        }
        h.globalInfectious = 0;
        for_parts(P, [&](int64_t p0, int64_t p1, unsigned) {   // whole populations per thread
            for (int64_t pn = p0; pn < p1; pn++) {
                h.totalSusceptible[(size_t)pn] = 0;
                for (int64_t sn = 0; sn < S; sn++) {
                    h.initial_susceptible[(size_t)(pn * S + sn)] = h.susceptible[(size_t)(pn * S + sn)];
                    h.totalSusceptible[(size_t)pn] += h.susceptible[(size_t)(pn * S + sn)];
                }
                int64_t t = 0;
                for (int64_t hn = 0; hn < H; hn++) {
                    const int64_t v = h.infectious[(size_t)(pn * H + hn)];
                    h.initial_infectious[(size_t)(pn * H + hn)] = v;
                    t += v;
                }
                h.totalInfectious[(size_t)pn] = t;
            }
        }, H);
        for (int64_t pn = 0; pn < P; pn++) h.globalInfectious += h.totalInfectious[(size_t)pn];
        h.first_simulation = 1;
    }
}

// the direct Gillespie driver (vgx_direct_run.hip); the tau driver runs it with zero attempts for PrepareParameters
int direct_core(vgx_engine *e, int64_t iterations, int64_t sample_size, float time, int64_t attempts, const vgx_run_opts *opts);
// the clock of one replicate of the last direct call, rebuilt on the host into e->hc (vgx_api.hip); a continued call starts from it
int host_clock(vgx_engine *e, int64_t rep);
// The kernel of a direct call and what goes with it, from numbers alone: no engine, no HIP call, no environment.  Returns VGX_OK, or the
// code of a refused request with its message in err.
int vgx_choose_direct(const vgx_direct_shape *s, const vgx_run_opts *o, vgx_direct_plan *plan, std::string &err);

#pragma GCC visibility pop
