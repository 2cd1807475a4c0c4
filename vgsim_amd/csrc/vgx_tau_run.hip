// vgx_tau_run.hip — the host driver of the tau-leaping path: vgx_stage_tau and vgx_simulate_tau of include/vgx.h.
//
// SimulatePopulation_tau (pyx:2293-2346): the step loop runs on the host, the steps on the device (the kernels of vgx_tau.hip), or
// the whole loop on the device for small models (vgx_taus.hip).  No kernels here: a .hip file for the build's flags alone
// (-ffp-contract=off: the host forms of PrepareParameters and CheckLockdown keep the reference's operation order).
//
// vgx_simulate_tau is a sequence of stages over one TauRun, which owns everything a call keeps between them; the stages are its
// member functions, in the order the call runs them.
#include "vgx_engine.h"

#define VGX_PIN_BYTES ((int64_t)64 << 20)
#define TAU_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

// One replicate's compartments into the tau kernels' layout: 4 bytes per compartment (population sizes < 2^31, checked by the
// callers), susceptible counts and population totals.  Large states are converted chunk by chunk into two pinned staging buffers,
// the copy of one chunk overlapping the conversion of the next.
static int tau_upload_state(vgx_engine *e, int64_t r, const std::vector<int64_t> &inf, const std::vector<int64_t> &sus) {
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
    const int64_t n = P * H;
    std::vector<int64_t> tot((size_t)P, 0);
    for_parts(P, [&](int64_t p0, int64_t p1, unsigned) {   // whole populations per thread
        for (int64_t pn = p0; pn < p1; pn++) {
            int64_t t = 0;
            const int64_t *src = &inf[(size_t)(pn * H)];
            for (int64_t hn = 0; hn < H; hn++) t += src[hn];
            tot[(size_t)pn] = t;
        }
    }, H);
    int32_t *dst = (int32_t *)e->t_I.p + r * n;
    const int64_t chunk = VGX_PIN_BYTES / 4;
    if (n >= chunk) {
        for (int i = 0; i < 2; i++) {
            if (!e->pin[i]) HIPCHECK(e, hipHostMalloc(&e->pin[i], VGX_PIN_BYTES, hipHostMallocDefault));
            if (!e->pin_ev[i]) HIPCHECK(e, hipEventCreateWithFlags(&e->pin_ev[i], hipEventDisableTiming));
        }
        int k = 0;
        for (int64_t c0 = 0; c0 < n; c0 += chunk, k ^= 1) {
            const int64_t len = std::min<int64_t>(chunk, n - c0);
            if (c0 >= 2 * chunk) HIPCHECK(e, hipEventSynchronize(e->pin_ev[k]));   // the buffer's previous copy is through
            int32_t *buf = (int32_t *)e->pin[k];
            const int64_t *src = inf.data() + c0;
            for_parts(len, [&](int64_t b, int64_t en, unsigned) { for (int64_t i = b; i < en; i++) buf[i] = (int32_t)src[i]; });
            HIPCHECK(e, hipMemcpyAsync(dst + c0, buf, (size_t)len * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipEventRecord(e->pin_ev[k], e->stream));
        }
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    } else {
        std::vector<int32_t> inf32((size_t)n);
        for (int64_t i = 0; i < n; i++) inf32[(size_t)i] = (int32_t)inf[(size_t)i];
        HIPCHECK(e, hipMemcpy(dst, inf32.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    HIPCHECK(e, hipMemcpy((int64_t *)e->t_S.p + r * P * S, sus.data(), (size_t)(P * S) * 8, hipMemcpyHostToDevice));
    HIPCHECK(e, hipMemcpy((int64_t *)e->t_totInf.p + r * P, tot.data(), (size_t)P * 8, hipMemcpyHostToDevice));
    return VGX_OK;
}

static int64_t count_occupied(const vgx_engine *e) {
    const HostState &h = e->hs;
    int64_t part[16] = {0}, occupied = 0;
    for_parts(e->d.popNum * e->d.hapNum, [&](int64_t b, int64_t en, unsigned t) {
        int64_t n = 0;
        for (int64_t i = b; i < en; i++) n += h.infectious[(size_t)i] != 0;
        part[t] = n;
    });
    for (int t = 0; t < 16; t++) occupied += part[t];
    return occupied;
}

// Puts the state handed over by vgx_set_state on the device in the tau kernels' layout ahead of vgx_simulate_tau (which does it itself
// otherwise): the first-call snapshot of PrepareParameters (pyx:435-448), the count of occupied compartments, conversion and upload of
// the P x H counts of every replicate.  At BASELINE config 4 that is 2^28 compartments: about 0.1 s of host work and PCIe transfer
// that a caller who times the simulate call may want outside it.  Valid until the next vgx_set_state / vgx_set_params / simulate call.
extern "C" int vgx_stage_tau(vgx_engine *e) {
    if (!e) return VGX_ERR_ARG;
    if (!e->have_params || !e->have_state) return fail(e, VGX_ERR_ARG, "vgx_stage_tau: set params and state first");
    if (e->n_sets > 1) return fail(e, VGX_ERR_ARG, "vgx_stage_tau: several parameter sets are installed (vgx_set_param_sets): tau-leaping runs one set only");
    HIPCHECK(e, hipSetDevice(e->device));
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum, R = e->R;
    for (int64_t pn = 0; pn < P; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_stage_tau: population sizes must be below 2^31");
    prepare_first(e);
    e->tau_occupied = count_occupied(e);
    int rc = 0;
    rc |= ensure(e, e->t_I, (size_t)(R * P * H) * 4);
    rc |= ensure(e, e->t_S, (size_t)(R * P * S) * 8);
    rc |= ensure(e, e->t_totInf, (size_t)(R * P) * 8);
    if (rc) return rc;
    for (int64_t r = 0; r < R; r++) TAU_TRY(tau_upload_state(e, r, e->hs.infectious, e->hs.susceptible));
    e->tau_staged = true;
    return VGX_OK;
}

// The first `n` lockdown records and times of replicate `src` on the device onto the lockdown log of replicates [dst0, dst1)
static int read_lockdown_log(vgx_engine *e, int64_t src, int64_t n, std::vector<int32_t> &rec, std::vector<double> &tt) {
    if (n <= 0) return VGX_OK;
    rec.resize((size_t)n * 2);
    tt.resize((size_t)n);
    HIPCHECK(e, hipMemcpy(rec.data(), (int32_t *)e->r_locrec.p + src * VGX_LOC_CAP * 2, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHECK(e, hipMemcpy(tt.data(), (double *)e->r_loctime.p + src * VGX_LOC_CAP, (size_t)n * 8, hipMemcpyDeviceToHost));
    return VGX_OK;
}
static void append_lockdown_log(vgx_engine *e, int64_t r, int64_t n, const std::vector<int32_t> &rec, const std::vector<double> &tt) {
    for (int64_t i = 0; i < n; i++) {
        e->tau_loc_state[(size_t)r].push_back(rec[(size_t)(i * 2)]);
        e->tau_loc_pop[(size_t)r].push_back(rec[(size_t)(i * 2 + 1)]);
        e->tau_loc_time[(size_t)r].push_back(tt[(size_t)i]);
    }
}
static int drain_lockdown_log(vgx_engine *e, int64_t src, int64_t n, int64_t dst0, int64_t dst1) {
    std::vector<int32_t> rec;
    std::vector<double> tt;
    TAU_TRY(read_lockdown_log(e, src, n, rec, tt));
    for (int64_t r = dst0; r < dst1 && n > 0; r++) append_lockdown_log(e, r, n, rec, tt);
    return VGX_OK;
}

// CheckLockdown (pyx:698-710) for every population on the host: `total` infected per population against the thresholds; a switch
// changes `lock` and `cd` and is logged at time `stamp` for replicates [dst0, dst1).  Returns the number of switches.
template <typename L>
static int64_t host_check_lockdown(vgx_engine *e, const std::vector<int64_t> &total, std::vector<L> &lock, std::vector<double> &cd,
                                   double stamp, int64_t dst0, int64_t dst1) {
    int64_t flips = 0;
    for (int64_t pn = 0; pn < e->d.popNum; pn++) {
        for (int pass = 0; pass < 2; pass++) {
            const double ti = (double)total[(size_t)pn], sz = (double)e->sizes[(size_t)pn];
            const bool flip = pass == 0 ? (ti > e->h_startLD[(size_t)pn] * sz && lock[(size_t)pn] == 0)
                                        : (ti < e->h_endLD[(size_t)pn] * sz && lock[(size_t)pn] == 1);
            if (!flip) continue;
            cd[(size_t)pn] = pass == 0 ? e->h_cdAfter[(size_t)pn] : e->h_cdBefore[(size_t)pn];
            lock[(size_t)pn] = pass == 0 ? 1 : 0;
            flips += 1;
            for (int64_t r = dst0; r < dst1; r++) {
                e->tau_loc_state[(size_t)r].push_back(pass == 0 ? 1 : 0);
                e->tau_loc_pop[(size_t)r].push_back(pn);
                e->tau_loc_time[(size_t)r].push_back(stamp);
            }
        }
    }
    return flips;
}

// The shapes the on-device loop (vgx_taus.hip) can run at all: its compile-time limits and the LDS of one workgroup
static bool taus_shape_ok(const vgx_engine *e, bool sparse_default) {
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
    return P * H <= VGX_TAUS_MAX_CELLS && P <= VGX_TAUS_MAX_P && S <= VGX_TAUS_MAX_S && e->d.sites <= 15 && sparse_default &&
           e->max_C() <= VGX_TAUS_MAX_C && e->max_CB() <= VGX_TAUS_MAX_CB && vgx_taus_lds_bytes(P, H, S, e->max_C(), e->max_CB()) <= 150 * 1024;
}

static int halving_guard(vgx_engine *e, int tries) {
    return tries > 600 ? fail(e, VGX_ERR_LOOP_GUARD, "vgx_simulate_tau: tau halving did not converge") : VGX_OK;
}

// Everything one vgx_simulate_tau call keeps between its stages, and the stages in the order the call runs them
struct __attribute__((visibility("hidden"))) TauRun {
    // what the entry point hands over
    vgx_engine *const e;
    HostState &h;
    const int64_t H, P, S, R, iterations, sample_size, attempts;
    const float time;
    const bool has_tl;
    const int64_t ev_ptr_start, ev_size;
    vgx_run_opts o{};
    // VGX_TIMING=1: host-side phases of the call on stderr (diagnostics)
    const bool timing = getenv("VGX_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    // the start state (staged: vgx_stage_tau already did the snapshot, the count and the upload of this start state)
    bool staged = false, start_ok = false, rates_nonzero_initial = false;
    int64_t occupied = 0;
    // several parameter sets (vgx_set_param_sets; the on-device loop only): what the preparation found per set and per replicate
    const bool sets = e->n_sets > 1;
    std::vector<int32_t> set_start_ok, set_rates_nonzero_initial;   // [n_sets]
    std::vector<int64_t> set_swaps;                                 // [n_sets] swapLockdown after the preparation
    std::vector<double> rep_cd, rep_total_rate, rep_total_mig;      // [R][P], [R], [R]
    std::vector<int32_t> rep_lock;                                  // [R][P]
    // the workspace: capacities (the growable ones: inc_cap, big_cap, q_scap, mev_cap) and what they were sized from
    int64_t mev_max = 0, mev_cap = 0, Ppad = 0, q_shards = 0, q_shard_max = 0, q_scap = 0, big_cap = 0, suspect_cap = 0, st_size = 64, inc_cap = 0;
    bool sparse_default = true, dense_ready = false;
    VgxTauArgs a{};
    const int32_t *pin_flags = nullptr;    // the host's view of VgxTauArgs.host_flags / host_res
    const int64_t *pin_res = nullptr;
    // per-replicate host bookkeeping
    std::vector<double> tnow, tau_h;
    std::vector<int64_t> ev_ptr, att, good, gI, base_cnt, cnt, restarts, steps_done, swaps_kept;
    std::vector<std::vector<int64_t>> cnt0;   // counters before this call / after a restart
    std::vector<int32_t> running, finished, step_h, att32, acc_h, fresh;   // fresh: attempt just opened, the pyx:2311 guard applies
    std::vector<unsigned long long> mevn, susp_h;
    std::vector<int32_t> dev_active, dev_step, dev_att;   // what the device holds (empty: nothing uploaded yet)
    std::vector<double> dev_time;
    // adaptive state of the step-kernel loop
    bool occ_lists_ok = false, dense_drift = false, front_split = false, spec_adapt = true, spec_rounds = false;
    int sparse_ban = 0, sparse_ban_len = 32, spec_k = 6;   // steps for which the drift pass stays dense; the next such span; front passes per round
    int64_t occ_est = 0, slog_cap = 1;
    bool front_done = false, dense_once = false;   // dense_once: the last try asked for dense delta arrays
    bool i8_dirty = true;      // I8 does not mirror I (start of the call, after a Restart's upload, after a dense try)
    // counters
    float ms_total = 0.f;
    int64_t launches = 0, host_syncs = 0, tries_total = 0, tries_lists = 0;

    void lap(const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "vgx_simulate_tau: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }

    // records of accepted steps a replicate can write in this call (a Restart rewinds the log to 0)
    int64_t step_log_rows() const {
        return std::max<int64_t>(ev_size - ((ev_ptr_start <= 100 && iterations > 100) ? 0 : ev_ptr_start), 1);
    }

    // Several parameter sets (vgx_set_param_sets) run on the on-device loop of vgx_taus.hip alone, whatever the ensemble's size: the
    // step kernels take one set.  A call that loop would not run is refused before anything is prepared.
    int check_sets() {
        const std::string who = "vgx_simulate_tau: " + std::to_string(e->n_sets) + " parameter sets are installed (vgx_set_param_sets), which run "
                                "on the on-device step loop only: ";
        auto over = [&](const char *what, int64_t v, int64_t limit) {
            return fail(e, VGX_ERR_ARG, who + what + " = " + std::to_string(v) + " is above the loop's limit of " + std::to_string(limit));
        };
        if (P * H > VGX_TAUS_MAX_CELLS) return over("popNum x hapNum", P * H, VGX_TAUS_MAX_CELLS);
        if (P > VGX_TAUS_MAX_P) return over("popNum", P, VGX_TAUS_MAX_P);
        if (S > VGX_TAUS_MAX_S) return over("susNum", S, VGX_TAUS_MAX_S);
        if (e->d.sites > 15) return over("sites", e->d.sites, 15);
        if (e->max_C() > VGX_TAUS_MAX_C) return over("the rate classes of the largest set", e->max_C(), VGX_TAUS_MAX_C);
        if (e->max_CB() > VGX_TAUS_MAX_CB) return over("the transmission classes of the largest set", e->max_CB(), VGX_TAUS_MAX_CB);
        const int64_t lds = (int64_t)vgx_taus_lds_bytes(P, H, S, e->max_C(), e->max_CB());
        if (lds > 150 * 1024) return over("the LDS bytes of a replicate", lds, 150 * 1024);
        if (o.reserved[1] == 1 || o.reserved[1] == 2)
            return fail(e, VGX_ERR_ARG, who + "vgx_run_opts.reserved[1] = " + std::to_string(o.reserved[1]) + " asks for a validation mode of the step kernels");
        const char *fs = getenv("VGX_TAU_STEP_KERNELS"), *th = getenv("VGX_TAU_LARGE_MODEL_THRESHOLDS");
        if (fs && fs[0] == '1') return fail(e, VGX_ERR_ARG, who + "VGX_TAU_STEP_KERNELS=1 asks for the step kernels");
        if (th && th[0] == '1') return fail(e, VGX_ERR_ARG, who + "VGX_TAU_LARGE_MODEL_THRESHOLDS=1 asks for the step kernels");
        const int64_t rows = step_log_rows();
        if ((double)R * (double)rows * 24.0 > 8e9)
            return fail(e, VGX_ERR_ARG, who + "the step log of " + std::to_string(R) + " replicates x " + std::to_string(rows) +
                                            " steps x 24 bytes is above the loop's limit of 8000000000 bytes");
        return VGX_OK;
    }

    // PrepareParameters (pyx:2298): first-call snapshot on the host, then CheckLockdown for every population and
    // UpdateAllRates.  The tau steps never read the direct path's rate caches; what the driver needs from
    // UpdateAllRates is only whether totalRate + totalMigrationRate is non-zero (pyx:2311).  For moderately
    // occupied states the direct kernel does that preparation exactly (run with zero attempts); for densely
    // occupied large states (its exact, lane-ordered row sums would take seconds) the lockdown switches and the
    // non-zero test are done on the host and totalRate is reported as NaN (the reference leaves a stale value).
    int prepare_start() {
        e->dev_state_valid = false;
        e->tau_loc_time.assign((size_t)R, {});
        e->tau_loc_state.assign((size_t)R, {});
        e->tau_loc_pop.assign((size_t)R, {});
        staged = e->tau_staged;
        e->tau_staged = false;                 // (the device copy stops being the start state as soon as a step is applied)
        if (!staged) prepare_first(e);
        lap("first-call snapshot");
        occupied = staged ? e->tau_occupied : count_occupied(e);
        lap("count of occupied");
        bool rates_nonzero = false;
        // (the device's UpdateAllRates for the start state — exact totalRate, lockdown switches — where building the direct kernels' occupancy
        // lists from the dense host arrays is cheap: at config 4's size that scan of 2.7e8 compartments is 0.3 s per call, and the host form
        // below — what a densely occupied state takes anyway — stands in)
        if (sets) {
            TAU_TRY(prepare_start_sets());
            rates_nonzero = set_start_ok[(size_t)e->h_setof[0]] != 0;
        } else if (occupied <= ((int64_t)1 << 18) && P * H <= ((int64_t)1 << 24)) {
            vgx_run_opts po{};
            po.record_events = 0;
            TAU_TRY(direct_core(e, 0, -1, -1.0f, 0, &po));
            const VgxRepScalars prep = e->sc_host[0];
            std::vector<double> popD((size_t)(PD_COUNT * P));
            std::vector<int64_t> popI((size_t)(PI_COUNT * P));
            HIPCHECK(e, hipMemcpy(popD.data(), e->r_popD.p, popD.size() * 8, hipMemcpyDeviceToHost));
            HIPCHECK(e, hipMemcpy(popI.data(), e->r_popI.p, popI.size() * 8, hipMemcpyDeviceToHost));
            for (int64_t pn = 0; pn < P; pn++) {
                h.contactDensity[(size_t)pn] = popD[(size_t)(PD_CD * P + pn)];
                h.lockdownON[(size_t)pn] = popI[(size_t)(PI_LOCK * P + pn)];
            }
            h.swapLockdown = prep.swapLockdown;
            h.totalRate = prep.totalRate;
            h.totalMigrationRate = prep.totalMig;
            rates_nonzero = prep.totalRate + prep.totalMig != 0.0;
            // (replicate 0's records of the preparation, for every replicate: they all start from the one state)
            TAU_TRY(drain_lockdown_log(e, 0, std::min<int64_t>(prep.loc_n, e->loc_cap), 0, R));
        } else {
            h.swapLockdown += host_check_lockdown(e, h.totalInfectious, h.lockdownON, h.contactDensity, h.currentTime, 0, R);
            rates_nonzero = h.globalInfectious != 0;   // an infected host always has a positive total event rate unless every rate is 0
            for (int64_t pn = 0; pn < P && !rates_nonzero; pn++)
                for (int64_t sn = 0; sn < S; sn++)
                    if (e->suscepCumul[(size_t)sn] * (double)h.susceptible[(size_t)(pn * S + sn)] != 0.0) rates_nonzero = true;
            h.totalRate = std::nan("");
            h.totalMigrationRate = std::nan("");
        }
        e->dev_state_valid = false;  // the occupancy lists are not maintained by the tau path
        for (int64_t pn = 0; pn < P; pn++)
            if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_simulate_tau: population sizes must be below 2^31");
        if (e->C > 256 && (e->CB > 16 || S > 64)) return fail(e, VGX_ERR_CLASSES, "vgx_simulate_tau: more than 16 transmission classes together with more than 256 rate classes is not supported");
        start_ok = rates_nonzero && h.globalInfectious != 0;
        // the same guard for the state a Restart restores: does an infected host of the initial state have any event rate?
        rates_nonzero_initial = initial_rates_nonzero(e->cls, e->h_class_pos, e->suscepCumul);
        for (int64_t g = 0; sets && g < e->n_sets; g++) {
            const TauSetTables &t = e->h_sets[(size_t)g];
            set_rates_nonzero_initial[(size_t)g] = initial_rates_nonzero(t.cls, t.class_pos, t.suscepCumul) ? 1 : 0;
        }
        lap("PrepareParameters");
        return VGX_OK;
    }

    // pyx:2311 on the state a Restart restores, under one set's class tables and suscepCumul
    bool initial_rates_nonzero(const std::vector<int32_t> &cls, const std::vector<char> &class_pos, const std::vector<double> &cumul) const {
        bool nonzero = false;
        for (int64_t pn = 0; pn < P && !nonzero; pn++) {
            for (int64_t hn = 0; hn < H && !nonzero; hn++) {
                if (h.initial_infectious[(size_t)(pn * H + hn)] == 0) continue;
                // any positive recovery / sampling / mutation / transmission rate of the haplotype's class makes tEventHapPopRate,
                // hence totalRate, non-zero (transmission additionally needs a susceptible host; a model without the other
                // three rates and without susceptibles has nothing left to simulate either way)
                if (class_pos[(size_t)cls[(size_t)hn]]) nonzero = true;
            }
            for (int64_t sn = 0; sn < S; sn++)
                if (cumul[(size_t)sn] * (double)h.initial_susceptible[(size_t)(pn * S + sn)] != 0.0) nonzero = true;
        }
        return nonzero;
    }

    // The preparation under several parameter sets: the same launch (the scenario form of the wavefront kernel, zero attempts) prepares
    // every replicate under its own set.  Replicates of one set start from one state under one set of parameters and draw nothing, so
    // they find the same: the first replicate of a set stands for the set (start_ok, swapLockdown, the lockdown records), and every
    // replicate's contact densities and lockdown states are read from its own block.
    int prepare_start_sets() {
        const int64_t G = e->n_sets;
        vgx_run_opts po{};
        po.record_events = 0;
        TAU_TRY(direct_core(e, 0, -1, -1.0f, 0, &po));
        std::vector<double> popD((size_t)(R * PD_COUNT * P));
        std::vector<int64_t> popI((size_t)(R * PI_COUNT * P));
        HIPCHECK(e, hipMemcpy(popD.data(), e->r_popD.p, popD.size() * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(popI.data(), e->r_popI.p, popI.size() * 8, hipMemcpyDeviceToHost));
        rep_cd.resize((size_t)(R * P)); rep_lock.resize((size_t)(R * P));
        rep_total_rate.resize((size_t)R); rep_total_mig.resize((size_t)R);
        for (int64_t r = 0; r < R; r++) {
            for (int64_t pn = 0; pn < P; pn++) {
                rep_cd[(size_t)(r * P + pn)] = popD[(size_t)((r * PD_COUNT + PD_CD) * P + pn)];
                rep_lock[(size_t)(r * P + pn)] = (int32_t)popI[(size_t)((r * PI_COUNT + PI_LOCK) * P + pn)];
            }
            rep_total_rate[(size_t)r] = e->sc_host[(size_t)r].totalRate;
            rep_total_mig[(size_t)r] = e->sc_host[(size_t)r].totalMig;
        }
        set_start_ok.assign((size_t)G, 0); set_swaps.assign((size_t)G, 0); set_rates_nonzero_initial.assign((size_t)G, 0);
        std::vector<int64_t> first((size_t)G, -1);
        for (int64_t r = R - 1; r >= 0; r--) first[(size_t)e->h_setof[(size_t)r]] = r;
        std::vector<int32_t> rec;
        std::vector<double> tt;
        for (int64_t g = 0; g < G; g++) {
            const int64_t r0 = first[(size_t)g];
            if (r0 < 0) continue;      // (a set without replicates)
            const VgxRepScalars &prep = e->sc_host[(size_t)r0];
            set_start_ok[(size_t)g] = (prep.totalRate + prep.totalMig != 0.0 && h.globalInfectious != 0) ? 1 : 0;
            set_swaps[(size_t)g] = prep.swapLockdown;
            const int64_t n = std::min<int64_t>(prep.loc_n, e->loc_cap);
            TAU_TRY(read_lockdown_log(e, r0, n, rec, tt));
            for (int64_t r = r0; r < R; r++)
                if (e->h_setof[(size_t)r] == g) append_lockdown_log(e, r, n, rec, tt);
        }
        // (the host's one copy of the state: replicate 0's, as a call under one set leaves it)
        for (int64_t pn = 0; pn < P; pn++) {
            h.contactDensity[(size_t)pn] = rep_cd[(size_t)pn];
            h.lockdownON[(size_t)pn] = rep_lock[(size_t)pn];
        }
        h.swapLockdown = e->sc_host[0].swapLockdown;
        h.totalRate = rep_total_rate[0];
        h.totalMigrationRate = rep_total_mig[0];
        return VGX_OK;
    }

    int ensure_dense() {
        if (dense_ready) return 0;
        int r2 = ensure(e, e->t_dChk, (size_t)(R * P * H) * 4) | ensure(e, e->t_dApp, (size_t)(R * P * H) * 4);
        dense_ready = r2 == 0;
        return r2;
    }

    // The device arrays of the call, their clears (on the null stream) and the upload of the start state
    int alloc_workspace() {
        // multievent rows (num > 0 only): at most a few per occupied compartment and step; sized from the start state with
        // room for the epidemic to grow, within 2^27 rows (6 GiB) per replicate; a run that still outgrows it fails loudly
        const int64_t rows_per_step = 16 * occupied + 4 * P * S * S + 4096;
        mev_max = ((int64_t)1 << 28) / std::max<int64_t>(R, 1);   // 12 GiB of rows over all replicates
        mev_cap = o.record_events
            ? std::max<int64_t>(1, std::min<int64_t>(mev_max / 2,
                                                     std::max<int64_t>((int64_t)1 << 22, std::min<int64_t>(iterations, 1 << 20) * rows_per_step)))
            : 0;   // doubled on demand (a try whose rows do not fit is run again), up to mev_max
        const size_t nF = 11;  // int32 flag arrays
        Ppad = (P + 31) / 32 * 32;
        int rc = 0;
        rc |= ensure(e, e->r_locrec, (size_t)(R * VGX_LOC_CAP * 2) * 4);
        rc |= ensure(e, e->r_loctime, (size_t)(R * VGX_LOC_CAP) * 8);
        rc |= ensure(e, e->t_I, (size_t)(R * P * H) * 4);
        rc |= ensure(e, e->t_S, (size_t)(R * P * S) * 8);
        rc |= ensure(e, e->t_I8, (size_t)(R * P * H) + 64);
        // mode of the tries: sparse (no dense delta arrays; the default), or dense with the fused checks (reserved[1] = 2), or
        // dense with the bounds check as a pass of its own (reserved[1] = 1); the dense arrays are allocated when first needed
        sparse_default = !(o.reserved[1] == 1 || o.reserved[1] == 2);
        if (!sparse_default) rc |= ensure_dense();
        rc |= ensure(e, e->t_dChkTot, (size_t)(R * P) * 8);
        // queue of the compartments that may draw events in a try: an eighth of the compartments to begin with, grown on demand
        q_shards = vgxi_tau_queue_shards(H, P); q_shard_max = vgxi_tau_queue_shard_max(H);
        q_scap = std::min<int64_t>(q_shard_max, std::max<int64_t>(256, q_shard_max / 8));
        rc |= ensure(e, e->t_q, (size_t)(R * q_shards * q_scap) * 8);
        rc |= ensure(e, e->t_qn, (size_t)(R * q_shards) * 8);
        rc |= ensure(e, e->t_dSi, (size_t)(R * P * S) * 8);
        rc |= ensure(e, e->t_dTot, (size_t)(R * P) * 8);
        rc |= ensure(e, e->t_totInf, (size_t)(R * P) * 8);
        rc |= ensure(e, e->t_gI, (size_t)R * 8);
        rc |= ensure(e, e->t_cd, (size_t)(R * P) * 8);
        rc |= ensure(e, e->t_lock, (size_t)(R * P) * 4);
        rc |= ensure(e, e->t_F, (size_t)(R * P) * 8);
        rc |= ensure(e, e->t_eff, (size_t)(R * P * P) * 8);
        rc |= ensure(e, e->t_Aeff, (size_t)(R * P * Ppad) * 8);
        rc |= ensure(e, e->t_Gout, (size_t)(R * P * e->CB) * 8);
        rc |= ensure(e, e->t_dS, (size_t)(R * P * S) * 8);
        rc |= ensure(e, e->t_taubits, (size_t)R * 8);
        rc |= ensure(e, e->t_tau, (size_t)R * 8);
        rc |= ensure(e, e->t_time, (size_t)R * 8);
        rc |= ensure(e, e->t_flags, (size_t)R * nF * 4);
        rc |= ensure(e, e->t_counters, (size_t)R * 8 * 8);
        big_cap = std::min<int64_t>(P * H, (int64_t)1 << 20);   // grown on demand
        rc |= ensure(e, e->t_big, (size_t)(R * big_cap) * 8);
        rc |= ensure(e, e->t_bign, (size_t)R * 8);
        rc |= ensure(e, e->t_res, (size_t)R * TR_WORDS * 8);
        suspect_cap = std::min<int64_t>(P * H, (int64_t)1 << 18);
        rc |= ensure(e, e->t_susp, (size_t)(R * suspect_cap * 2) * 8);
        while (st_size < 2 * suspect_cap) st_size *= 2;
        rc |= ensure(e, e->t_stkey, (size_t)(R * st_size) * 8);
        rc |= ensure(e, e->t_stval, (size_t)(R * st_size) * 8);
        rc |= ensure(e, e->t_suspn, (size_t)R * 8);
        rc |= ensure(e, e->t_sieve, (size_t)R * VGX_SIEVE_K * 8);
        rc |= ensure(e, e->t_sievepop, (size_t)(R * P) * VGX_SIEVE_K * 8);
        rc |= ensure(e, e->t_sieveskip, (size_t)R * 8);
        rc |= ensure(e, e->t_cnttry, (size_t)R * 8 * 8);
        rc |= ensure(e, e->t_cntpop, (size_t)(R * P) * 8 * 8);
        rc |= ensure(e, e->t_mev, (size_t)(R * std::max<int64_t>(mev_cap, 1) * 6) * 8);
        rc |= ensure(e, e->t_mevn, (size_t)R * 8);
        rc |= ensure(e, e->t_mevbase, (size_t)R * 8);
        rc |= ensure(e, e->t_locn, (size_t)R * 8);
        // summary trajectories [R][T][P][2] as the direct calls bin them (direct_core), the step kernels' copy of the totals before a step
        if (o.traj_points > 0) {
            rc |= ensure(e, e->r_traj, (size_t)(R * o.traj_points * P * 2) * 8);
            rc |= ensure(e, e->t_trajpre, (size_t)(R * P * 2) * 8);
            rc |= ensure(e, e->t_trajn, (size_t)R * 8);
        }
        if (e->h_has_mig && !e->h_mig_uniform) rc |= ensure(e, e->t_migIn, (size_t)(R * P * H) * 8);
        if (e->h_mig_uniform) { rc |= ensure(e, e->t_colT, (size_t)(R * H) * 8); rc |= ensure(e, e->t_colTW, (size_t)(R * H) * 8); }
        rc |= ensure(e, e->t_mutHi, (size_t)(e->d.sites > 6 ? R * P * H : 1) * 8);   // tiled drift, first pass (vgx_tau_muthigh_kernel)
        inc_cap = std::max<int64_t>((int64_t)1 << 22, P * H / 8) / VGX_INC_SHARDS * VGX_INC_SHARDS;   // grown on demand
        rc |= ensure(e, e->t_inc, (size_t)(R * inc_cap) * 8);
        rc |= ensure(e, e->t_incn, (size_t)R * VGX_INC_SHARDS * 8);
        rc |= ensure(e, e->t_migcdf, (size_t)(R * P * e->CB * P * S) * 8);
        {
            std::vector<double> cum;
            double acc = 0.0;
            for (int64_t s2 = 0; s2 < e->d.sites && s2 < 16; s2++)
                for (int i = 0; i < 3; i++) { acc += e->h_mutp[s2][i]; cum.push_back(acc); }
            if (cum.empty()) cum.push_back(0.0);
            rc |= upload(e, e->t_mutcum, cum.data(), cum.size());
        }
        rc |= upload(e, e->r_seeds, e->seeds.data(), e->seeds.size());
        if (rc) return VGX_ERR_HIP;
        lap("device allocations");
        HIPCHECK(e, hipMemset(e->t_incn.p, 0, (size_t)R * VGX_INC_SHARDS * 8));
        HIPCHECK(e, hipMemset(e->t_stkey.p, 0, (size_t)(R * st_size) * 8));   // try counter 0: every slot reads as empty
        HIPCHECK(e, hipMemset(e->t_dChkTot.p, 0, (size_t)(R * P) * 8));
        HIPCHECK(e, hipMemset(e->t_qn.p, 0, (size_t)(R * q_shards) * 8));
        HIPCHECK(e, hipMemset(e->t_dSi.p, 0, (size_t)(R * P * S) * 8));
        HIPCHECK(e, hipMemset(e->t_dTot.p, 0, (size_t)(R * P) * 8));
        HIPCHECK(e, hipMemset(e->t_counters.p, 0, (size_t)R * 64));
        HIPCHECK(e, hipMemset(e->t_bign.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_suspn.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_sieve.p, 0, (size_t)R * VGX_SIEVE_K * 8));
        HIPCHECK(e, hipMemset(e->t_sievepop.p, 0, (size_t)(R * P) * VGX_SIEVE_K * 8));
        HIPCHECK(e, hipMemset(e->t_sieveskip.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_cnttry.p, 0, (size_t)R * 64));
        HIPCHECK(e, hipMemset(e->t_cntpop.p, 0, (size_t)(R * P) * 64));
        HIPCHECK(e, hipMemset(e->t_mevn.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_mevbase.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_locn.p, 0, (size_t)R * 8));
        HIPCHECK(e, hipMemset(e->t_flags.p, 0, (size_t)R * nF * 4));
        std::vector<int32_t> lock32((size_t)P);
        for (int64_t pn = 0; pn < P; pn++) lock32[(size_t)pn] = (int32_t)h.lockdownON[(size_t)pn];
        for (int64_t r = 0; r < R; r++) {
            if (!staged) TAU_TRY(tau_upload_state(e, r, h.infectious, h.susceptible));
            if (sets) continue;
            HIPCHECK(e, hipMemcpy((double *)e->t_cd.p + r * P, h.contactDensity.data(), (size_t)P * 8, hipMemcpyHostToDevice));
            HIPCHECK(e, hipMemcpy((int32_t *)e->t_lock.p + r * P, lock32.data(), (size_t)P * 4, hipMemcpyHostToDevice));
        }
        if (sets) {    // every replicate's own, as its set's preparation left them
            HIPCHECK(e, hipMemcpy(e->t_cd.p, rep_cd.data(), (size_t)(R * P) * 8, hipMemcpyHostToDevice));
            HIPCHECK(e, hipMemcpy(e->t_lock.p, rep_lock.data(), (size_t)(R * P) * 4, hipMemcpyHostToDevice));
        }
        lap("memsets + state upload");
        return VGX_OK;
    }

    // VgxTauArgs: the workspace's pointers and the model's shape-dependent choices (with the buffers only those choices need)
    int fill_args() {
        a.p = e->dp;
        a.R = R;
        a.I = (int32_t *)e->t_I.p; a.I8 = (uint8_t *)e->t_I8.p; a.S = (int64_t *)e->t_S.p; a.dChk = (int32_t *)e->t_dChk.p; a.dApp = (int32_t *)e->t_dApp.p;
        a.dSi = (int64_t *)e->t_dSi.p; a.dTot = (int64_t *)e->t_dTot.p; a.totInf = (int64_t *)e->t_totInf.p;
        a.gI = (int64_t *)e->t_gI.p; a.cd = (double *)e->t_cd.p; a.lockON = (int32_t *)e->t_lock.p; a.F = (double *)e->t_F.p;
        a.effMig = (double *)e->t_eff.p; a.Aeff = (double *)e->t_Aeff.p; a.Gout = (double *)e->t_Gout.p;
        a.dS = (double *)e->t_dS.p; a.tau_bits = (unsigned long long *)e->t_taubits.p; a.tau = (double *)e->t_tau.p;
        a.time_now = (double *)e->t_time.p;
        int32_t *fl = (int32_t *)e->t_flags.p;
        a.active = fl; a.ok = fl + R; a.accepted = fl + 2 * R; a.grow = fl + 3 * R; a.retry = fl + 4 * R;   // accepted, grow: one copy per try
        // the host's pinned mirror of accepted / grow (written by the decide kernel) and of the finish kernel's record: read after a
        // stream synchronisation, no copy in between
        const size_t res_off = ((size_t)R * 3 * 4 + 63) & ~(size_t)63;
        const size_t need = (size_t)R * 3 * 4 + 64 + (size_t)R * TR_WORDS * 8;
        if (e->pin_tau_bytes < need) {
            if (e->pin_tau) (void)hipHostFree(e->pin_tau);
            e->pin_tau = nullptr; e->pin_tau_bytes = 0;
            HIPCHECK(e, hipHostMalloc(&e->pin_tau, need, hipHostMallocDefault));
            e->pin_tau_bytes = need;
        }
        memset(e->pin_tau, 0, need);
        void *dp = nullptr;
        HIPCHECK(e, hipHostGetDevicePointer(&dp, e->pin_tau, 0));
        a.host_flags = (int32_t *)dp;
        a.host_res = (int64_t *)((char *)dp + res_off);
        pin_flags = (const int32_t *)e->pin_tau;
        pin_res = (const int64_t *)((const char *)e->pin_tau + res_off);
        a.step = fl + 5 * R; a.error = fl + 6 * R; a.attempt = fl + 7 * R; a.eff_dirty = fl + 8 * R; a.deciding = fl + 9 * R;
        a.spec = fl + 10 * R; a.gate = 0;
        a.Ppad = (int32_t)Ppad;
        const std::vector<int32_t> ones((size_t)R, 1);
        HIPCHECK(e, hipMemcpy(a.eff_dirty, ones.data(), (size_t)R * 4, hipMemcpyHostToDevice));
        a.seeds = (const int64_t *)e->r_seeds.p;
        a.has_mig = e->h_has_mig ? 1 : 0;
        a.mut_uniform = (e->h_mut_uniform && sites_ok16(e)) ? 1 : 0;
        memcpy(a.mutp, e->h_mutp, sizeof(a.mutp));
        a.mut_total = e->h_mut_total;
        a.mutcum = (const double *)e->t_mutcum.p;
        a.migcdf = (double *)e->t_migcdf.p;
        a.migIn = (double *)e->t_migIn.p;
        a.mutHi = (double *)e->t_mutHi.p;
        {   // high sites (the first sites - 6) all with one rate and equally likely derived states?
            const int nh = (int)e->d.sites - 6;
            bool same = a.mut_uniform && nh > 0 && nh <= 4;
            for (int s2 = 0; s2 < nh && same; s2++)
                for (int i = 0; i < 3; i++)
                    if (e->h_mutp[s2][i] != e->h_mutp[0][0]) same = false;
            a.mutHi_int = same ? 1 : 0;
            a.mutHi_rate = same ? e->h_mutp[0][0] : 0.0;
        }
        a.mig_uniform = e->h_mig_uniform ? 1 : 0; a.mig_b = e->h_mig_b; a.mig_d = e->h_mig_d;
        a.colT = (double *)e->t_colT.p; a.colTW = (double *)e->t_colTW.p;
        a.inc = (int64_t *)e->t_inc.p; a.inc_cap = inc_cap; a.inc_shards = vgxi_tau_inc_shards(H, P); a.inc_n = (unsigned long long *)e->t_incn.p;
        a.counters = (int64_t *)e->t_counters.p; a.cnt_try = (int64_t *)e->t_cnttry.p; a.cnt_pop = (unsigned long long *)e->t_cntpop.p;
        // the front pass of a try (vgx_tau_front_kernel): the tabulated scan's shapes, sparse mode
        const char *nf = getenv("VGX_TAU_NO_FRONT");
        a.front_cap = 512;
        a.front_on = (sparse_default && e->C <= 16 && e->CB <= 16 && (H & 15) == 0 && !(nf && nf[0] == '1')) ? 1 : 0;
        TAU_TRY(ensure(e, e->t_front, (size_t)(R * P) * (size_t)a.front_cap * 8));
        TAU_TRY(ensure(e, e->t_frontn, (size_t)(R * P) * 4 + 64));
        HIPCHECK(e, hipMemset(e->t_frontn.p, 0, (size_t)(R * P) * 4));
        a.front = (int64_t *)e->t_front.p; a.front_n = (unsigned int *)e->t_frontn.p;
        a.big = (int64_t *)e->t_big.p; a.big_cap = big_cap; a.big_n = (unsigned long long *)e->t_bign.p;
        a.res = (int64_t *)e->t_res.p;
        a.suspect = (int64_t *)e->t_susp.p; a.suspect_cap = suspect_cap; a.suspect_n = (unsigned long long *)e->t_suspn.p;
        a.dense_check = o.reserved[1] == 1 ? 1 : 0;   // validation: the bounds check as one dense pass over all compartments
        a.sparse = sparse_default ? 1 : 0;
        a.gen = 0;
        a.st_key = (unsigned long long *)e->t_stkey.p; a.st_val = (long long *)e->t_stval.p; a.st_size = st_size;
        a.dChkTot = (int64_t *)e->t_dChkTot.p;
        a.q = (int64_t *)e->t_q.p; a.q_cap = q_shards * q_scap; a.q_shards = q_shards; a.q_n = (unsigned long long *)e->t_qn.p;
        // A compartment's events are drawn by ONE lane of the events kernel (a draw of their number, then one by one) up to this
        // mean, by a group of lanes of vgx_tau_draw_big_kernel (one Poisson draw per channel) from it on.  The lane's way is far
        // cheaper per compartment but its time grows with the mean, and the slowest lane holds its wavefront: with few
        // compartments (nothing else to overlap with) the switch comes earlier.  Same joint law either way.
        a.big_lam = P * H * R <= ((int64_t)1 << 18) ? VGX_TAU_BIG_SMALL : VGX_TAU_BIG;
        // tests: the thresholds of large models on a small one (so that its draws go through the one-draw-per-kind form)
        const char *th = getenv("VGX_TAU_LARGE_MODEL_THRESHOLDS");
        if (th && th[0] == '1') a.big_lam = VGX_TAU_BIG;
        // enough blocks of the events kernel to fill the chip whatever the number of shards (mid-size models have few)
        a.ev_split = (int32_t)std::max<int64_t>(1, std::min<int64_t>(q_shard_max / 64, 4096 / std::max<int64_t>(1, q_shards * R)));
        a.sieve = (double *)e->t_sieve.p; a.sieve_pop = (double *)e->t_sievepop.p; a.sieve_skipped = (int64_t *)e->t_sieveskip.p;
        // vgx_run_opts.reserved[0] = 1: run every try of the halving loop; with few compartments no try is ever a certain rejection
        a.sieve_on = (o.reserved[0] == 1 || P * H < 32768) ? 0 : 1;
        {   // low sites (the last min(sites, 6)): equally likely derived states at each of them?  one common rate?
            const int ns = (int)e->d.sites, low = ns < 6 ? ns : 6, nh = ns - low;
            bool flat = a.mut_uniform && low >= 2 && ns <= 10 && e->t_mutHi.p != nullptr && e->C <= 256 && e->CB <= 16, same = true;
            for (int s2 = nh; s2 < ns && flat; s2++) {
                if (e->h_mutp[s2][0] != e->h_mutp[s2][1] || e->h_mutp[s2][1] != e->h_mutp[s2][2]) flat = false;
                if (e->h_mutp[s2][0] != e->h_mutp[nh][0]) same = false;
            }
            // the fast drift kernel's inner loop loads its inputs unconditionally an iteration ahead: high-site sums as integers,
            // migration (if any) through the two column sums; the other forms take the general tiled kernel
            flat = flat && (nh == 0 || a.mutHi_int) && (!a.has_mig || a.mig_uniform);
            a.mutlow_fast = flat ? 1 : 0;
            a.mutlow_same = (flat && same) ? 1 : 0;
            // the drift pass on the one-byte counts (vgx_tau_drift8_kernel): the fast form's models from seven sites on with one
            // rate class and one rate for the low sites (VGX_TAU_NO_BYTE_DRIFT=1: the two-pass form, for comparisons)
            const char *nb8 = getenv("VGX_TAU_NO_BYTE_DRIFT");
            a.use8 = (flat && same && nh >= 1 && e->C == 1 && S <= 64 && !(nb8 && nb8[0] == '1')) ? 1 : 0;
            a.nt8 = ns > 8 ? 1 << (2 * (ns - 8)) : 1;
            TAU_TRY(ensure(e, e->t_tmax8, (size_t)(R * P * a.nt8) * 4 + 64));
            a.tmax8 = (unsigned int *)e->t_tmax8.p;
            if (a.use8) {   // lists of the occupied compartments for sparse states (vgx_tau_listscan_kernel), filled by the drift pass
                a.occ_nreg = a.nt8 * VGX_D8_WAVES;
                TAU_TRY(ensure(e, e->t_occ, (size_t)(R * P) * (size_t)a.occ_nreg * VGX_OCC_CAP * 4));
                TAU_TRY(ensure(e, e->t_occn, (size_t)(R * P) * (size_t)a.occ_nreg * 4 + 64));
                TAU_TRY(ensure(e, e->t_occpop, (size_t)(R * P) * 8 + 64));
                HIPCHECK(e, hipMemset(e->t_occpop.p, 0, (size_t)(R * P) * 8));
                a.occ = (int32_t *)e->t_occ.p; a.occ_n = (unsigned int *)e->t_occn.p; a.occ_pop = (unsigned long long *)e->t_occpop.p;
                // the drift pass over those lists (vgx_tau_drift8s_*)
                TAU_TRY(ensure(e, e->t_tIpt, (size_t)(R * P * a.nt8) * 8 + 64));
                TAU_TRY(ensure(e, e->t_d8spk, (size_t)(R * P) * 64 + 64));
                TAU_TRY(ensure(e, e->t_d8sbc, (size_t)R * 64 + 64));
                TAU_TRY(ensure(e, e->t_d8sovf, (size_t)(R * P) * (size_t)a.occ_nreg * 4 + 64));
                TAU_TRY(ensure(e, e->t_d8smax, (size_t)(R * P) * (size_t)a.occ_nreg * 4 + 64));
                TAU_TRY(ensure(e, e->t_d8stile, (size_t)(R * 2 * a.nt8) * 8 + 64));
                a.tI_pt = (unsigned long long *)e->t_tIpt.p; a.d8s_pk = (double *)e->t_d8spk.p; a.d8s_bc = (unsigned long long *)e->t_d8sbc.p;
                a.d8s_tile = (double *)e->t_d8stile.p; a.d8s_ovf = (int32_t *)e->t_d8sovf.p; a.d8s_regmax = (int32_t *)e->t_d8smax.p;
            }
            a.hist = nullptr;
            if (flat && a.sieve_on && e->C <= 8) {   // (VGX_HIST_CMAX classes x 64 sizes per population)
                TAU_TRY(ensure(e, e->t_hist, (size_t)(R * P * e->C * 64) * 4));
                HIPCHECK(e, hipMemset(e->t_hist.p, 0, (size_t)(R * P * e->C * 64) * 4));
                a.hist = (unsigned int *)e->t_hist.p;
            }
        }
        // the drift kernel's blocks write their parts of the susceptible drift into their own slots
        a.ds_nb = vgxi_tau_drift_blocks(&a);
        TAU_TRY(ensure(e, e->t_dSpart, (size_t)(R * P * a.ds_nb * S) * 8));
        a.dS_part = (double *)e->t_dSpart.p;
        a.mev = (int64_t *)e->t_mev.p; a.mev_cap = mev_cap;
        e->tau_mev_cap = mev_cap;
        a.mev_n = (unsigned long long *)e->t_mevn.p; a.mev_base = (unsigned long long *)e->t_mevbase.p;
        a.loc_n = (unsigned long long *)e->t_locn.p; a.loc_rec = (int32_t *)e->r_locrec.p; a.loc_time = (double *)e->r_loctime.p;
        if (o.traj_points > 0) {
            a.traj = (double *)e->r_traj.p; a.traj_points = o.traj_points; a.traj_t0 = o.traj_t0;
            a.traj_dt = o.traj_points > 1 ? (o.traj_t1 - o.traj_t0) / (double)(o.traj_points - 1) : 0.0;
            a.traj_pre = (double *)e->t_trajpre.p; a.traj_next = (int64_t *)e->t_trajn.p;
        }
        return VGX_OK;
    }

    // Per-replicate host bookkeeping at the start of the first attempt, and the switches of the step-kernel loop
    void open_bookkeeping() {
        tnow.assign((size_t)R, h.currentTime);
        ev_ptr.assign((size_t)R, ev_ptr_start); att.assign((size_t)R, 0); good.assign((size_t)R, h.good_attempt); gI.assign((size_t)R, h.globalInfectious);
        base_cnt = {h.bCounter, h.dCounter, h.sCounter, h.mCounter, h.iCounter, h.migPlus, h.swapLockdown, 0};
        cnt0.assign((size_t)R, base_cnt);
        cnt.assign((size_t)R * 8, 0);
        running.assign((size_t)R, (attempts > 0 && start_ok) ? 1 : 0); finished.assign((size_t)R, 0); step_h.assign((size_t)R, 0); att32.assign((size_t)R, 0);
        restarts.assign((size_t)R, 0); steps_done.assign((size_t)R, 0); swaps_kept.assign((size_t)R, 0);
        e->tau_log.assign((size_t)R, {});
        e->tau_ev_ptr0.assign((size_t)R, ev_ptr_start);
        mevn.assign((size_t)R, 0);
        fresh.assign((size_t)R, 1);
        // occupied-compartment lists (sparse states): possible with the byte drift pass and the front pass; the estimate is the count of the
        // uploaded state, then what the drift pass of the last step counted (the largest replicate)
        const char *nol = getenv("VGX_TAU_NO_OCCLIST");
        occ_lists_ok = a.use8 && a.front_on && a.occ != nullptr && !(nol && nol[0] == '1');
        const char *ddr = getenv("VGX_TAU_DENSE_DRIFT");     // comparisons: vgx_tau_drift8_kernel also on sparse states
        dense_drift = ddr && ddr[0] == '1';
        occ_est = occupied;
        const char *nfo = getenv("VGX_TAU_NO_FRONT_ALONE");
        front_split = R == 1 && a.front_on && !(nfo && nfo[0] == '1');   // (several replicates: their tries end at different places)
        // ... and whole rounds of a step without the host in between (VgxTauArgs.spec / gate); VGX_TAU_SPEC=0: one try per synchronisation as
        // before, VGX_TAU_SPEC=k: k front passes per round; otherwise the number of front passes per round follows the last step's (rejected
        // tries + the one that ran + one to spare)
        if (const char *sk = getenv("VGX_TAU_SPEC")) { spec_k = atoi(sk); spec_adapt = false; }
        spec_rounds = front_split && spec_k > 0;
    }

    // Small models: the whole step loop on the device, one workgroup per replicate (vgx_taus.hip).  VGX_TAU_STEP_KERNELS=1 and the
    // test switches of the step kernels (dense validation modes, the large-model draw thresholds) keep the step kernels.
    bool choose_device_loop() {
        slog_cap = step_log_rows();
        if (sets) return true;      // (check_sets has refused what the loop cannot run)
        // One workgroup (one CU) runs a replicate's whole loop: that wins where a step is launch-bound (up to ~2000 compartments at any
        // ensemble size) or where there are replicates to fill the chip with; few replicates of a larger model are faster spread over the
        // chip by the step kernels.  Measured in round 4 (tools/probe_tau_single.py, steps/s of ONE trajectory, step kernels / loop):
        // 256 compartments 8.9e3 / 5.3e4, 1280: 8.6e3 / 1.46e4 (1.2e6 infected: 7.1e3 / 6.5e3), 2048: 8.7e3 / 9.3e3, 4096: 8.3e3 / 3.9e3,
        // 8192: 8.2e3 / 3.1e3; at 32 replicates 4096 compartments are level (1.4e5 / 1.2e5), from 128 on the loop leads everywhere.
        const int64_t n_channels = P * H * (2 + 3 * e->d.sites + S + (P - 1) * S) + P * S * S;
        bool use_small = taus_shape_ok(e, sparse_default) && (n_channels <= 4096 || P * H <= 2048 || R >= 32) &&
                         (double)R * (double)slog_cap * 24.0 <= 8e9;
        const char *fs = getenv("VGX_TAU_STEP_KERNELS"), *th = getenv("VGX_TAU_LARGE_MODEL_THRESHOLDS");
        if ((fs && fs[0] == '1') || (th && th[0] == '1')) use_small = false;
        if (fs && fs[0] == '0' && taus_shape_ok(e, sparse_default))
            use_small = true;      // (VGX_TAU_STEP_KERNELS=0: the on-device loop wherever it can run, for tests and comparisons)
        return use_small;
    }

    // The on-device loop: one launch, then its per-replicate record and step log
    int run_device_loop() {
        std::vector<int32_t> i32((size_t)(P * H));
        for (int64_t i = 0; i < P * H; i++) i32[(size_t)i] = (int32_t)h.initial_infectious[(size_t)i];
        int rc = upload(e, e->t_iI, i32.data(), i32.size());
        rc |= upload(e, e->t_iS, h.initial_susceptible.data(), h.initial_susceptible.size());
        rc |= ensure(e, e->t_slog, (size_t)(R * slog_cap * 3) * 8);
        rc |= ensure(e, e->t_sres, (size_t)(R * 24) * 8);
        if (rc) return rc;
        VgxTausArgs ta{};
        ta.p = e->dp; ta.R = R;
        ta.I = a.I; ta.S = a.S; ta.totInf = a.totInf; ta.cd = a.cd; ta.lock = a.lockON;
        ta.i_I = (const int32_t *)e->t_iI.p; ta.i_S = (const int64_t *)e->t_iS.p;
        ta.seeds = a.seeds;
        ta.iterations = iterations; ta.sample_size = sample_size; ta.attempts = attempts; ta.time = time;
        ta.start_ok = start_ok ? 1 : 0; ta.rates_nonzero_initial = rates_nonzero_initial ? 1 : 0;
        ta.ev_ptr0 = ev_ptr_start; ta.ev_size = ev_size;
        ta.t0 = h.currentTime; ta.gI0 = h.globalInfectious; ta.good0 = h.good_attempt;
        for (int i = 0; i < 8; i++) ta.base_cnt[i] = base_cnt[(size_t)i];
        ta.mut_uniform = a.mut_uniform;
        memcpy(ta.mutp, a.mutp, sizeof(ta.mutp));
        ta.mev = a.mev; ta.mev_cap = mev_cap;
        ta.slog = (int64_t *)e->t_slog.p; ta.slog_cap = slog_cap;
        ta.loc_rec = a.loc_rec; ta.loc_time = a.loc_time; ta.loc_n = a.loc_n;
        ta.res = (int64_t *)e->t_sres.p;
        ta.traj = a.traj; ta.traj_points = a.traj_points; ta.traj_t0 = a.traj_t0; ta.traj_dt = a.traj_dt;
        VgxTausSetsArgs sa{};
        if (sets) {    // what the one-set kernels read as one value of `ta`, per set
            std::vector<VgxTausSetRec> recs((size_t)e->n_sets, VgxTausSetRec{});
            for (int64_t g = 0; g < e->n_sets; g++) {
                VgxTausSetRec &q = recs[(size_t)g];
                const TauSetTables &t = e->h_sets[(size_t)g];
                q.start_ok = set_start_ok[(size_t)g]; q.rates_nonzero_initial = set_rates_nonzero_initial[(size_t)g];
                q.mut_uniform = (t.mut_uniform && sites_ok16(e)) ? 1 : 0;
                memcpy(q.mutp, t.mutp, sizeof(q.mutp));
                for (int i = 0; i < 8; i++) q.base_cnt[i] = base_cnt[(size_t)i];
                q.base_cnt[6] = set_swaps[(size_t)g];
            }
            TAU_TRY(upload(e, e->ps_taurec, recs.data(), recs.size()));
            HIPCHECK(e, hipStreamSynchronize(e->stream));    // (recs goes out of scope)
            sa.a = ta;
            sa.psets = (const VgxDevParams *)e->ps_blocks.p; sa.set_of = (const int32_t *)e->ps_setof.p;
            sa.recs = (const VgxTausSetRec *)e->ps_taurec.p;
        }
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        if (sets) HIPCHECK(e, vgxi_launch_taus_sets(&sa, e->max_C(), e->max_CB(), e->stream));
        else HIPCHECK(e, vgxi_launch_taus(&ta, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        HIPCHECK(e, hipEventElapsedTime(&ms_total, e->ev0, e->ev1));
        launches = 1;
        std::vector<int64_t> res((size_t)R * 24);
        HIPCHECK(e, hipMemcpy(res.data(), e->t_sres.p, res.size() * 8, hipMemcpyDeviceToHost));
        tau_h.assign((size_t)R, 0.0);
        std::vector<int64_t> sl;
        for (int64_t r = 0; r < R; r++) {
            const int64_t *o2 = &res[(size_t)r * 24];
            const int64_t er = o2[TS_ERROR];
            if (er == VGX_ERR_CAPACITY)
                return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: replicate " + std::to_string(r) + ": multievent buffer full (" + std::to_string(mev_cap) +
                                                     " rows per replicate; pass record_events=0 for large runs)");
            if (er == 7) return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: replicate " + std::to_string(r) + ": lockdown log full (" + std::to_string(VGX_LOC_CAP) + " switches per call)");
            if (er) {
                double tl_, tn_;
                memcpy(&tl_, &o2[TS_TAU], 8); memcpy(&tn_, &o2[TS_TIME], 8);
                return fail(e, VGX_ERR_LOOP_GUARD, "vgx_simulate_tau: replicate " + std::to_string(r) + (er == 6 ? ": step loop guard" : ": tau underflow in the halving loop") +
                                                       " (step " + std::to_string(o2[TS_STEPS]) + ", tries " + std::to_string(o2[TS_TRIES]) + ", tau " + std::to_string(tl_) +
                                                       ", time " + std::to_string(tn_) + ", infected " + std::to_string(o2[TS_GI]) + ")");
            }
            memcpy(&tau_h[(size_t)r], &o2[TS_TAU], 8);
            if (o2[TS_STEPS] == 0 && o2[TS_RESTARTS] == 0) tau_h[(size_t)r] = h.tau_l;
            if (timing && r == 0) fprintf(stderr, "vgx_simulate_tau: on-device loop: %lld steps, %lld tries, %.3f ms\n", (long long)o2[TS_STEPS], (long long)o2[TS_TRIES], (double)ms_total);
            gI[(size_t)r] = o2[TS_GI];
            for (int i = 0; i < 8; i++) { cnt[(size_t)r * 8 + i] = o2[TS_CNT0 + i]; cnt0[(size_t)r][(size_t)i] = 0; }
            ev_ptr[(size_t)r] = o2[TS_EVPTR]; att[(size_t)r] = o2[TS_ATT]; good[(size_t)r] = o2[TS_GOOD];
            restarts[(size_t)r] = o2[TS_RESTARTS]; steps_done[(size_t)r] = o2[TS_STEPS];
            mevn[(size_t)r] = (unsigned long long)o2[TS_MEVROWS];
            memcpy(&tnow[(size_t)r], &o2[TS_TIME], 8);
            e->tau_ev_ptr0[(size_t)r] = o2[TS_EVPTR0];
            const int64_t n = o2[TS_EVPTR] - o2[TS_EVPTR0];
            sl.resize((size_t)std::max<int64_t>(n, 0) * 3);
            if (n > 0) HIPCHECK(e, hipMemcpy(sl.data(), (int64_t *)e->t_slog.p + r * slog_cap * 3, (size_t)n * 24, hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < n; k++) {
                double t;
                memcpy(&t, &sl[(size_t)k * 3], 8);
                e->tau_log[(size_t)r].push_back({t, sl[(size_t)k * 3 + 1] & (((int64_t)1 << 56) - 1), sl[(size_t)k * 3 + 2], (int32_t)((uint64_t)sl[(size_t)k * 3 + 1] >> 56)});
            }
        }
        return VGX_OK;
    }

    // The step-kernel loop: one pass per step of all running replicates
    int run_step_loop() {
        if (a.traj) {   // the step kernels' trajectories start from the uploaded state
            HIPCHECK(e, vgxi_tau_traj(&a, 0, R, 0, e->stream));
            launches += 1;
        }
        for (int64_t guard = 1;; guard++) {
            bool any = false, finished_on_device = false;
            TAU_TRY(close_attempts(any));
            if (!any) break;
            if (guard > (int64_t)4 * (iterations + 16) * std::max<int64_t>(attempts, 1)) return fail(e, VGX_ERR_LOOP_GUARD, "vgx_simulate_tau: step loop guard");
            TAU_TRY(upload_changed());
            TAU_TRY(start_step());
            TAU_TRY(halving_loop(finished_on_device));
            TAU_TRY(read_step_record(finished_on_device));
        }
        if (a.traj) {   // the grid points after the last step: the final state
            HIPCHECK(e, vgxi_tau_traj(&a, 0, R, 1, e->stream));
            HIPCHECK(e, hipStreamSynchronize(e->stream));
            launches += 1;
        }
        return VGX_OK;
    }

    // Loop condition (pyx:2312) / end of attempt (pyx:2331-2335) for every replicate; any: some replicate takes another step
    int close_attempts(bool &any) {
        for (int64_t r = 0; r < R; r++) {
            if (finished[(size_t)r]) continue;
            if (attempts <= 0) { finished[(size_t)r] = 1; continue; }
            bool go = running[(size_t)r] && ev_ptr[(size_t)r] < ev_size && (sample_size == -1 || cnt0[(size_t)r][2] + cnt[(size_t)r * 8 + 2] < sample_size) &&
                      (!has_tl || tnow[(size_t)r] < (double)time) && (fresh[(size_t)r] || gI[(size_t)r] != 0);
            fresh[(size_t)r] = 0;
            if (go) { any = true; continue; }
            running[(size_t)r] = 0;
            if (ev_ptr[(size_t)r] <= 100 && iterations > 100) {
                TAU_TRY(restart(r));
                if (running[(size_t)r]) any = true;
                else if (!finished[(size_t)r]) r -= 1;  // re-evaluate: the attempt ends at once
            } else {
                good[(size_t)r] = att[(size_t)r] + 1;
                finished[(size_t)r] = 1;
            }
        }
        return VGX_OK;
    }

    // Restart (pyx:714-738) of replicate r: the initial state back on the device, the attempt's counters and log dropped, the next
    // attempt opened (running and fresh) or, past the last one, the replicate finished
    int restart(int64_t r) {
        restarts[(size_t)r] += 1;
        TAU_TRY(tau_upload_state(e, r, h.initial_infectious, h.initial_susceptible));
        if (a.traj) { HIPCHECK(e, vgxi_tau_traj(&a, r, 1, 0, e->stream)); launches += 1; }   // (its bins start again, on the restored state)
        i8_dirty = true;
        occ_est = occupied;   // (the start state again)
        // the lockdown records of the failed attempt stay (Restart does not clear `loc`); then CheckLockdown for
        // every population on the restored totals at time 0 (pyx:736-737), whose switches change the contact
        // densities the next attempt starts with
        unsigned long long ln_r = 0;
        HIPCHECK(e, hipMemcpy(&ln_r, a.loc_n + r, 8, hipMemcpyDeviceToHost));
        const int64_t nrec = std::min<int64_t>((int64_t)ln_r, VGX_LOC_CAP);
        TAU_TRY(drain_lockdown_log(e, r, nrec, r, r + 1));
        if (nrec > 0) HIPCHECK(e, hipMemset(a.loc_n + r, 0, 8));
        std::vector<double> cd_r((size_t)P);
        std::vector<int32_t> lk_r((size_t)P);
        HIPCHECK(e, hipMemcpy(cd_r.data(), (double *)e->t_cd.p + r * P, (size_t)P * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(lk_r.data(), (int32_t *)e->t_lock.p + r * P, (size_t)P * 4, hipMemcpyDeviceToHost));
        std::vector<int64_t> total((size_t)P, 0);
        for (int64_t pn = 0; pn < P; pn++)
            for (int64_t hn = 0; hn < H; hn++) total[(size_t)pn] += h.initial_infectious[(size_t)(pn * H + hn)];
        const int64_t flips = host_check_lockdown(e, total, lk_r, cd_r, 0.0, r, r + 1);
        if (flips > 0) {
            HIPCHECK(e, hipMemcpy((double *)e->t_cd.p + r * P, cd_r.data(), (size_t)P * 8, hipMemcpyHostToDevice));
            HIPCHECK(e, hipMemcpy((int32_t *)e->t_lock.p + r * P, lk_r.data(), (size_t)P * 4, hipMemcpyHostToDevice));
            const int32_t one = 1;
            HIPCHECK(e, hipMemcpy(a.eff_dirty + r, &one, 4, hipMemcpyHostToDevice));
        }
        swaps_kept[(size_t)r] += cnt[(size_t)r * 8 + 6] + flips;   // swapLockdown survives a Restart
        HIPCHECK(e, hipMemset((int64_t *)e->t_counters.p + r * 8, 0, 64));
        HIPCHECK(e, hipMemset((unsigned long long *)e->t_mevn.p + r, 0, 8));
        HIPCHECK(e, hipMemset((unsigned long long *)e->t_mevbase.p + r, 0, 8));
        for (int i = 0; i < 8; i++) cnt[(size_t)r * 8 + i] = 0;
        cnt0[(size_t)r] = {0, 0, 0, 0, 0, 0, base_cnt[6] + swaps_kept[(size_t)r], 0};
        tnow[(size_t)r] = 0.0;
        ev_ptr[(size_t)r] = 0;
        e->tau_ev_ptr0[(size_t)r] = 0;
        e->tau_log[(size_t)r].clear();
        int64_t g0 = 0;
        for (int64_t i = 0; i < P * H; i++) g0 += h.initial_infectious[(size_t)i];
        gI[(size_t)r] = g0;
        att[(size_t)r] += 1;
        if (att[(size_t)r] < attempts) {
            running[(size_t)r] = (g0 != 0 && rates_nonzero_initial) ? 1 : 0;   // pyx:2311 on the restored state
            fresh[(size_t)r] = 1;
        } else {
            finished[(size_t)r] = 1;
        }
        return VGX_OK;
    }

    // The device keeps step and time itself (vgx_tau_finish_kernel advances them exactly as the host does in read_step_record): only
    // what an attempt's end or a Restart changed is uploaded
    int upload_changed() {
        for (int64_t r = 0; r < R; r++) att32[(size_t)r] = (int32_t)att[(size_t)r];
        if (running != dev_active) { HIPCHECK(e, hipMemcpy(a.active, running.data(), (size_t)R * 4, hipMemcpyHostToDevice)); dev_active = running; }
        if (step_h != dev_step) { HIPCHECK(e, hipMemcpy(a.step, step_h.data(), (size_t)R * 4, hipMemcpyHostToDevice)); dev_step = step_h; }
        if (att32 != dev_att) { HIPCHECK(e, hipMemcpy(a.attempt, att32.data(), (size_t)R * 4, hipMemcpyHostToDevice)); dev_att = att32; }
        if (tnow != dev_time) { HIPCHECK(e, hipMemcpy(a.time_now, tnow.data(), (size_t)R * 8, hipMemcpyHostToDevice)); dev_time = tnow; }
        return VGX_OK;
    }

    // What a step enqueues before its first try: the one-byte counts if stale, rates, drift, the tau candidates, the sieve
    int start_step() {
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        if (a.use8 && i8_dirty) {     // the one-byte counts after an upload / a dense try: one pass over the 4-byte counts
            HIPCHECK(e, hipMemsetAsync(a.tmax8, 0, (size_t)(R * P * a.nt8) * 4, e->stream));
            HIPCHECK(e, vgxi_tau_conv8(&a, e->stream));
            i8_dirty = false;
            launches += 1;
        }
        // a sparse state (at most 1/32 of the compartments occupied when the last step began): the drift pass lists the occupied
        // compartments and the tries' scan and front pass go over the lists
        a.build_occ = a.use_list = (occ_lists_ok && occ_est >= 0 && occ_est * 32 <= P * H) ? 1 : 0;
        // ... and with uniform migration (the column sums' pass is there to write the lists) the drift pass itself goes over them
        // (unless the last such pass had to form the empty neighbours of too many compartments — a high mutation rate, or a smallest
        // candidate far above what the lineages' mutants bring: the dense pass for a while, then another look)
        if (sparse_ban > 0) sparse_ban -= 1;
        a.drift_sparse = (a.build_occ && a.has_mig && a.mig_uniform && !dense_drift && sparse_ban == 0 && e->d.sites <= 12) ? 1 : 0;   // (12: VGX_D8S_MAX_SITES)
        HIPCHECK(e, vgxi_tau_eff(&a, e->stream));
        HIPCHECK(e, vgxi_tau_prep(&a, e->stream));
        HIPCHECK(e, vgxi_tau_drift(&a, e->stream));
        HIPCHECK(e, vgxi_tau_choose(&a, e->stream));
        launches += 4;
        if (a.sieve_on) { HIPCHECK(e, vgxi_tau_sieve(&a, e->stream)); launches += 2; }
        return VGX_OK;
    }

    // What a discarded try asks of the host (VgxTauArgs.grow): a larger list / buffer, or the dense delta arrays for the same try
    int handle_again(int again) {
        if (again & 1) {
            if (inc_cap > ((int64_t)1 << 33) / std::max<int64_t>(R, 1))
                return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: more than 2^33 individuals change compartment in one leap");
            inc_cap *= 2;
            TAU_TRY(ensure(e, e->t_inc, (size_t)(R * inc_cap) * 8));
            a.inc = (int64_t *)e->t_inc.p;
            a.inc_cap = inc_cap;
        }
        if (again & 4) {
            if (big_cap >= P * H) return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: list of large compartments full");
            big_cap = std::min<int64_t>(P * H, big_cap * 2);
            TAU_TRY(ensure(e, e->t_big, (size_t)(R * big_cap) * 8));
            a.big = (int64_t *)e->t_big.p;
            a.big_cap = big_cap;
        }
        if (again & 8) {
            if (q_scap >= q_shard_max) return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: queue of drawing compartments full");
            q_scap = std::min<int64_t>(q_shard_max, q_scap * 2);
            TAU_TRY(ensure(e, e->t_q, (size_t)(R * q_shards * q_scap) * 8));
            a.q = (int64_t *)e->t_q.p;
            a.q_cap = q_shards * q_scap;
        }
        if (again & 16) {   // multievent rows: a larger buffer, the rows of the accepted steps move over
            if (mev_cap >= mev_max)
                return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: multievent buffer full (" + std::to_string(mev_cap) +
                                                 " rows per replicate; pass record_events=0 for large runs)");
            const int64_t new_cap = std::min<int64_t>(mev_max, mev_cap * 2);
            DevBuf nb;
            TAU_TRY(ensure(e, nb, (size_t)(R * new_cap * 6) * 8));
            std::vector<unsigned long long> base_h((size_t)R);
            HIPCHECK(e, hipMemcpy(base_h.data(), a.mev_base, (size_t)R * 8, hipMemcpyDeviceToHost));
            for (int64_t r = 0; r < R; r++)
                if (base_h[(size_t)r] > 0)
                    HIPCHECK(e, hipMemcpy((int64_t *)nb.p + r * new_cap * 6, (int64_t *)e->t_mev.p + r * mev_cap * 6,
                                          (size_t)std::min<int64_t>((int64_t)base_h[(size_t)r], mev_cap) * 48, hipMemcpyDeviceToDevice));
            // the new buffer takes the old one's place in the engine's bookkeeping
            HIPCHECK(e, hipFree(e->t_mev.p));
            e->dev_bytes -= e->t_mev.bytes;
            e->all.erase(std::remove(e->all.begin(), e->all.end(), &nb), e->all.end());
            e->t_mev.p = nb.p; e->t_mev.bytes = nb.bytes;
            mev_cap = new_cap;
            a.mev = (int64_t *)e->t_mev.p; a.mev_cap = mev_cap;
            e->tau_mev_cap = mev_cap;
        }
        if (again & 2) dense_once = true;
        if (again) HIPCHECK(e, hipMemset(a.grow, 0, (size_t)R * 4));
        return VGX_OK;
    }

    // The next try's index in the suspects' table
    int next_gen() {
        if (++a.gen >= (1u << 25)) {   // the table's try counter wraps: start over with an empty table
            HIPCHECK(e, hipMemsetAsync(e->t_stkey.p, 0, (size_t)(R * st_size) * 8, e->stream));
            a.gen = 1;
        }
        return VGX_OK;
    }

    // The try proper of a sparse try: events, arrivals, the bounds check's verdict, the decision and, if accepted, the step applied
    int enqueue_sparse_try() {
        HIPCHECK(e, vgxi_tau_draw(&a, e->stream));
        HIPCHECK(e, vgxi_tau_draw_big(&a, e->stream));   // (+ the immunity transitions: extra blocks of the same launch)
        HIPCHECK(e, vgxi_tau_arrivals(&a, e->stream));
        HIPCHECK(e, vgxi_tau_verdict(&a, e->stream));
        HIPCHECK(e, vgxi_tau_decide(&a, e->stream));
        HIPCHECK(e, vgxi_tau_apply(&a, e->stream));
        if (a.use8) { HIPCHECK(e, vgxi_tau_sync8(&a, e->stream)); launches += 1; }
        return VGX_OK;
    }

    // The halving loop of one step (pyx:2316-2321): tries until every running replicate has accepted one
    int halving_loop(bool &finished_on_device) {
        dense_once = false;
        for (int tries = 0;; tries++) {
            bool step_over = false;
            if (spec_rounds && sparse_default && !dense_once) {
                TAU_TRY(spec_round(tries, finished_on_device));
                step_over = finished_on_device;
            } else {
                a.sparse = (sparse_default && !dense_once) ? 1 : 0;
                if (!a.sparse && !dense_ready) {
                    TAU_TRY(ensure_dense());
                    a.dChk = (int32_t *)e->t_dChk.p; a.dApp = (int32_t *)e->t_dApp.p;
                }
                dense_once = false;
                TAU_TRY(next_gen());
                TAU_TRY((front_split && a.sparse && !front_done) ? front_alone(tries, step_over) : plain_try(tries, step_over));
            }
            if (step_over) return VGX_OK;
        }
    }

    // One replicate, ONE synchronisation per round: the front passes of `spec_k` tries back to back (each returns at once when
    // an earlier one has found nothing: VgxTauArgs.spec), the try proper of that one, and the end of the step, all enqueued
    // without a look from the host.  What the host reads afterwards: accepted / grow as the last decide kernel that ran left
    // them.  (Tries that find a failure cost what they cost before; what goes is the host's turn between them.)
    int spec_round(int &tries, bool &finished_on_device) {
        a.sparse = 1;
        HIPCHECK(e, hipMemsetAsync(a.spec, 0, (size_t)R * 4, e->stream));
        for (int j = 0; j < spec_k; j++) {
            TAU_TRY(next_gen());
            a.phase = 1; a.gate = 1;
            HIPCHECK(e, vgxi_tau_draw(&a, e->stream));
            HIPCHECK(e, vgxi_tau_decide(&a, e->stream));
            launches += 3;
        }
        TAU_TRY(next_gen());
        a.phase = 2; a.gate = 2;
        TAU_TRY(enqueue_sparse_try());
        a.gate = 3;
        HIPCHECK(e, vgxi_tau_finish(&a, e->stream));
        a.gate = 0; a.phase = 0;
        launches += 8;
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        host_syncs += 1;
        tries += spec_k;
        acc_h.assign(pin_flags, pin_flags + (size_t)R * 2);
        if (acc_h[0]) { finished_on_device = true; return VGX_OK; }
        // (the rare cases: a list to enlarge, or the dense delta arrays — then the plain try runs this one)
        if (const int again = acc_h[(size_t)R]) TAU_TRY(handle_again(again));
        return halving_guard(e, tries);
    }

    // One replicate: the front pass of the try first, alone (most tries end there: three kernels and the host's turn instead
    // of ten); if it finds nothing the try proper follows (phase 2), with the queue the list pass has already built.
    int front_alone(int tries, bool &step_over) {
        a.phase = 1;
        tries_total += 1;
        if (a.use_list) tries_lists += 1;
        HIPCHECK(e, vgxi_tau_draw(&a, e->stream));
        HIPCHECK(e, vgxi_tau_decide(&a, e->stream));
        launches += 3;
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        host_syncs += 1;
        a.phase = 0;
        if (pin_flags[2 * R] == 1) { front_done = true; return VGX_OK; }     // nothing found: the same try, for real
        if (pin_flags[0]) { step_over = true; return VGX_OK; }                // (the loop guard of the halving: handled like an accepted step)
        return halving_guard(e, tries);                                       // rejected: tau halved, the next try
    }

    // One try of all running replicates and the host's look at it (after the front pass alone: its try proper)
    int plain_try(int tries, bool &step_over) {
        a.phase = front_done ? 2 : 0;
        front_done = false;
        if (a.phase == 0) {
            tries_total += 1;
            if (a.use_list && a.front_on && a.sparse) tries_lists += 1;
        }
        if (a.sparse) {
            TAU_TRY(enqueue_sparse_try());
        } else {
            HIPCHECK(e, vgxi_tau_draw(&a, e->stream));
            HIPCHECK(e, vgxi_tau_draw_big(&a, e->stream));
            i8_dirty = true;     // (the dense commit pass changes the counts without the one-byte copy)
            HIPCHECK(e, vgxi_tau_scatter(&a, e->stream));
            HIPCHECK(e, vgxi_tau_suspect(&a, e->stream));
            if (a.dense_check) HIPCHECK(e, vgxi_tau_check(&a, e->stream));
            else if (suspect_cap < P * H) {
                // more compartments below zero on their own than the list holds (never at tries the sieve lets through; tiny
                // models list every compartment): the dense pass decides
                susp_h.resize((size_t)R);
                HIPCHECK(e, hipMemcpyAsync(susp_h.data(), a.suspect_n, (size_t)R * 8, hipMemcpyDeviceToHost, e->stream));
                HIPCHECK(e, hipStreamSynchronize(e->stream));
                bool over = false;
                for (int64_t r = 0; r < R; r++) over = over || (int64_t)susp_h[(size_t)r] > suspect_cap;
                if (over) { HIPCHECK(e, vgxi_tau_check(&a, e->stream)); launches += 1; }
            }
            HIPCHECK(e, vgxi_tau_decide(&a, e->stream));
            HIPCHECK(e, vgxi_tau_commit(&a, e->stream));
        }
        launches += 8;
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        host_syncs += 1;
        acc_h.assign(pin_flags, pin_flags + (size_t)R * 2);   // accepted[R], grow[R]: the decide kernel's copy in pinned host memory
        step_over = true;
        for (int64_t r = 0; r < R; r++)
            if (running[(size_t)r] && !acc_h[(size_t)r]) step_over = false;
        if (step_over) return VGX_OK;
        // a try that lost data (a full list) or that the sparse check could not decide was discarded by the decide kernel
        // without touching tau or the try index: enlarge the list (it is empty now) / switch to the dense delta arrays
        // and run the same try again
        int again = 0;
        for (int64_t r = 0; r < R; r++) again |= acc_h[(size_t)(R + r)];
        TAU_TRY(handle_again(again));
        return halving_guard(e, tries);
    }

    // End of the step: the finish kernel (unless a speculative round has run it) and the host's copy of its record (TauRecord)
    int read_step_record(bool finished_on_device) {
        if (!finished_on_device) {
            HIPCHECK(e, vgxi_tau_finish(&a, e->stream));
            launches += 1;
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            HIPCHECK(e, hipStreamSynchronize(e->stream));
            host_syncs += 1;
        }
        float ms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
        ms_total += ms;
        tau_h.resize((size_t)R);
        std::vector<int64_t> res_h((size_t)R * TR_WORDS);
        int64_t occ_step = -1;
        memcpy(res_h.data(), pin_res, (size_t)R * TR_WORDS * 8);   // packed by the finish kernel, its copy in pinned host memory
        for (int64_t r = 0; r < R; r++) {
            if (!running[(size_t)r]) continue;
            const int64_t *rec = &res_h[(size_t)r * TR_WORDS];
            memcpy(&tau_h[(size_t)r], &rec[TR_TAU], 8);
            for (int i = 0; i < 8; i++) cnt[(size_t)r * 8 + i] = rec[TR_CNT0 + i];
            mevn[(size_t)r] = (unsigned long long)rec[TR_MEVN];
            if (rec[TR_OCC] >= 0) occ_step = std::max<int64_t>(occ_step, rec[TR_OCC]);
            if (a.drift_sparse && rec[TR_FORMED] >= 0) {
                // (another look after 32 steps, then 64, ... 4096 while the answer stays the same: such a pass can be many times the dense one)
                if ((rec[TR_OCC] + 30 * rec[TR_FORMED]) * 26 > P * H) { sparse_ban = sparse_ban_len; sparse_ban_len = std::min(2 * sparse_ban_len, 4096); }
                else sparse_ban_len = 32;
            }
            if (spec_rounds && r == 0) {
                tries_total += rec[TR_RETRY] + 1;
                if (a.use_list) tries_lists += rec[TR_RETRY] + 1;
                if (spec_adapt) spec_k = (int)std::min<int64_t>(std::max<int64_t>(rec[TR_RETRY] + 2, 2), 8);
            }
        }
        if (occ_step >= 0) occ_est = occ_step;
        for (int64_t r = 0; r < R; r++) {
            if (!running[(size_t)r]) continue;
            const int64_t *rec = &res_h[(size_t)r * TR_WORDS];
            const int32_t err = (int32_t)rec[TR_ERROR];
            if (err == VGX_ERR_CAPACITY) return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: replicate " + std::to_string(r) + ": list of cross-compartment events full");
            if (err == 7) return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: replicate " + std::to_string(r) + ": lockdown log full (" + std::to_string(VGX_LOC_CAP) + " switches per call)");
            if (err) return fail(e, VGX_ERR_LOOP_GUARD, "vgx_simulate_tau: replicate " + std::to_string(r) + ": tau underflow in the halving loop");
            if (mev_cap > 0 && (int64_t)mevn[(size_t)r] > mev_cap)
                return fail(e, VGX_ERR_CAPACITY, "vgx_simulate_tau: multievent buffer full (" + std::to_string(mevn[(size_t)r]) + " rows after " +
                                                     std::to_string(steps_done[(size_t)r] + 1) + " steps, room for " + std::to_string(mev_cap) +
                                                     "; pass record_events=0 for large runs)");
            tnow[(size_t)r] += tau_h[(size_t)r];                       // pyx:2322
            e->tau_log[(size_t)r].push_back({tnow[(size_t)r], rec[TR_MEVBASE], (int64_t)mevn[(size_t)r], (int32_t)rec[TR_RETRY]});  // pyx:2325
            ev_ptr[(size_t)r] += 1;
            step_h[(size_t)r] += 1;
            steps_done[(size_t)r] += 1;
            gI[(size_t)r] = rec[TR_GI];
            dev_time[(size_t)r] = tnow[(size_t)r];   // the finish kernel made the same two updates on the device
            dev_step[(size_t)r] = step_h[(size_t)r];
        }
        return VGX_OK;
    }

    // The lockdown log's remainder, the scalars of every replicate, and what the getters of the engine read after a tau call
    int collect_results() {
        lap("step loop");
        if (timing) {
            int64_t st_all = 0;
            for (int64_t r = 0; r < R; r++) st_all += steps_done[(size_t)r];
            fprintf(stderr, "vgx_simulate_tau: %lld tries, %lld of them over the lists of occupied compartments; %lld host synchronisations in the step loop "
                            "(%.2f per step)\n", (long long)tries_total, (long long)tries_lists, (long long)host_syncs,
                    (double)host_syncs / (double)std::max<int64_t>(st_all, 1));
        }
        std::vector<unsigned long long> locn((size_t)R);
        HIPCHECK(e, hipMemcpy(locn.data(), a.loc_n, (size_t)R * 8, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < R; r++) TAU_TRY(drain_lockdown_log(e, r, std::min<int64_t>((int64_t)locn[(size_t)r], VGX_LOC_CAP), r, r + 1));
        e->tau_sc.assign((size_t)R, VgxRepScalars{});
        for (int64_t r = 0; r < R; r++) {
            VgxRepScalars &s = e->tau_sc[(size_t)r];
            const std::vector<int64_t> &c0 = cnt0[(size_t)r];
            const int64_t *c = &cnt[(size_t)r * 8];
            s.currentTime = tnow[(size_t)r]; s.totalRate = h.totalRate; s.totalMig = h.totalMigrationRate;
            if (sets) { s.totalRate = rep_total_rate[(size_t)r]; s.totalMig = rep_total_mig[(size_t)r]; }
            s.tau_l = tau_h.empty() ? h.tau_l : tau_h[(size_t)r];
            s.globalInfectious = gI[(size_t)r];
            s.bCounter = c0[0] + c[0]; s.dCounter = c0[1] + c[1]; s.sCounter = c0[2] + c[2]; s.mCounter = c0[3] + c[3];
            s.iCounter = c0[4] + c[4]; s.migPlus = c0[5] + c[5]; s.migNonPlus = h.migNonPlus;
            s.swapLockdown = c0[6] + c[6];
            s.good_attempt = good[(size_t)r];
            s.ev_ptr = ev_ptr[(size_t)r];
            s.loop_iterations = steps_done[(size_t)r];
            s.restarts = restarts[(size_t)r];
            s.loc_n = (int64_t)e->tau_loc_time[(size_t)r].size();
            s.mev_rows = (int64_t)mevn[(size_t)r];
            s.traj_next = c[7];  // events drawn (sum of multiplicities), reported through vgx_counters.reserved[0]
            if (restarts[(size_t)r] > 0) s.migNonPlus = 0;
        }
        e->tau_sieve_skipped.assign((size_t)R, 0);
        HIPCHECK(e, hipMemcpy(e->tau_sieve_skipped.data(), a.sieve_skipped, (size_t)R * 8, hipMemcpyDeviceToHost));
        e->sc_host = e->tau_sc;
        e->sc_host_valid = true;
        e->direct_logs_valid = false;
        e->last_was_tau = true;
        e->last_ms = ms_total;
        e->last_launches = launches;
        e->last_ev_size = ev_size;
        e->ev_ptr0 = ev_ptr_start;
        e->traj_points = o.traj_points > 0 ? o.traj_points : 0;
        h.ev_ptr = ev_ptr[0];
        return VGX_OK;
    }
};

extern "C" int vgx_simulate_tau(vgx_engine *e, int64_t iterations, int64_t sample_size, float time, int64_t attempts,
                                const vgx_run_opts *opts) {
    if (!e) return VGX_ERR_ARG;
    e->traj_points = 0;    // (until this call has written its own: vgx_get_trajectories never returns the bins of an earlier call)
    if (!e->have_params || !e->have_state) return fail(e, VGX_ERR_ARG, "vgx_simulate_tau: set params and state first");
    HIPCHECK(e, hipSetDevice(e->device));
    TauRun run{e, e->hs, e->d.hapNum, e->d.popNum, e->d.susNum, e->R, iterations, sample_size, attempts, time, !(time == -1.0f), e->hs.ev_ptr, e->hs.ev_size};
    run.o.record_events = 1;
    if (opts) run.o = *opts;
    if (run.sets) {
        // (a call that does not ask for the sets is refused as it was before they could run: nothing a caller relied on changes)
        if (run.o.reserved[0] != 2)
            return fail(e, VGX_ERR_ARG, "vgx_simulate_tau: several parameter sets are installed (vgx_set_param_sets): tau-leaping runs one set only "
                                        "unless vgx_run_opts.reserved[0] = 2 asks for one set per replicate on the on-device step loop");
        TAU_TRY(run.check_sets());
    }
    TAU_TRY(run.prepare_start());
    TAU_TRY(run.alloc_workspace());
    TAU_TRY(run.fill_args());
    run.open_bookkeeping();
    if (run.choose_device_loop()) TAU_TRY(run.run_device_loop());
    else TAU_TRY(run.run_step_loop());
    return run.collect_results();
}
