// vgx_direct_run.hip — the host driver of the direct Gillespie path: vgx_simulate_direct of include/vgx.h, and direct_core, which
// the tau driver shares.
//
// No kernels here: a .hip file for the build's flags and the launchers' types alone.  Three parts: the choice of the call's kernel
// (vgx_choose_direct: a pure function of a vgx_direct_shape and the options, which a test reaches without a device through
// vgx_test_direct_plan); the upload of a state into the kernels' layout (init_device_state); and the call itself, a sequence of stages
// over one DirectRun, which owns everything a pass keeps between them — the stages are its member functions, in the order a pass runs
// them.
#include "vgx_engine.h"

#define DIRECT_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

// ------------------------------------------------------------------------------------------------
// The kernel choice.  Small models run one replicate per LANE (vgx_lanes.hip: the reference's serial loops, dense state); everything
// else one replicate per wavefront, or four.  opts.kernel: 0 = automatic, 1 = wavefront, 2 = lane, 3 = four replicates per wavefront
// (whichever of its forms takes the model), 4 = its general form, 5 = single trajectory (vgx_solo.hip), 6 = single trajectory of a
// large haplotype space (vgx_lone.hip).  Every limit of a kernel's scope is written once, in the predicates below.

// One rate class, one susceptibility group, at most 64 populations: the shapes the four-replicates-per-wavefront kernels of one-class
// models (vgx_quad.hip, vgx_quadf.hip) take; the device state keeps the 4-byte copy of the counts for them alone.
static bool one_class(int64_t P, int64_t S, int64_t C, int64_t CB) { return P <= 64 && S == 1 && C == 1 && CB == 1; }
// ... and no population that can switch its lockdown state
static bool one_class_shape(const vgx_direct_shape *s) { return one_class(s->P, s->S, s->C, s->CB) && !s->ld_possible; }

// The general form of that kernel (vgx_quadg.hip): several susceptibility groups and rate classes, lockdown switches, up to 128 populations.
static bool general_row_shape(const vgx_direct_shape *s) {
    return s->P <= VGX_QG_MAX_P && s->S <= VGX_QG_MAX_S && s->C <= VGX_QG_MAX_C && s->CB <= VGX_QG_MAX_CB &&
           3 * s->S + s->CB <= VGX_QG_MAX_W && s->n_seg <= VGX_QG_MAX_SEG;
}

// The compact layout of the single-trajectory kernel (vgx_solo.h): 0 = the model does not fit it, 1 / 2 = with one / two registers of terms.
static int64_t solo_compact(const vgx_direct_shape *s) {
    const int64_t maxterms = s->solo_maxnnz * s->P;
    if (s->solo_ncls > VGX_SOLO_ROWS || s->S > VGX_SOLO_MAX_S || s->P > 64 || maxterms > 32) return 0;
    return maxterms <= 16 ? 1 : 2;
}

// LDS bytes of the single-trajectory kernel for a model within its limits; migrationRates stay in HBM where they do not fit beside the rest.
static int64_t solo_lds_bytes(const vgx_direct_shape *s, int64_t *mig_in_lds) {
    const int64_t with_mig = vgx_solo_layout((int)s->P, (int)s->H, (int)s->S, (int)s->sites, 1).total;
    *mig_in_lds = with_mig <= VGX_SOLO_MAX_LDS ? 1 : 0;
    return *mig_in_lds ? with_mig : vgx_solo_layout((int)s->P, (int)s->H, (int)s->S, (int)s->sites, 0).total;
}

// The requests for FAST arithmetic that the exact kernels serve.
enum Remap { REMAP_NONE, REMAP_FAST, REMAP_PHILOX };
static Remap remap_of(const vgx_direct_shape *s, const vgx_run_opts *o) {
    const int64_t k = o->kernel;
    if (s->recomb) return REMAP_NONE;
    const bool general_model = !one_class_shape(s) && general_row_shape(s);
    // FAST mode promises the exact mode's integer rows on the same seed and times within 1e-9 — which the exact mode delivers.  Its
    // own row kernel (vgx_quadf.hip) takes one-class models; for every other model that the exact row kernels or the latency
    // kernel take, those ARE the fast path (tools/probe_fast_general.py, 16 384 replicates of the Table-3 model: 1.4e9 / 1.1e9 /
    // 4.2e8 events/s at 2 / 10 / 100 demes against 2.5e8 / 2.5e8 / 1.3e8 on the FAST form of the wavefront kernel).  The
    // counter-based stream (mode 2) is another trajectory and stays where it is.
    if (o->mode == 1 && k == 0 && general_model) return REMAP_FAST;
    // The counter-based stream (mode 2) on such a model: the general row kernel's EXACT arithmetic on the Philox stream — the exact
    // mode's rows for those random numbers (the oracle on the same stream agrees bit for bit), at that kernel's rate instead of the
    // wavefront kernel's (16 384 replicates of the Table-3 model, K = 10: 1.3e9 against 2.5e8 events/s).  The latency kernels and the
    // one-class exact row kernel draw from the PCG64 stream only.
    // Likewise the latency kernels (one trajectory or a few: vgx_solo.hip, vgx_lone.hip), for every shape they take.
    if (o->mode == 2 && (k == 0 || k == 5 || k == 6 || ((k == 3 || k == 4) && general_model))) return REMAP_PHILOX;
    return REMAP_NONE;
}

int vgx_choose_direct(const vgx_direct_shape *s, const vgx_run_opts *o, vgx_direct_plan *plan, std::string &err) {
    const int64_t P = s->P, H = s->H, S = s->S, R = s->R, C = s->C, CB = s->CB, k = o->kernel;
    const bool ld_possible = s->ld_possible != 0;
    // Recombination (pyx:575-596), exact mode only: the single-trajectory kernel, the general row kernel (its *_rec instantiations), the
    // wavefront kernel (any shape), and — when asked for — the lane kernel (serial, dense state) while the dense arrays fit.
    const bool recomb = s->recomb != 0;
    *plan = vgx_direct_plan{};
    auto refuse = [&err](const char *msg) { err = msg; return (int)VGX_ERR_ARG; };

    // Several parameter sets (vgx_set_param_sets): the wavefront kernel's scenario form, exact mode; every other kernel and mode reads
    // one shared parameter copy.
    if (s->param_sets > 1) {
        if (o->mode != 0)
            return refuse("vgx_simulate_direct: several parameter sets are installed (vgx_set_param_sets): they run in exact mode (mode 0) only");
        if (k != 0 && k != 1)
            return refuse("vgx_simulate_direct: several parameter sets are installed (vgx_set_param_sets): they run on the "
                          "one-replicate-per-wavefront kernel only (kernel 0 or 1)");
        plan->kernel = VGX_K_WAVE;
        return VGX_OK;
    }

    // A FAST request that the exact kernels serve counts as exact in every scope below.  Where the call then lands on no exact kernel,
    // plan->mode (set once, after the choice) is the request's own mode again.
    const Remap remap = remap_of(s, o);
    const bool exact = o->mode == 0 || remap != REMAP_NONE;
    const bool exact_pcg = exact && remap != REMAP_PHILOX;          // ... on the PCG64 stream

    if (recomb && !exact) return refuse("vgx_simulate_direct: recombination runs in exact mode only");
    if (k < 0 || k > 6) return refuse("vgx_simulate_direct: kernel must be 0..6");
    const bool lane_ok = exact_pcg && (recomb ? P * H * std::max<int64_t>(S, 1) <= (1 << 24)
                                              : (P * H <= 1024 && P <= 16 && S <= 8 && H <= s->cap));
    if (k == 2 && !lane_ok)
        return refuse("vgx_simulate_direct: the lane-per-replicate kernel needs exact mode, popNum <= 16, "
                      "popNum * hapNum <= 1024 and susNum <= 8");
    // One trajectory (or a few) of a small model: the latency kernel (vgx_solo.hip), the whole model in LDS and registers.
    int64_t solo_mig_in_lds = 0, solo_lds = 0;
    bool solo_ok = exact && H <= VGX_SOLO_MAX_H && P <= VGX_SOLO_MAX_P && S <= VGX_SOLO_MAX_S && s->n_solo_seg <= VGX_SOLO_MAX_SEG &&
                   H <= s->cap &&
                   ((P <= 16 && H <= 16) || (s->n_seg <= VGX_SOLO_MAX_TSEG && s->solo_npass0 >= 0 && s->solo_npass1 >= 0)) &&
                   s->max_size < ((int64_t)1 << 52);   // counts are kept as doubles
    if (solo_ok) {
        solo_lds = solo_lds_bytes(s, &solo_mig_in_lds);
        solo_ok = solo_lds <= VGX_SOLO_MAX_LDS;
    }
    if (k == 5 && !solo_ok)
        return refuse("vgx_simulate_direct: the single-trajectory kernel needs exact mode, hapNum <= 64, "
                      "popNum <= 128, susNum <= 16 and a model that fits 160 KB of LDS");
    // Four replicates per wavefront, one per 16-lane DPP row (vgx_quad.hip): one rate class, one susceptibility group,
    // at most 64 populations, no population that can switch its lockdown state, exact mode.
    const bool quad_shape = !recomb && one_class_shape(s) && s->suscep_cumul0_zero && s->have_counts32 &&
                            s->cap <= ((int64_t)1 << 24) &&        // (the 64-ary lower bound of vgx_rowlist.h descends from stride 64^3: lists of up to 2^24 entries)
                            s->max_size < ((int64_t)1 << 31) &&    // its streaming passes read 4-byte counts
                            s->hosts_below_2p53 &&   // vgx_quad_kernel keeps the per-population totals and globalInfectious as doubles: exact while the model's host count is below 2^53
                            s->tot_sus_is_sus;
    const bool quad_ok = exact_pcg && quad_shape;
    // One trajectory (or a few hundred) of such a model with a LARGE haplotype space: the latency kernel on occupancy lists
    // (vgx_lone.hip), every list resident in LDS.  One wavefront per CU with 160 KB each up to 256 replicates, two with 80 KB beyond
    // (512 at a time).  The row kernels' four replicates per wavefront win from about 2000 replicates on (tools/probe_lone_crossover.py,
    // config 3 / its general variant, events/s: 1536 replicates 2.6e8 / 1.6e8 here against 2.3e8 / 1.3e8 there, 2048: 2.6e8 / 1.6e8 against
    // 3.1e8 / 1.8e8).  Chosen by itself only for a state that came through
    // vgx_set_state (when the lists outgrow the heap the call runs again from that state on the row kernel) whose lists leave half
    // the heap free; opts.kernel = 6 forces it on any state (a full heap is then the call's error).
    // Its general form takes what the general row kernel takes at up to 64 populations: several rate classes (the class of a list entry
    // rides in the top six bits of its haplotype word: hapNum <= 2^26), several susceptibility groups, lockdown switches.
    const int64_t lone_lds_bytes = R <= 256 ? VGX_LONE_MAX_LDS : VGX_LONE_MAX_LDS / 2;
    const bool lone_gen_shape = exact && !recomb && P <= 64 && S <= VGX_LONE_MAX_S && C <= VGX_LONE_MAX_C && CB <= VGX_LONE_MAX_CB &&
                                s->n_seg <= VGX_LONE_MAX_SEG && H <= ((int64_t)1 << VGX_LONE_HAP_BITS) &&
                                s->max_size < ((int64_t)1 << 31);   // 4-byte counts in the heap
    const bool lone_one_class = exact && quad_shape;      // (its one-class form: the exact row kernel's scope, whatever the stream)
    const int64_t lone_general = lone_one_class ? 0 : 1;
    int64_t lone_rows = 0;
    if (lone_one_class || lone_gen_shape)
        lone_rows = vgx_lone_layout((int)P, (int)lone_lds_bytes, lone_general ? (int)S : 0, lone_general ? (int)CB : 0).nrows;
    const bool lone_ok = (lone_one_class || lone_gen_shape) && lone_rows >= 2 * P;
    if (k == 6 && !lone_ok)
        return refuse("vgx_simulate_direct: the single-trajectory kernel for large haplotype spaces needs exact mode, popNum <= 64, "
                      "susNum <= 16, at most 64 rate classes and 16 transmission/susceptibility classes, hapNum <= 2^26, no recombination");
    // FAST mode (order-free sums, the PCG64 or the counter-based stream) on the same layout and scope: vgx_quadf.hip
    const bool quadf_ok = !exact_pcg && quad_shape;
    const bool quadg_ok = exact && general_row_shape(s);
    if (k == 3 && !quad_ok && !quadg_ok && !quadf_ok)
        return refuse("vgx_simulate_direct: the four-replicates-per-wavefront kernels need "
                      "popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes");
    if (k == 4 && !quadg_ok)
        return refuse("vgx_simulate_direct: the general four-replicates-per-wavefront kernel needs exact mode, "
                      "popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes");

    int64_t kernel = k;     // a kernel that was asked for and passed its check; 3 = whichever row kernel takes the request
    if (k == 3) kernel = quad_ok ? VGX_K_QUAD : quadf_ok ? VGX_K_QUADF : VGX_K_QUADG;
    if (k == 0) {
        // measured (tools/probe_lanes.py): the lane kernel only wins for minimal models in very large ensembles (config 2 at
        // 262 144 replicates: 2.4e9 vs 7.0e8 events/s); its state lives in HBM/L2, so every other shape is latency-bound
        // (recombination: the single-trajectory kernel for few replicates of a model it takes, else the general row kernel, else the wavefront kernel)
        // (recombination, measured in round 4 — tools/probe_recomb_ens.py, 16 384 replicates of the recomb_a / recomb_pos models: the general row
        // kernel 6.4-6.9e8 events/s, the wavefront kernel 3.1-3.4e8, the lane kernel 1.0-1.2e7: the lane kernel only when it is asked for)
        // (config 2, tools/probe_config2.py: 65 536 replicates 1.8e9 events/s here against 2.0e9 on the row kernel, 262 144: 4.0e9 against 2.1e9)
        const bool lanes = !recomb && lane_ok && P * H * S <= 4 && R >= 131072;
        // measured (tools/probe_single.py, round 3): the row kernels lead at every ensemble size, a single trajectory included —
        // config 2: 2.9e5 events/s against 2.0e5 on the one-replicate-per-wavefront kernel, config 3: 1.75e5 against 1.26e5; four
        // replicates in one wavefront: 1.1e6 / 5.9e5 against 7.9e5 / 4.9e5 in four wavefronts
        // measured (bench legs table3 / single_trajectory, round 4): a lone wavefront of the latency kernel does a Table-3 trajectory
        // several times faster than a row of the row kernels; those win back from a few thousand replicates on (four per wavefront)
        // ... except general models (what the general row kernel would take) in the compact layout with a small LDS footprint: there two
        // wavefronts per SIMD of this kernel beat it too (tools/probe_solo_ens.py, 16 384 replicates of the Table-3 model: K = 2 1.68e9
        // against 1.09e9 events/s, K = 10 1.37e9 against 1.09e9; K = 100, general layout, 150 KB of LDS: 4.7e7 against 3.6e8)
        // One-class models the latency kernel takes too: the row kernel needs four replicates per wavefront, so below 8192 replicates it
        // cannot give every SIMD its two wavefronts (tools/probe_oneclass_small.py, config 2 and the one-class goldens: 2048 replicates
        // 1.3-1.6e9 events/s here against 5e8 there, 4096: 1.4-1.7e9 against 1.0e9; from 8192 on the row kernel leads, 1.8-1.9e9 against 1.5-1.7e9)
        const bool solo_many = solo_ok && (quad_ok ? R < 8192 : solo_compact(s) != 0) && solo_lds <= 20 * 1024;
        const bool solo = solo_ok && !lanes && (R < 2048 || solo_many);
        const bool lone = lone_ok && !lanes && s->fresh_state && R <= 1536 && 2 * s->start_lone_rows <= lone_rows && !s->no_lone;
        // The general row kernel also for FEW replicates of models with up to 16 populations (one register slot): a wavefront running alone
        // does a Table-3 trajectory at 1.7e5 events/s there against 1.0e5 on the one-replicate-per-wavefront kernel
        // (tools/probe_single.py; at 64 populations the wave kernel leads, 1.25e5 against 0.94e5).
        const bool quadg = quadg_ok && (R >= 2048 || (P <= 16 && (S > 1 || C > 1 || ld_possible)));
        kernel = lanes ? VGX_K_LANES : solo ? VGX_K_SOLO : lone ? VGX_K_LONE : quad_ok ? VGX_K_QUAD : quadf_ok ? VGX_K_QUADF
                 : quadg ? VGX_K_QUADG : VGX_K_WAVE;
    }
    plan->kernel = kernel;
    // A remapped request that landed on no exact kernel keeps its own mode: fewer than 2048 replicates of a model neither the row nor the
    // latency kernels take there run faster on the wavefront kernel's own FAST form; a counter-based request on a one-class model runs
    // on the FAST row kernel, else on that form too.
    const bool exact_kernel = kernel != VGX_K_WAVE && kernel != VGX_K_QUADF;
    plan->mode = (remap != REMAP_NONE && exact_kernel) ? 0 : o->mode;
    plan->fast = plan->mode >= 1 ? 1 : 0;
    plan->philox = o->mode == 2 ? 1 : 0;
    if (kernel == VGX_K_SOLO) {
        plan->solo_mig_in_lds = solo_mig_in_lds;
        plan->solo_compact = s->solo_general ? 0 : solo_compact(s);
    }
    if (kernel == VGX_K_LONE) {
        plan->lone_general = lone_general;
        plan->lone_lds_bytes = lone_lds_bytes;
        if (k == 0) {   // a full heap sends the automatic choice to the row kernels, or to the wavefront kernel
            plan->fallback_kernel = (quad_ok || quadg_ok || quadf_ok) ? VGX_K_QUAD : VGX_K_WAVE;
            plan->fallback_mode = remap == REMAP_PHILOX ? 2 : plan->mode;       // (the request as it came)
        }
    }
    // the row kernels with zero-count entries work on the 4-byte counts alone; everything else reads the 8-byte ones
    plan->long_lists = (kernel == VGX_K_QUAD && s->start_max_nocc > 64) ? 1 : 0;
    plan->leaves32 = (kernel == VGX_K_QUADF || plan->long_lists) ? 1 : 0;
    return VGX_OK;
}

extern "C" int vgx_test_direct_plan(const vgx_direct_shape *shape, const vgx_run_opts *opts, vgx_direct_plan *plan, char *errbuf, int64_t errcap) {
    if (!shape || !opts || !plan) return VGX_ERR_ARG;
    std::string err;
    const int rc = vgx_choose_direct(shape, opts, plan, err);
    if (errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", err.c_str());
    return rc;
}

// dense [P][H] -> ordered occupancy lists
static void build_lists(const vgx_engine *e, const std::vector<int64_t> &dense, std::vector<int32_t> &nocc,
                        std::vector<int32_t> &hap, std::vector<int32_t> &cl, std::vector<int64_t> &cnt, int64_t &cap) {
    const int64_t H = e->d.hapNum, P = e->d.popNum;
    nocc.assign((size_t)P, 0);
    int64_t mx = 0;
    for (int64_t pn = 0; pn < P; pn++) {
        int64_t n = 0;
        for (int64_t h = 0; h < H; h++) n += dense[(size_t)(pn * H + h)] != 0;
        nocc[(size_t)pn] = (int32_t)n;
        mx = std::max(mx, n);
    }
    cap = std::max<int64_t>(mx, 1);
    hap.assign((size_t)(P * cap), 0);
    cl.assign((size_t)(P * cap), 0);
    cnt.assign((size_t)(P * cap), 0);
    for (int64_t pn = 0; pn < P; pn++) {
        int64_t k = 0;
        for (int64_t h = 0; h < H; h++) {
            int64_t v = dense[(size_t)(pn * H + h)];
            if (v != 0) {
                hap[(size_t)(pn * cap + k)] = (int32_t)h;
                cl[(size_t)(pn * cap + k)] = e->cls[(size_t)h];
                cnt[(size_t)(pn * cap + k)] = v;
                k++;
            }
        }
    }
}

static size_t lds_bytes_for(const vgx_engine *e) {
    return vgxi_direct_lds_bytes((int)e->d.popNum, (int)e->d.susNum, e->max_C(), e->max_CB());
}

static int init_device_state(vgx_engine *e, int64_t traj_points) {
    HostState &h = e->hs;
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum, R = e->R;
    std::vector<int32_t> nocc, hap, cl, i_nocc, i_hap, i_cl;
    std::vector<int64_t> cnt, i_cnt;
    int64_t s_cap = 1, i_cap = 1;
    build_lists(e, h.infectious, nocc, hap, cl, cnt, s_cap);
    build_lists(e, h.initial_infectious, i_nocc, i_hap, i_cl, i_cnt, i_cap);

    // list capacity per (replicate, population): worst case H when it fits the memory budget
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t need = std::max<int64_t>(std::max(s_cap, i_cap), 1);
    e->start_max_nocc = s_cap;
    {
        int64_t rows_s = 0, rows_i = 0;
        for (int64_t pn = 0; pn < P; pn++) { rows_s += vgx_lone_min_rows(nocc[(size_t)pn]); rows_i += vgx_lone_min_rows(i_nocc[(size_t)pn]); }
        e->start_lone_rows = std::max(rows_s, rows_i);
    }
    // capacity per list: what fits 45 % of the free memory (buffers of an earlier state count as free: they are reused), at most
    // 32 GiB for all lists together (an ensemble of 16 384 x 64 lists still gets 1600 entries each; the rest of the memory
    // belongs to the event logs and trajectories), never below the start state's longest list + one tile.  Rounded down to a
    // multiple of 64 entries: the row kernels read whole 64-entry tiles with 16-byte loads.
    const double reusable = (double)(e->r_lhap.bytes + e->r_lcls.bytes + e->r_lcnt.bytes + e->r_lcnt32.bytes);
    const double list_bytes = std::min(((double)free_b + reusable) * 0.45, 32.0 * 1073741824.0);
    int64_t budget = (int64_t)(list_bytes / (double)(R * P * 24));
    if (const char *lc = getenv("VGX_LIST_CAP")) {     // diagnostics / tests: a small list capacity (the overflow paths of the kernels)
        const long long v = atoll(lc);
        if (v > 0) budget = std::min<int64_t>(budget, (int64_t)v);
    }
    int64_t cap = std::min<int64_t>(H, std::max<int64_t>(budget, 64));
    cap = std::max(cap, std::min<int64_t>(H, need + 64));
    if (cap < H) cap = std::max<int64_t>((cap / 64) * 64, ((need + 63) / 64) * 64);
    if (cap < need) return fail(e, VGX_ERR_CAPACITY, "occupancy lists do not fit device memory");
    e->cap = cap;

    int rc = 0;
    rc |= ensure(e, e->r_popD, (size_t)(R * PD_COUNT * P) * 8);
    rc |= ensure(e, e->r_popI, (size_t)(R * PI_COUNT * P) * 8);
    rc |= ensure(e, e->r_sus, (size_t)(R * P * S) * 8);
    rc |= ensure(e, e->r_immSrc, (size_t)(R * P * S) * 8);
    rc |= ensure(e, e->r_birthC, (size_t)(R * P * e->max_CB()) * 8);
    rc |= ensure(e, e->r_xC, (size_t)(R * P * e->max_CB() * S) * 8);
    rc |= ensure(e, e->r_effMig, (size_t)(R * P * P) * 8);
    rc |= ensure(e, e->r_nocc, (size_t)(R * P) * 4);
    rc |= ensure(e, e->r_lhap, (size_t)(R * P * cap + 64) * 4);
    rc |= ensure(e, e->r_lcls, (size_t)(R * P * cap) * 4);
    rc |= ensure(e, e->r_lcnt, (size_t)(R * P * cap + 64) * 8);   // + one tile: vgx_quad.hip reads whole 64-entry tiles
    const bool want32 = one_class(P, S, e->max_C(), e->max_CB());   // shapes the four-replicates-per-wavefront kernel takes
    if (want32) rc |= ensure(e, e->r_lcnt32, (size_t)(R * P * cap + 64) * 4 + (size_t)(R * P * cap) + 128);   // + the one-byte copy of vgx_quad_long_kernel
    const int64_t capT = cap / 64 + 1;
    rc |= ensure(e, e->r_ltsum, (size_t)(R * P * capT) * 16 + 64);   // tile sums, then the exact row kernel's cached running sums
    rc |= ensure(e, e->r_sc, (size_t)R * sizeof(VgxRepScalars));
    rc |= ensure(e, e->r_prof, (size_t)(R * VGX_PROF_SLOTS) * 8);
    if (rc) return rc;
    HIPCHECK(e, hipMemsetAsync(e->r_effMig.p, 0, (size_t)(R * P * P) * 8, e->stream));
    HIPCHECK(e, hipMemsetAsync(e->r_popD.p, 0, (size_t)(R * PD_COUNT * P) * 8, e->stream));
    HIPCHECK(e, hipMemsetAsync(e->r_immSrc.p, 0, (size_t)(R * P * S) * 8, e->stream));

    rc |= upload(e, e->s_nocc, nocc.data(), nocc.size());
    rc |= upload(e, e->s_hap, hap.data(), hap.size());
    rc |= upload(e, e->s_cls, cl.data(), cl.size());
    rc |= upload(e, e->s_cnt, cnt.data(), cnt.size());
    rc |= upload(e, e->s_sus, h.susceptible.data(), h.susceptible.size());
    rc |= upload(e, e->s_cd, h.contactDensity.data(), h.contactDensity.size());
    std::vector<int64_t> tot((size_t)(3 * P));
    for (int64_t pn = 0; pn < P; pn++) {
        tot[(size_t)pn] = h.totalSusceptible[(size_t)pn];
        tot[(size_t)(P + pn)] = h.totalInfectious[(size_t)pn];
        tot[(size_t)(2 * P + pn)] = h.lockdownON[(size_t)pn];
    }
    rc |= upload(e, e->s_tot, tot.data(), tot.size());
    rc |= upload(e, e->i_nocc, i_nocc.data(), i_nocc.size());
    rc |= upload(e, e->i_hap, i_hap.data(), i_hap.size());
    rc |= upload(e, e->i_cls, i_cl.data(), i_cl.size());
    rc |= upload(e, e->i_cnt, i_cnt.data(), i_cnt.size());
    rc |= upload(e, e->i_sus, h.initial_susceptible.data(), h.initial_susceptible.size());
    rc |= upload(e, e->r_seeds, e->seeds.data(), e->seeds.size());
    if (rc) return VGX_ERR_HIP;

    e->sc_host.assign((size_t)R, VgxRepScalars{});
    for (int64_t r = 0; r < R; r++) {
        VgxRepScalars &s = e->sc_host[(size_t)r];
        s.currentTime = h.currentTime; s.totalRate = h.totalRate; s.totalMig = h.totalMigrationRate; s.tau_l = h.tau_l;
        s.globalInfectious = h.globalInfectious;
        s.bCounter = h.bCounter; s.dCounter = h.dCounter; s.sCounter = h.sCounter; s.mCounter = h.mCounter;
        s.iCounter = h.iCounter; s.swapLockdown = h.swapLockdown; s.migPlus = h.migPlus; s.migNonPlus = h.migNonPlus;
        s.good_attempt = h.good_attempt;
        s.ev_ptr = h.ev_ptr;
    }
    HIPCHECK(e, hipMemcpyAsync(e->r_sc.p, e->sc_host.data(), (size_t)R * sizeof(VgxRepScalars), hipMemcpyHostToDevice, e->stream));

    VgxDevRep &d = e->dr;
    d.popD = (double *)e->r_popD.p; d.popI = (int64_t *)e->r_popI.p; d.sus = (int64_t *)e->r_sus.p;
    d.immSrc = (double *)e->r_immSrc.p; d.birthC = (double *)e->r_birthC.p; d.xC = (double *)e->r_xC.p;
    d.effMig = (double *)e->r_effMig.p; d.nocc = (int32_t *)e->r_nocc.p; d.lhap = (int32_t *)e->r_lhap.p;
    d.lcls = (int32_t *)e->r_lcls.p; d.lcnt = (int64_t *)e->r_lcnt.p; d.cap = cap;
    d.lcnt32 = want32 ? (int32_t *)e->r_lcnt32.p : nullptr;
    d.ltsum = (int64_t *)e->r_ltsum.p; d.capT = capT;
    HIPCHECK(e, hipMemsetAsync(e->r_ltsum.p, 0, (size_t)(R * P * capT) * 8, e->stream));
    d.i_nocc = (const int32_t *)e->i_nocc.p; d.i_hap = (const int32_t *)e->i_hap.p;
    d.i_cls = (const int32_t *)e->i_cls.p; d.i_cnt = (const int64_t *)e->i_cnt.p; d.i_cap = i_cap;
    d.i_sus = (const int64_t *)e->i_sus.p;
    d.sc = (VgxRepScalars *)e->r_sc.p; d.seeds = (const int64_t *)e->r_seeds.p;
    d.prof = (unsigned long long *)e->r_prof.p;
    HIPCHECK(e, hipMemsetAsync(e->r_prof.p, 0, (size_t)(R * VGX_PROF_SLOTS) * 8, e->stream));

    HIPCHECK(e, vgxi_launch_init_reps(&d, (int)P, (int)S, R, (const int32_t *)e->s_nocc.p, (const int32_t *)e->s_hap.p,
                                      (const int32_t *)e->s_cls.p, (const int64_t *)e->s_cnt.p, s_cap,
                                      (const int64_t *)e->s_sus.p, (const double *)e->s_cd.p,
                                      (const int64_t *)e->s_tot.p, e->stream));
    if (e->n_sets > 1)   // the list classes of every replicate from its own set (s_cls holds set 0's)
        HIPCHECK(e, vgxi_launch_init_reps_sets(&d, (int)P, R, (const VgxDevParams *)e->ps_blocks.p, (const int32_t *)e->ps_setof.p, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));  // host vectors above go out of scope
    e->dev_state_valid = true;
    e->counts32_valid = want32;   // (vgx_init_reps_kernel fills both)
    e->counts64_valid = true;
    (void)traj_points;
    return VGX_OK;
}

// Everything one pass of a direct call keeps between its stages, and the stages in the order the pass runs them
struct __attribute__((visibility("hidden"))) DirectRun {
    // what direct_core hands over
    vgx_engine *const e;
    HostState &h;
    const int64_t P, R, iterations, sample_size, attempts;
    const float time;
    vgx_run_opts o;                // the request (max_loop_factor filled in)
    // the start of the call
    size_t lds = 0;                // LDS of the wavefront kernel's tables
    bool fresh_state = false;      // the call starts from the state of vgx_set_state
    std::vector<double> cont_t0;   // [R] the clock the call continues from
    int64_t ev_size = 0, evcap = 0;
    bool ld_possible = false;
    // the kernel and its arguments
    vgx_direct_shape shape{};
    vgx_direct_plan plan{};
    VgxDirectArgs a{};
    VgxSoloArgs soa{};
    VgxLoneArgs loa{};
    VgxQuadgArgs qga{};
    VgxLaneWs ws{};
    bool dev_clock = true;         // the latency kernels keep the device clock (time limit, trajectories, no event log)
    int exact_rcp_div = 1;         // x / actualSizes through the reciprocal; 0 (validation, VGX_SOLO_PLAIN_DIV): the compiler's division
    bool heap_full = false;        // vgx_lone.hip as the automatic choice ran out of LDS heap: the call runs again as plan.fallback_* say

    int check_call() {
        if (!e->have_params || !e->have_state) return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: set params and state first");
        if (iterations < 0 || attempts < 0) return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: negative iterations/attempts");
        HIPCHECK(e, hipSetDevice(e->device));
        if (o.max_loop_factor <= 0) o.max_loop_factor = 1024;
        if (o.mode < 0 || o.mode > 2) return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: mode must be 0 (exact), 1 (fast) or 2 (fast, Philox stream)");
        lds = lds_bytes_for(e);
        if (lds > 160 * 1024)
            return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: the population/class tables need " + std::to_string(lds) +
                                            " bytes of LDS per wavefront (limit 163840): too many populations x rate classes");
        return VGX_OK;
    }

    int ensure_device_state() {
        fresh_state = !e->dev_state_valid;
        if (!fresh_state) return VGX_OK;
        prepare_first(e);
        return init_device_state(e, o.traj_points);
    }

    // A call that continues the device-resident state of the previous one: its clock starts where the HOST clock of the
    // previous call ended (the reference's own libm sums), rebuilt now from that call's logs while they still exist —
    // for up to 5e7 loop iterations over all replicates (about half a second of host time); beyond that, and after calls
    // without an event log, from the device clock (vgx_log: < 1 ulp per step from the host's).
    int continue_clock() {
        std::vector<double> &t0 = cont_t0;
        t0.assign((size_t)R, h.currentTime);
        if (fresh_state || !e->sc_host_valid || e->sc_host.size() != (size_t)R) return VGX_OK;
        int64_t work = 0;
        for (int64_t r = 0; r < R; r++) work += e->sc_host[(size_t)r].loop_iterations;
        // After a call of the latency kernel without its device clock (event log, no time limit, no trajectories) the device's
        // currentTime is still that call's START time: the rebuild is then not optional, whatever it costs, and its result goes
        // back to the device before the continued call reads it (time limit, trajectory grid, calls without a log).
        const bool stale = e->dev_clock_stale;
        const bool rebuild = e->direct_logs_valid && (work <= 50000000 || stale);
        if (stale && !rebuild)
            return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: the previous call ran without a device clock and left no event log to "
                                        "rebuild it from: set the state again (vgx_set_state) before continuing");
        const int64_t mism = e->clock_mismatches;
        for (int64_t r = 0; r < R; r++) {
            t0[(size_t)r] = e->sc_host[(size_t)r].currentTime;
            const bool ok = rebuild && host_clock(e, r) == VGX_OK && e->hc.exact;
            if (ok) t0[(size_t)r] = e->hc.final_time;
            else if (stale)
                return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: cannot rebuild the clock of replicate " + std::to_string(r) +
                                            " after a call without a device clock");
        }
        e->clock_mismatches = mism;   // (counted when a caller fetches the replicate)
        e->hc.rep = -1;
        if (stale) {
            for (int64_t r = 0; r < R; r++) e->sc_host[(size_t)r].currentTime = t0[(size_t)r];
            HIPCHECK(e, hipMemcpy(e->r_sc.p, e->sc_host.data(), (size_t)R * sizeof(VgxRepScalars), hipMemcpyHostToDevice));
            e->dev_clock_stale = false;
        }
        return VGX_OK;
    }

    // the window of the event log the call can write, the lockdown and first-attempt logs, the trajectory bins
    int size_logs() {
        // events.ptr / events.size as maintained by the caller's Events.CreateEvents (events.pxi:52-68)
        const int64_t ev_ptr0 = h.ev_ptr;
        ev_size = h.ev_size;
        if (ev_size < ev_ptr0) return fail(e, VGX_ERR_ARG, "vgx_simulate_direct: ev_size < ev_ptr");
        // every replicate's own events.ptr (one value after vgx_set_state; where each one stopped when the call continues)
        e->call_ev0.assign((size_t)R, ev_ptr0);
        if (!fresh_state && e->sc_host_valid && e->sc_host.size() == (size_t)R)
            for (int64_t r = 0; r < R; r++) e->call_ev0[(size_t)r] = e->sc_host[(size_t)r].ev_ptr;
        const int64_t ev_min = *std::min_element(e->call_ev0.begin(), e->call_ev0.end());
        // a Restart (pyx:414-415) rewinds the log to 0, so the device log must then cover [0, ev_size)
        const bool may_restart = ev_min <= 100 && iterations > 100;
        e->ev_base = may_restart ? 0 : ev_min;
        e->ev_ptr0 = ev_ptr0;
        evcap = o.record_events ? std::max<int64_t>(ev_size - e->ev_base, 1) : 1;
        // lockdown log: a population can switch on only if its threshold lies below its size, off only if it is on
        for (int64_t pn = 0; pn < P; pn++)
            if (e->h_startLD[(size_t)pn] * (double)e->sizes[(size_t)pn] < (double)e->sizes[(size_t)pn] || h.lockdownON[(size_t)pn] != 0)
                ld_possible = true;
        for (int64_t g = 0; g < e->n_sets && e->n_sets > 1; g++)   // ... under any of the parameter sets
            for (int64_t pn = 0; pn < P; pn++)
                if (e->sets_startLD[(size_t)(g * P + pn)] * (double)e->sizes[(size_t)pn] < (double)e->sizes[(size_t)pn]) ld_possible = true;
        e->loc_cap = ld_possible ? VGX_LOC_CAP : 1;
        e->fa_cap = (ld_possible && may_restart && o.record_events) ? VGX_FA_CAP : 0;
        int rc = 0;
        rc |= ensure(e, e->r_locrec, (size_t)(R * e->loc_cap * 2) * 4);
        rc |= ensure(e, e->r_loctime, (size_t)(R * e->loc_cap) * 8);
        rc |= ensure(e, e->r_lociter, (size_t)(R * e->loc_cap) * 8);
        rc |= ensure(e, e->r_farate, (size_t)(R * e->fa_cap) * 8);
        rc |= ensure(e, e->r_fakey, (size_t)(R * e->fa_cap) * 8);
        rc |= ensure(e, e->r_evrate, (size_t)(R * evcap) * 8);
        rc |= ensure(e, e->r_evcols, (size_t)(R * evcap * VGX_EV_COLS) * 4);
        if (o.traj_points > 0) rc |= ensure(e, e->r_traj, (size_t)(R * o.traj_points * P * 2) * 8);
        if (rc) return rc;
        e->evcap = evcap;
        e->traj_points = o.traj_points;
        e->last_ev_size = ev_size;
        return VGX_OK;
    }

    // the arguments every kernel takes, and what the host clock of this call starts from
    void fill_args() {
        a.p = e->dp;
        a.r = e->dr;
        a.r.ev_rate = (double *)e->r_evrate.p;
        a.r.ev_cols = (int32_t *)e->r_evcols.p;
        a.r.loc_rec = (int32_t *)e->r_locrec.p; a.r.loc_time = (double *)e->r_loctime.p; a.r.loc_iter = (int64_t *)e->r_lociter.p;
        a.r.loc_cap = e->loc_cap;
        a.r.fa_rate = (double *)e->r_farate.p; a.r.fa_key = (int64_t *)e->r_fakey.p; a.r.fa_cap = e->fa_cap;
        // the host clock starts where the caller's state stands (one value for all replicates after vgx_set_state; the
        // replicates' own device clocks when a call continues without a new state)
        e->call_t0 = cont_t0;
        e->call_recorded = o.record_events != 0;
        e->call_has_tlimit = !(time == -1.0f);
        e->call_tlimit = (double)time;
        e->hc.rep = -1;
        a.r.evcap = evcap;
        a.r.ev_base = e->ev_base;
        a.r.traj = o.traj_points > 0 ? (double *)e->r_traj.p : nullptr;
        a.r.traj_points = o.traj_points;
        a.r.traj_t0 = o.traj_t0;
        a.r.traj_dt = o.traj_points > 1 ? (o.traj_t1 - o.traj_t0) / (double)(o.traj_points - 1) : 0.0;
        a.n_replicates = R;
        a.iterations = iterations; a.sample_size = sample_size; a.attempts = attempts; a.time = time;
        a.ev_size = ev_size;
        a.max_loop = o.max_loop_factor * std::max<int64_t>(iterations, 1) + (1 << 20);
        a.record_events = o.record_events ? 1 : 0;
        a.lds_bytes = (int32_t)lds;
        dev_clock = e->call_has_tlimit || o.traj_points > 0 || !o.record_events;
    }

    // what vgx_choose_direct reads, from the engine; the one place that reads the choice's two environment variables
    void fill_shape() {
        vgx_direct_shape &s = shape;
        s.P = P; s.H = e->d.hapNum; s.S = e->d.susNum; s.sites = e->d.sites; s.R = R;
        s.C = e->max_C(); s.CB = e->max_CB(); s.cap = e->cap;
        s.param_sets = e->n_sets;
        s.n_seg = (int64_t)e->h_seg_par.size(); s.n_solo_seg = (int64_t)e->h_so_sn.size();
        s.solo_npass0 = e->h_so_npass0; s.solo_npass1 = e->h_so_npass1;
        s.solo_ncls = e->h_so_ncls; s.solo_maxnnz = e->h_so_maxnnz;
        s.start_lone_rows = e->start_lone_rows; s.start_max_nocc = e->start_max_nocc;
        double hosts = 0.0;
        s.tot_sus_is_sus = s.S == 1;
        for (int64_t pn = 0; pn < P; pn++) {
            s.max_size = std::max(s.max_size, e->sizes[(size_t)pn]);
            hosts += (double)e->sizes[(size_t)pn];
            if (s.S == 1 && h.totalSusceptible[(size_t)pn] != h.susceptible[(size_t)pn]) s.tot_sus_is_sus = 0;
        }
        s.hosts_below_2p53 = hosts < 9007199254740992.0;
        s.ld_possible = ld_possible;
        s.recomb = e->recombination != 0.0;
        s.fresh_state = fresh_state;
        s.suscep_cumul0_zero = e->suscepCumul[0] == 0.0;
        s.have_counts32 = e->dr.lcnt32 != nullptr;
        s.no_lone = getenv("VGX_NO_LONE") != nullptr;
        s.solo_general = getenv("VGX_SOLO_GENERAL") != nullptr;
    }

    int choose() {
        e->call_philox = o.mode == 2;      // the last direct call drew from the counter-based stream (the host clock must too)
        fill_shape();
        std::string msg;
        const int rc = vgx_choose_direct(&shape, &o, &plan, msg);
        if (rc) return fail(e, rc, msg);
        a.fast = (int32_t)plan.fast;
        a.rng_philox = (int32_t)plan.philox;
        return VGX_OK;
    }

    // what the chosen kernel needs beyond the state: the recombination log, the lane kernel's dense state, the row kernels' tables
    int alloc_workspace() {
        a.r.rec = nullptr; a.r.rec_cap = 0;
        e->rec_cap = 0;
        if (shape.recomb) {
            // every recorded event can be a recombinant birth; failed attempts (<= 100 events each) keep their records
            const int64_t rec_cap = evcap + 101 * std::max<int64_t>(attempts, 1);
            DIRECT_TRY(ensure(e, e->r_rec, (size_t)(R * rec_cap * 5) * 8));
            a.r.rec = (int64_t *)e->r_rec.p; a.r.rec_cap = rec_cap;
            e->rec_cap = rec_cap;
        }
        const int64_t H = shape.H, S = shape.S, k = plan.kernel;
        if (k == VGX_K_LANES) {
            const int64_t PH = P * H;
            const int64_t n_i = PH + P * S + 3 * P, n_d = P + 3 * PH + PH * S + P * S + 5 * P + P * P;
            DIRECT_TRY(ensure(e, e->r_lanews, (size_t)((n_i + n_d) * R) * 8));
            int64_t *wi = (int64_t *)e->r_lanews.p;
            ws.inf = wi; wi += PH * R; ws.sus = wi; wi += P * S * R; ws.totS = wi; wi += P * R; ws.totI = wi; wi += P * R; ws.lock = wi; wi += P * R;
            double *wd = (double *)wi;
            ws.cd = wd; wd += P * R; ws.birth = wd; wd += PH * R; ws.tE = wd; wd += PH * R; ws.hpr = wd; wd += PH * R;
            ws.shpr = wd; wd += PH * S * R; ws.immSrc = wd; wd += P * S * R; ws.infP = wd; wd += P * R; ws.immP = wd; wd += P * R;
            ws.popR = wd; wd += P * R; ws.migR = wd; wd += P * R; ws.maxEBM = wd; wd += P * R; ws.effMig = wd; wd += P * P * R;
        }
        e->last_kernel = k;
        if (k == VGX_K_QUADG) DIRECT_TRY(ensure(e, e->r_cold, (size_t)(R * P * (3 * S + e->CB)) * 8));
        if (k == VGX_K_QUAD || k == VGX_K_QUADG || k == VGX_K_QUADF || k == VGX_K_LONE) {
            int rcq = 0;
            rcq |= ensure(e, e->r_qeff, (size_t)(P * P) * 8);
            rcq |= ensure(e, e->r_qmebm, (size_t)P * 8);
            rcq |= ensure(e, e->r_qflag, 8);
            if (rcq) return rcq;
        }
        return VGX_OK;
    }

    // the extra arguments of the chosen kernel
    void fill_kernel_args() {
        exact_rcp_div = getenv("VGX_SOLO_PLAIN_DIV") ? 0 : 1;
        if (plan.kernel == VGX_K_SOLO) {
            soa.mig_in_lds = (int32_t)plan.solo_mig_in_lds;
            soa.seg_sn = (const int32_t *)e->so_sn.p; soa.seg_sig = (const double *)e->so_sig.p; soa.nseg = (int32_t)e->h_so_sn.size();
            soa.rcpAs = (const double *)e->so_rcp.p;
            soa.tseg_par = (const int32_t *)e->q_segpar.p; soa.tseg_sn = (const int32_t *)e->q_segsn.p; soa.tseg_sig = (const double *)e->q_segsig.p;
            soa.cb_seg = (const int32_t *)e->q_cbseg.p; soa.pass = (const int32_t *)e->so_pass.p;
            soa.tnseg = (int32_t)e->h_seg_par.size(); soa.npass0 = e->h_so_npass0; soa.npass1 = e->h_so_npass1;
            soa.exact_rcp_div = exact_rcp_div;
            soa.hap_cls = (const int32_t *)e->so_hapcls.p; soa.cls_nnz = (const int32_t *)e->so_nnz.p; soa.cls_tsn = (const int32_t *)e->so_tsn.p;
            soa.cls_tsig = (const double *)e->so_tsig.p; soa.cls_sigma = (const double *)e->so_clssig.p;
            soa.n_cls = e->h_so_ncls;
            soa.maxterms = (int32_t)(e->h_so_maxnnz * P);
            soa.compact = (int32_t)plan.solo_compact;
        }
        if (plan.kernel == VGX_K_LONE) {
            loa.lds_bytes = (int32_t)plan.lone_lds_bytes;
            loa.general = (int32_t)plan.lone_general;
            loa.effMig = (const double *)e->r_qeff.p; loa.maxEBM = (const double *)e->r_qmebm.p; loa.has_mig = (const int32_t *)e->r_qflag.p;
            loa.rcpAs = (const double *)e->so_rcp.p;
            loa.exact_rcp_div = exact_rcp_div;
            loa.mut_uniform = (e->h_mut_uniform && !getenv("VGX_LONE_NO_MUTUNI")) ? 1 : 0;
            loa.seg_par = (const int32_t *)e->q_segpar.p; loa.seg_sn = (const int32_t *)e->q_segsn.p;
            loa.seg_sig = (const double *)e->q_segsig.p; loa.cb_seg = (const int32_t *)e->q_cbseg.p;
            loa.nseg = (int32_t)e->h_seg_par.size();
        }
        if (plan.kernel == VGX_K_QUADG) {
            qga.effMig0 = (const double *)e->r_qeff.p; qga.mebm0 = (const double *)e->r_qmebm.p; qga.has_mig0 = (const int32_t *)e->r_qflag.p;
            qga.cd0 = (const double *)e->s_cd.p;
            qga.seg_par = (const int32_t *)e->q_segpar.p; qga.seg_sn = (const int32_t *)e->q_segsn.p;
            qga.seg_sig = (const double *)e->q_segsig.p; qga.cb_seg = (const int32_t *)e->q_cbseg.p;
            qga.nseg = (int32_t)e->h_seg_par.size(); qga.W = (int32_t)(3 * shape.S + e->CB);
            qga.cold = (int64_t *)e->r_cold.p;
        }
    }

    // the copy of the counts the kernel reads: the 4-byte one is kept by the one-class row kernels alone
    // (both forms of the exact row kernel work on the 4-byte counts alone, like the kernels the plan marks leaves32: the 8-byte counts
    // are widened on demand, by the next kernel that reads them or by vgx_get_state)
    bool on_counts32() const { return plan.leaves32 || plan.kernel == VGX_K_QUAD; }
    int sync_counts() {
        const bool row32 = plan.kernel == VGX_K_QUAD || plan.kernel == VGX_K_QUADF;
        if (!e->counts64_valid && !(on_counts32() && e->counts32_valid)) {
            HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, R * P * e->cap, e->stream));
            e->counts64_valid = true;
        }
        if (row32 && !e->counts32_valid) {
            HIPCHECK(e, vgxi_launch_counts32(e->dr.lcnt, e->dr.lcnt32, R * P * e->cap, e->stream));
            e->counts32_valid = true;
        }
        return VGX_OK;
    }

    // (which copy of the counts the kernel leaves current is recorded once it has been enqueued: a failure before that leaves the flags
    // describing what is on the device; whatever a failed launch may have touched is rebuilt from the host state, by the next call)
    int launch() {
        const double *cd0 = (const double *)e->s_cd.p;
        double *qeff = (double *)e->r_qeff.p, *qmebm = (double *)e->r_qmebm.p;
        int32_t *qflag = (int32_t *)e->r_qflag.p;
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        switch (plan.kernel) {
        case VGX_K_SOLO: HIPCHECK(e, vgxi_launch_solo(&a, &soa, dev_clock ? 1 : 0, e->stream)); break;
        case VGX_K_LONE:
            HIPCHECK(e, vgxi_launch_quad_prep(&a.p, cd0, qeff, qmebm, qflag, e->stream));
            HIPCHECK(e, vgxi_launch_lone(&a, &loa, dev_clock ? 1 : 0, e->stream));
            break;
        case VGX_K_LANES: HIPCHECK(e, vgxi_launch_lanes(&a, &ws, e->stream)); break;
        case VGX_K_QUAD: HIPCHECK(e, vgxi_launch_quad(&a, cd0, qeff, qmebm, qflag, (int)plan.long_lists, exact_rcp_div ? 0 : 1, e->stream)); break;
        case VGX_K_QUADF: HIPCHECK(e, vgxi_launch_quadf(&a, cd0, qeff, qmebm, qflag, e->stream)); break;
        case VGX_K_QUADG:
            HIPCHECK(e, vgxi_launch_quad_prep(&a.p, cd0, qeff, qmebm, qflag, e->stream));
            HIPCHECK(e, vgxi_launch_quadg(&a, &qga, e->stream));
            break;
        default:
            if (e->n_sets > 1)
                HIPCHECK(e, vgxi_launch_direct_sets(&a, (const VgxDevParams *)e->ps_blocks.p, (const int32_t *)e->ps_setof.p, lds, e->stream));
            else
                HIPCHECK(e, vgxi_launch_direct(&a, lds, e->stream));
            break;
        }
        e->counts32_valid = plan.kernel == VGX_K_QUAD || plan.kernel == VGX_K_QUADF;
        if (on_counts32()) e->counts64_valid = false;
        e->dev_clock_stale = (plan.kernel == VGX_K_SOLO || plan.kernel == VGX_K_LONE) && !dev_clock;
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if (hipStreamSynchronize(e->stream) != hipSuccess) {
            e->dev_state_valid = false;     // a kernel that did not finish leaves no state to continue from
            return fail(e, VGX_ERR_HIP, std::string("vgx_simulate_direct: kernel failed: ") + hipGetErrorString(hipGetLastError()));
        }
        HIPCHECK(e, hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1));
        e->last_launches = 1;
        return VGX_OK;
    }

    // the replicates' scalars back on the host; a replicate's error is the call's
    int collect() {
        e->sc_host.resize((size_t)R);
        HIPCHECK(e, hipMemcpy(e->sc_host.data(), e->r_sc.p, (size_t)R * sizeof(VgxRepScalars), hipMemcpyDeviceToHost));
        e->sc_host_valid = true;
        if (plan.kernel == VGX_K_LONE && o.kernel == 0) {
            // The lists of some replicate outgrew the LDS heap: the call is a function of the state and the seeds, so it runs again from the
            // state of vgx_set_state on the row kernel (the automatic choice takes this kernel only on such a state).
            for (int64_t r = 0; r < R; r++) heap_full = heap_full || e->sc_host[(size_t)r].error == (VGX_ERR_CAPACITY | (VGX_LONE_FULL_SITE << 8));
            if (heap_full) {
                if (getenv("VGX_TIMING")) fprintf(stderr, "vgx_lone: LDS heap full, the call runs again on the row kernel\n");
                e->dev_state_valid = false;
                e->sc_host_valid = false;
                e->lone_fallbacks += 1;
                return VGX_OK;
            }
        }
        e->direct_logs_valid = e->call_recorded;
        // the caller's next simulate continues from where replicate 0 stopped unless it sets a new state
        h.ev_ptr = e->sc_host[0].ev_ptr;
        for (int64_t r = 0; r < R; r++) {
            int64_t er = e->sc_host[(size_t)r].error;
            if (er) {
                const int64_t where = er >> 8;   // the quad kernel tags the site of a zero-weight alert (diagnostics)
                er &= 255;
                const char *what = er == VGX_ERR_ZERO_WEIGHT ? "zero weight sampled (fastChoose alert)"
                                   : er == VGX_ERR_CAPACITY  ? "capacity exceeded (occupancy list / event or lockdown log)"
                                   : er == VGX_ERR_LOOP_GUARD ? "loop guard tripped"
                                                              : "kernel error";
                return fail(e, (int)er, std::string("vgx_simulate_direct: replicate ") + std::to_string(r) + ": " + what +
                                            (where ? " [site " + std::to_string(where) + "]" : std::string()));
            }
        }
        return VGX_OK;
    }

    int run() {
        DIRECT_TRY(check_call());
        DIRECT_TRY(ensure_device_state());
        DIRECT_TRY(continue_clock());
        DIRECT_TRY(size_logs());
        fill_args();
        DIRECT_TRY(choose());
        DIRECT_TRY(alloc_workspace());
        fill_kernel_args();
        DIRECT_TRY(sync_counts());
        DIRECT_TRY(launch());
        return collect();
    }
};

// One pass, or two: when the automatic choice took vgx_lone.hip and its LDS heap filled up, the call runs once more from the state of
// vgx_set_state as the first pass's plan says (a row kernel or the wavefront kernel: that pass cannot ask for a third).
int direct_core(vgx_engine *e, int64_t iterations, int64_t sample_size, float time, int64_t attempts,
                const vgx_run_opts *opts) {
    vgx_run_opts o{};
    o.record_events = 1;
    if (opts) o = *opts;
    DirectRun first{e, e->hs, e->d.popNum, e->R, iterations, sample_size, attempts, time, o};
    const int rc = first.run();
    if (rc || !first.heap_full) return rc;
    vgx_run_opts again = first.o;
    again.kernel = first.plan.fallback_kernel;
    again.mode = first.plan.fallback_mode;
    DirectRun second{e, e->hs, e->d.popNum, e->R, iterations, sample_size, attempts, time, again};
    return second.run();
}

extern "C" int vgx_simulate_direct(vgx_engine *e, int64_t iterations, int64_t sample_size, float time,
                                   int64_t attempts, const vgx_run_opts *opts) {
    if (!e) return VGX_ERR_ARG;
    e->last_was_tau = false;
    return direct_core(e, iterations, sample_size, time, attempts, opts);
}
