/*
 * vgx.h — C ABI of the MI355X-native forward epidemic simulation engine (libvgx.so).
 *
 * This is the drop-in boundary for ONE path of Genomics-HSE/VGsim: the two native entry points that
 * `Simulator.simulate` calls on its engine object (reference src/_interface.py:821-829):
 *     BirthDeathModel.SimulatePopulation      (src/_BirthDeath.pyx:396-429, direct Gillespie)
 *     BirthDeathModel.SimulatePopulation_tau  (src/_BirthDeath.pyx:2293-2346, Poisson tau-leaping)
 * plus what the caller needs to hand the model over and read the results back.  Plain pointers and
 * sizes only; every array is a C-contiguous host buffer with the reference's own name, dtype and shape
 * (numpy arrays of the reference's `cdef class BirthDeathModel`, pyx:47-68).  A binding for the
 * reference (ctypes, or `cdef extern` from Cython) is shown in INTEGRATION.md.
 *
 * One engine = one model shape and `n_replicates` independent trajectories of it (replicate = one
 * seeded run; the classic API uses 1).  Engines are independent; calls on one engine must not overlap.
 * Every function returns VGX_OK (0) or an error code; vgx_last_error() gives the message.
 *
 * Environment switches read by the library (diagnostics and tests; none is needed in production):
 *   VGX_LIST_CAP=n                 caps the capacity of every occupancy list at n entries (exercises the kernels' overflow paths)
 *   VGX_TIMING=1                   vgx_simulate_tau prints its host-side phases on stderr
 *   VGX_SOLO_PLAIN_DIV=1           single-trajectory kernels and the exact row kernel: x / actualSizes by the compiler's division instead of
 *                                  the reciprocal sequence
 *   VGX_SOLO_GENERAL=1             ... its general BirthRate layout where the compact one would be taken
 *   VGX_SOLO_NO_UNIT=1             ... no one-haplotype / one-population instantiation
 *   VGX_TAU_STEP_KERNELS=1 / 0     tau: always / never the step kernels (default: the on-device step loop for small models)
 *   VGX_TAU_NO_BYTE_DRIFT=1        tau: the two-pass drift instead of the pass on the one-byte counts
 *   VGX_TAU_NO_FRONT=1             tau: no front pass of a try (the compartments that can fall below zero on their own drawn first)
 *   VGX_TAU_NO_OCCLIST=1           tau: a try's scan and front pass always stream all compartments (no lists of the occupied ones)
 *   VGX_TAU_NO_FRONT_ALONE=1       tau, one replicate: the front pass is enqueued together with the try proper, not ahead of it
 *   VGX_TAU_LARGE_MODEL_THRESHOLDS=1  tau: the draw thresholds of large models on a small one
 *   VGX_GENEALOGY_CHUNK_BYTES=n    vgx_get_genealogies, vgx_get_tau_genealogies: device bytes of workspace per pass (several passes)
 *   VGX_TIMELINES_LDS_BYTES=n      vgx_get_timelines, vgx_get_tau_timelines: LDS budget of a replay workgroup (default 65536, at most 163840; the
 *                                  queries are split over launches)
 *   VGX_TIMELINES_CHUNK_BYTES=n    vgx_get_timelines, vgx_get_tau_timelines: device bytes of staging and outputs per chunk of replicates
 *   VGX_COLSUMMARY_CHUNK_BYTES=n   vgx_get_trajectory_summary, vgx_test_column_summary: device bytes of the transposed scratch per chunk of
 *                                  columns (default 2^28; one tile of 64 columns at the least)
 *   VGX_INCIDENCE_TILE_EVENTS=n    vgx_get_incidence / vgx_get_tau_incidence: consecutive events (rows) a counting workgroup takes (default 4096; no result depends on it)
 *   VGX_PREVALENCE_TILE_EVENTS=n   vgx_get_prevalence / vgx_get_tau_prevalence and vgx_get_susceptibles / vgx_get_tau_susceptibles: consecutive events (rows) a counting workgroup takes (default 4096; no result depends on it)
 *   VGX_MILESTONES_TILE_EVENTS=n   vgx_get_milestones: consecutive events a walking workgroup takes, and pass A's tile (default 4096; no result depends on it)
 *   VGX_MILESTONES_WAVES=4         vgx_get_milestones, diagnostic: four wavefronts per (replicate, tile) taking rounds in turn behind a barrier instead of one (same results)
 *   VGX_TAU_MILESTONES_TILE_ROWS=n vgx_get_tau_milestones: rows of a tile of whole events that a walking workgroup takes (default 4096; no result depends on it)
 *   VGX_TAU_MILESTONES_WAVES=4     vgx_get_tau_milestones, diagnostic: workgroups of four wavefronts (256 threads) instead of one (same results)
 *   VGX_FLOWS_TILE_EVENTS=n        vgx_get_flows / vgx_get_tau_flows: consecutive events (rows) a counting workgroup takes (default 4096; no result depends on it)
 *   VGX_FLOWS_FORM=dense|split     vgx_get_flows / vgx_get_tau_flows: the table a counting workgroup keeps in LDS, all popNum^2 * V cells or the diagonal alone
 *                                  (default: dense where it fits, else split; no result depends on it; a form that does not fit is refused)
 */
#ifndef VGX_H
#define VGX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgx_engine vgx_engine;

enum {
    VGX_OK = 0,
    VGX_ERR_ARG = 1,            /* bad argument / unsupported configuration */
    VGX_ERR_HIP = 2,            /* HIP runtime failure (no device, out of memory, launch failure) */
    VGX_ERR_ZERO_WEIGHT = 3,    /* fastChoose hit a zero weight: the reference prints and exits (fast_choose.pxi:5-13) */
    VGX_ERR_CAPACITY = 4,       /* occupancy list / lockdown log / multievent buffer capacity exceeded */
    VGX_ERR_LOOP_GUARD = 5,     /* iteration guard tripped (would be an endless loop upstream) */
    VGX_ERR_CLASSES = 6         /* more distinct per-haplotype rate rows than the engine supports */
};

/* Event types: src/events.pxi:2-8 */
enum { VGX_BIRTH = 0, VGX_DEATH = 1, VGX_SAMPLING = 2, VGX_MUTATION = 3, VGX_SUSCCHANGE = 4,
       VGX_MIGRATION = 5, VGX_MULTITYPE = 6 };

/* pyx:84-90: hapNum must equal 4^sites */
typedef struct vgx_dims {
    int64_t sites, hapNum, popNum, susNum;
} vgx_dims;

/* Model parameters (borrowed, copied by vgx_set_params).  Names, dtypes, shapes: pyx:157-204. */
typedef struct vgx_params {
    const double *bRate, *dRate, *sRate;         /* [H]            pyx:158-160 */
    const double *mRate;                         /* [H][sites]     pyx:161 */
    const double *hapMutType;                    /* [H][sites][3]  pyx:163 */
    const double *susceptibility;                /* [H][S]         pyx:162 */
    const int64_t *suscType;                     /* [H]            pyx:157 */
    const double *suscepTransition;              /* [S][S]         pyx:196 */
    const int64_t *sizes;                        /* [P]            pyx:173 */
    const double *contactDensityBeforeLockdown;  /* [P]            pyx:190 */
    const double *contactDensityAfterLockdown;   /* [P]            pyx:191 */
    const double *startLD, *endLD;               /* [P]            pyx:192-193 */
    const double *samplingMultiplier;            /* [P]            pyx:194 */
    const double *migrationRates;                /* [P][P]         pyx:198 (diagonal ignored: recomputed, pyx:290-295) */
} vgx_params;

/* Compartment state and scalars that persist between simulate() calls (pyx:34-38, 47-49).
 * In vgx_set_state the arrays are read; in vgx_get_state they are written (any may be NULL = skip). */
typedef struct vgx_state {
    int64_t *susceptible;          /* [P][S] */
    int64_t *infectious;           /* [P][H] */
    int64_t *initial_susceptible;  /* [P][S]  snapshot used by Restart (pyx:714-738) */
    int64_t *initial_infectious;   /* [P][H] */
    int64_t *totalSusceptible, *totalInfectious, *lockdownON; /* [P] */
    double *contactDensity;        /* [P]  current value (flips with lockdowns, pyx:698-710) */
    int64_t first_simulation;      /* pyx:34, 435-448 */
    int64_t globalInfectious;
    int64_t bCounter, dCounter, sCounter, mCounter, iCounter, swapLockdown, migPlus, migNonPlus;
    int64_t good_attempt;
    double currentTime, totalRate, totalMigrationRate, tau_l;
    int64_t ev_ptr, ev_size;       /* event-log position/capacity as maintained by Events.CreateEvents (events.pxi:52-68) */
} vgx_state;

/* Options of one simulate call beyond the reference's four arguments. */
typedef struct vgx_run_opts {
    int64_t record_events;   /* 1: keep the event log (default for the classic API); 0: counters/trajectories only */
    int64_t max_loop_factor; /* loop guard: at most max_loop_factor*iterations + 2^20 loop iterations (0 = 1024) */
    int64_t traj_points;     /* >0: bin totalInfectious/totalSusceptible[P] at this many uniform time points (direct and tau calls;
                                a grid point gets the totals before the event / step that takes the time past it) */
    double traj_t0, traj_t1; /* time window of the trajectory grid */
    int64_t mode;            /* direct path: 0 = EXACT (the reference's floating-point summation order, bit-exact log);
                                1 = FAST (order-free sums: class-aggregated infection rate, integer prefix search,
                                factored BirthRate, tree scans; same random stream and event semantics, identical
                                integer columns on the same seed); 2 = FAST with a counter-based random stream
                                (Philox4x32-10 keyed by the seed, counter = (draw index, attempt): every draw can be formed
                                on its own; other numbers than PCG64's, so another trajectory of the same law).  Ignored by
                                vgx_simulate_tau. */
    int64_t kernel;          /* direct path: 0 = automatic, 1 = one replicate per wavefront (vgx_direct.hip: every model, every mode),
                                2 = one replicate per lane (vgx_lanes.hip; small models: popNum <= 16, popNum*hapNum <= 1024,
                                susNum <= 8, mode 0),
                                3 = four replicates per wavefront, one per 16-lane row: for popNum <= 64, one susceptibility group,
                                one rate class, no possible lockdown switch and no recombination vgx_quad.hip in mode 0 and the FAST
                                row kernel vgx_quadf.hip in modes 1 and 2, else the general form vgx_quadg.hip (popNum <= 128,
                                susNum <= 8, <= 64 rate classes, <= 16 transmission/susceptibility classes; also models with a
                                recombination probability; mode 0, and mode 2 as exact arithmetic on the counter-based stream);
                                4 = the general form even where 3 would take another (mode 0; mode 2 only for models outside the
                                one-class scope);
                                5 = one replicate per wavefront with the whole DENSE model in LDS and registers (vgx_solo.hip: the
                                latency kernel of single trajectories; hapNum <= 64, popNum <= 128, susNum <= 16; modes 0 and 2).
                                Automatic: 5 for fewer than 2048 replicates of a model it takes (and for more where it beats 3 / 4:
                                small models with several classes, one-class models below 8192 replicates — in mode 2 at every size);
                                6 = one replicate per wavefront with the occupancy LISTS in LDS (vgx_lone.hip: single trajectories of
                                large haplotype spaces; popNum <= 64; modes 0 and 2, both of its forms; automatic up to 1536 replicates
                                of models 5 does not take, on a state that came through vgx_set_state);
                                2 automatically for P*H*S <= 4 from 131072 replicates in mode 0.
                                Where an exact kernel serves the request, the call runs in mode 0 whatever was asked for: mode 1 with
                                kernel 0 on a model outside the one-class scope that 4 takes (4, 5 or 6 then runs it: their output
                                is what FAST promises); mode 2 with kernel 0, 5 or 6 on every model without recombination, and with 3 or 4 on a model
                                outside the one-class scope that 4 takes — exact arithmetic on the counter-based stream.  A request
                                that then lands on 1 or on the FAST row kernel keeps its own mode.  Recombination: mode 0 only.
                                tests/test_direct_plan.py has the table. */
    int64_t reserved[2];     /* [0] tau path: 1 = run every try of the halving loop (pyx:2316-2321) instead of starting at the
                                first try that is not certain to be rejected (same accepted steps either way);
                                2 = with several parameter sets installed (vgx_set_param_sets): run every replicate under its own
                                set on the on-device step loop (without it such a call is refused; ignored with one set);
                                [1] tau path, how a try's deltas are kept and checked (same draws and decisions in every mode):
                                0 = sparse (default): a list of moves, own deltas checked where they are drawn, no dense arrays;
                                2 = dense delta arrays written by every try, the fused own-delta / arrival tests;
                                1 = dense arrays and the bounds check (pyx:2522-2528) as one pass over all compartments */
} vgx_run_opts;

/* Per-replicate results of the last simulate call. */
typedef struct vgx_counters {
    int64_t ev_ptr;                /* events.ptr after the call */
    int64_t ev_first_new;          /* first log index written by this call (0 if a Restart rewound the log) */
    int64_t loop_iterations;       /* loop iterations incl. rejected migrations (each draws 2 uniforms) */
    int64_t restarts;
    int64_t lockdown_records;
    int64_t error;                 /* VGX_* code raised inside the kernel for this replicate */
    int64_t multievent_rows;       /* tau: rows appended to the multievent log by this call */
    int64_t reserved[5];           /* [0] tau: events drawn; direct: [1] index of the last attempt that drew random
                                      numbers (-1 none), [2] its loop iterations (2 uniforms each); both: [4] sCounter
                                      (the cases sampled); [3] tau: tries of the halving loop left out as certain rejections */
} vgx_counters;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int vgx_create(const vgx_dims *dims, int64_t n_replicates, int device, vgx_engine **out);
void vgx_destroy(vgx_engine *e);
const char *vgx_last_error(const vgx_engine *e);   /* e may be NULL: message of the last failed vgx_create */
int vgx_device_count(void);

/* ---- model hand-over ------------------------------------------------------------------------ */
int vgx_set_params(vgx_engine *e, const vgx_params *p);
/* Scenario ensembles: n_sets parameter sets over the one start state of vgx_set_state, and for every replicate the set it runs under.
 * Replicate r of the next vgx_simulate_direct call is, bit for bit, the run of an engine that was given sets[set_of[r]] through
 * vgx_set_params, the same state and seed r: one launch of the one-replicate-per-wavefront kernel runs all of them, every wavefront
 * reading its own set's tables (classes of identical rate rows, actualSizes, the recomputed migration diagonal, suscepCumul,
 * maxEffectiveBirth are built per set).  So is replicate r of a vgx_simulate_tau call that asks for the sets
 * (vgx_run_opts.reserved[0] = 2; a call that does not is refused, as every tau call under sets used to be), where the on-device
 * step loop runs it
 * (one workgroup per replicate, every workgroup under its own set: compartments, counters, times, restarts, lockdown state and
 * records, multievent rows, step times and trajectories equal that engine's run on the on-device loop; the preparation's lockdown
 * check, swapLockdown and the non-zero-rate guards of the start and of a Restart are each set's own).  n_sets == 1 is vgx_set_params(e, &sets[0]); a later vgx_set_params returns the engine to one
 * set.  Like vgx_set_params the call invalidates the device state.  Dimensions, start state and recombination settings are the
 * engine's, shared by all sets; so `sizes` must be bitwise equal in all sets (VGX_ERR_ARG otherwise).  One value of the state is a
 * set's own: a replicate starts with contactDensityAfterLockdown of its set in the populations whose lockdownON is set in the start
 * state and contactDensityBeforeLockdown in the others (what a model with that set's parameters holds there); vgx_state's
 * contactDensity is the start value while one set is installed.  VGX_ERR_CLASSES and the LDS
 * limit of the kernel's tables are reported for the set that exceeds them, by its index.  vgx_get_state, the event and lockdown
 * logs, vgx_get_genealogies, vgx_get_timelines and the trajectories read logs and state only and work unchanged.
 * Limits while more than one set is installed (each refused with VGX_ERR_ARG and a message naming it): vgx_simulate_direct runs in
 * mode 0 on kernel 0 or 1 only (the row, latency and lane kernels, FAST and the counter-based stream read one shared parameter
 * copy).  vgx_simulate_tau runs only when vgx_run_opts.reserved[0] = 2 asks for it, and then on the on-device step loop only, whatever the ensemble's size (the step kernels of large states
 * read one shared copy), and is refused where that loop does not run, the message naming the number: popNum * hapNum above 8192,
 * popNum above 64, susNum above 8, more than 15 sites, more than 256 rate classes or 64 transmission classes in the largest set,
 * more than 150 KiB of LDS per replicate, VGX_TAU_STEP_KERNELS=1, VGX_TAU_LARGE_MODEL_THRESHOLDS=1, the step kernels' validation
 * modes (vgx_run_opts.reserved[1]), or a step log (replicates x steps x 24 bytes) above 8e9 bytes.  A refused call leaves the engine
 * usable.  vgx_stage_tau is refused.  The tau getters (states, multievent rows, lockdowns, timelines, genealogies, incidence,
 * prevalence, susceptibles, milestones, flows) read logs and state only and work unchanged.
 * Device memory: one copy of every parameter array per set. */
int vgx_set_param_sets(vgx_engine *e, int64_t n_sets, const vgx_params *sets /* [n_sets] */,
                       const int32_t *set_of /* [n_replicates], values in [0, n_sets) */);
/* Recombination branch of Birth (pyx:575-596): `recombination_probability` (pyx:93, set_coinfection_parameters
 * pyx:1422-1426), `genome_length` (pyx:1409-1417) and sitesPosition[sites] (pyx:98-101, set_mutation_position
 * pyx:1516-1524).  Optional: without this call the probability is 0 and the branch is never taken.  With a non-zero
 * probability direct runs are exact mode only and take the single-trajectory kernel (few replicates of a small model), the general
 * four-replicates-per-wavefront kernel (its *_rec instantiations) or the one-replicate-per-wavefront kernel (any shape). */
int vgx_set_recombination(vgx_engine *e, double recombination_probability, int64_t genome_length,
                          const int64_t *sitesPosition /* [sites], may be NULL when the probability is 0 */);
/* The same state is given to every replicate; replicates differ by their seed only (and, after vgx_set_param_sets, by their
 * parameter set). */
int vgx_set_state(vgx_engine *e, const vgx_state *s);
int vgx_get_state(vgx_engine *e, int64_t replicate, vgx_state *out);
/* user_seed of each replicate: the RNG of attempt k is PCG64(SeedSequence(seed, spawn_key=(k,))),
 * the stream RndmWrapper(seed=(user_seed, k)) creates at pyx:403 / pyx:2310. */
int vgx_set_seeds(vgx_engine *e, const int64_t *seeds /* [n_replicates] */);

/* Optional: puts the state of vgx_set_state on the device in the tau kernels' layout ahead of vgx_simulate_tau (first-call snapshot of
 * PrepareParameters pyx:435-448, conversion and upload of the P x H counts of every replicate), so that a caller who times the simulate
 * call finds its inputs resident.  Valid until the next vgx_set_state / vgx_set_params / simulate call; vgx_simulate_tau does the same
 * work itself when this was not called. */
int vgx_stage_tau(vgx_engine *e);

/* ---- the hot path --------------------------------------------------------------------------- */
/* Replaces BirthDeathModel.SimulatePopulation(iterations, sample_size, float time, attempts), pyx:396. */
int vgx_simulate_direct(vgx_engine *e, int64_t iterations, int64_t sample_size, float time, int64_t attempts,
                        const vgx_run_opts *opts /* may be NULL */);
/* Replaces BirthDeathModel.SimulatePopulation_tau(iterations, sample_size, float time, attempts), pyx:2293. */
int vgx_simulate_tau(vgx_engine *e, int64_t iterations, int64_t sample_size, float time, int64_t attempts,
                     const vgx_run_opts *opts /* may be NULL */);

/* ---- results -------------------------------------------------------------------------------- */
int vgx_get_counters(vgx_engine *e, int64_t replicate, vgx_counters *out);
/* All replicates at once: out[replicate][4] = ev_ptr, loop_iterations, restarts, tau events drawn. */
int vgx_get_counters_all(vgx_engine *e, int64_t *out);
/* Copies log rows [first, first+count) into the caller's Events arrays (events.pxi:26-29). */
int vgx_get_events(vgx_engine *e, int64_t replicate, int64_t first, int64_t count, double *times,
                   int64_t *types, int64_t *haplotypes, int64_t *populations, int64_t *newHaplotypes,
                   int64_t *newPopulations);
/* Lockdown switches recorded by the last call (models.pxi:52-66): up to `cap` rows, returns the count in *n. */
int vgx_get_lockdowns(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *states, int64_t *populations,
                      double *times, int64_t *n);
/* Forward recombination records of the last direct call (Recombination.AddRecombination_forward, models.pxi:82-89):
 * event index, parent haplotypes hi and hi2, recombinant haplotype, breakpoint.  Like upstream, records of failed
 * attempts stay in the list (Restart does not clear `rec`, pyx:714-738). */
int vgx_get_recombinations(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *idevents, int64_t *his,
                           int64_t *hi2s, int64_t *nhis, int64_t *posRecombs, int64_t *n);
/* Tau multievents of the last call (events.pxi:105-152), rows with num > 0 only. */
/* Rejected tries (halvings of tau_l, pyx:2316-2321) of steps [first, first + count) of the last vgx_simulate_tau call: the leap a step
 * made times 2^tries is the tau ChooseTau (pyx:2432-2450) gave it. */
int vgx_get_tau_tries(vgx_engine *e, int64_t replicate, int64_t first, int64_t count, int32_t *out);
int vgx_get_multievents(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *num, double *times, int64_t *types,
                        int64_t *haplotypes, int64_t *populations, int64_t *newHaplotypes,
                        int64_t *newPopulations, int64_t *n);
/* The rows of ALL replicates of the last tau call in one read-out: offsets[r] .. offsets[r + 1] are the rows of replicate r in `rows`
 * ([.][6]: num, type, haplotype, population, newHaplotype, newPopulation, in the order the device appended them) and `steps` (the step
 * of the call, 0-based, a row belongs to; may be NULL).  rows == NULL: only `offsets` ([R + 1]) is filled (sizing); cap: rows there is room for. */
int vgx_get_multievents_all(vgx_engine *e, int64_t cap, int64_t *offsets, int64_t *rows, int64_t *steps);
/* The states of ALL replicates after the last tau call: infectious [R][P][H], susceptible [R][P][S], counters [R][8] (bCounter, dCounter,
 * sCounter, mCounter, iCounter, migPlus, globalInfectious, ev_ptr), times [R] (currentTime); each may be NULL. */
int vgx_get_tau_states_all(vgx_engine *e, int64_t *infectious, int64_t *susceptible, int64_t *counters, double *times);
/* Summary trajectories of the last call (direct or tau; an error when it recorded none): out[replicate][point][population][0=infectious,
 * 1=susceptible], f64.
 * `out` is a host pointer, or a device pointer when out_is_device != 0 (e.g. a torch tensor for an RCCL gather). */
int vgx_get_trajectories(vgx_engine *e, double *out, int out_is_device);
/* The same trajectories as 32-bit integers written to a DEVICE buffer of the same shape (compartment totals are whole numbers;
 * refused when a population size is 2^31 or more): the wire format of the ensemble gather, formed without an f64 copy. */
int vgx_get_trajectories_int(vgx_engine *e, int32_t *out_device);
/* Direct calls with a time limit take their `currentTime < time` stop decisions (pyx:407) on the device clock; event times are
 * rebuilt on the host with libm.  Number of replicates (fetched so far) for which the two clocks disagreed on one such
 * decision (an event time within rounding of the limit): the run reported is then the device clock's. */
int64_t vgx_clock_mismatches(const vgx_engine *e);

/* ---- backward pass ------------------------------------------------------------------------- */
/* Replaces BirthDeathModel.GetGenealogy(seed) (pyx:743-1000) with its recorders Mutations / Migrations
 * (models.pxi:1-48): one backward walk over the event log that coalesces the sampled lineages.  Host code (no
 * device, no engine handle needed).  `infectious` is walked back in place exactly as the reference does. */
typedef struct vgx_genealogy_io {
    int64_t popNum, hapNum;
    int64_t sCounter;                      /* number of samples; the tree has 2*sCounter-1 nodes */
    /* event log (events.pxi:24-68) */
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    /* multievent rows (events.pxi:105-152) referenced by MULTITYPE events as [haplotypes, populations); may be NULL */
    int64_t mev_rows;
    const int64_t *mev_num; const double *mev_times;
    const int64_t *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t *infectious;                   /* [P][H], state at the end of the simulation (in/out) */
    /* PCG64 position of the reference's self.seed: state hi, lo, increment hi, lo + numpy's buffered 32-bit half */
    uint64_t rng_state[4];
    int64_t rng_has_uint32;
    uint64_t rng_uinteger;
    /* outputs, caller-allocated */
    int64_t *tree, *tree_pop; double *times;            /* [2*sCounter-1]: parent (-1 = root), population, time */
    int64_t mut_cap, mut_n; int64_t *mut_node, *mut_AS, *mut_DS, *mut_site; double *mut_time;
    int64_t mig_cap, mig_n; int64_t *mig_node, *mig_old, *mig_new; double *mig_time;
    int64_t nodes_used;
} vgx_genealogy_io;
int vgx_get_genealogy(vgx_genealogy_io *io, char *errbuf, int64_t errcap);
/* (state, inc) of PCG64(SeedSequence(seed, spawn_key=(attempt,))) after `draws` outputs: where the reference's
 * self.seed stands when GetGenealogy(seed=None) continues the simulation's stream (pyx:766-767). */
void vgx_rng_position(int64_t seed, int64_t attempt, int64_t draws, uint64_t out[4]);

/* The same backward pass for many replicates of the last vgx_simulate_direct call at once, on the device: one walk per
 * replicate over the device event log in place (the log is not copied to the host), started from the replicate's final
 * state; event times from the host clock (the times vgx_get_events gives).  For every selected replicate the result is
 * what vgx_get_genealogy returns on that replicate's chain, state and start position: tree, tree_pop, times, the
 * mutation and migration records, nodes_used and the final generator state.  Direct chains only (refused after
 * vgx_simulate_tau or a call without an event log); every selected replicate's chain must start at log index 0
 * (vgx_counters.ev_first_new == 0).  Two calls:
 *   1. sizing: tree == NULL.  Fills node_off, mut_off, mig_off [n+1] with the capacities the walk needs, as offsets into
 *      the concatenated outputs (2 sCounter - 1 nodes, or 0 when fewer than two cases were sampled; the log's MUTATION
 *      events; its MIGRATION events + the nodes), counted on the device.
 *   2. walk: the caller allocates the outputs by those offsets and calls again.  Outputs of replicate i start at its
 *      offsets; status[i] = 0 or the reason its walk stopped (vgx_genealogy_message gives the text vgx_get_genealogy
 *      reports for it); a failed replicate does not fail the call.
 * Replicates whose workspace exceeds half of the free device memory (or VGX_GENEALOGY_CHUNK_BYTES) are walked in several
 * passes. */
typedef struct vgx_genealogies_io {
    int64_t n;                               /* selected replicates */
    const int64_t *replicates;               /* [n] */
    const uint64_t *rng_state;               /* [n][4] PCG64 start: state hi, lo, increment hi, lo (walk call) */
    int64_t *node_off, *mut_off, *mig_off;   /* [n+1] written by the sizing call, read by the walk call */
    int64_t *tree, *tree_pop; double *times;                         /* [node_off[n]] */
    int64_t *mut_node, *mut_AS, *mut_DS, *mut_site; double *mut_time; /* [mut_off[n]] */
    int64_t *mig_node, *mig_old, *mig_new; double *mig_time;         /* [mig_off[n]] */
    int64_t *status, *status_arg, *nodes_used, *mut_n, *mig_n;       /* [n] */
    uint64_t *rng_out;                       /* [n][4] generator state after the walk */
    int64_t layout;                          /* 0 = one replicate per lane (default), 1 = one replicate per wavefront */
    int64_t passes;                          /* out: device passes the walk took */
    double ms[3];                            /* out: walk kernels (device time), host clock and output conversion, whole call */
} vgx_genealogies_io;
int vgx_get_genealogies(vgx_engine *e, vgx_genealogies_io *io);
/* Text of a walk status (vgx_genealogies_io.status, .status_arg) as vgx_get_genealogy reports the same condition; returns
 * the status. */
int vgx_genealogy_message(int64_t status, int64_t arg, char *errbuf, int64_t errcap);
/* Test hook: the walk of vgx_get_genealogies (same code, compiled for the host) on the chain, state and generator of a
 * vgx_genealogy_io; same outputs as vgx_get_genealogy.  Direct chains only: a MULTITYPE event with rows is refused. */
int vgx_test_genealogy_walk(vgx_genealogy_io *io, char *errbuf, int64_t errcap);

/* The backward pass for many replicates of the last vgx_simulate_tau call (with the event log), on the device.  For every selected
 * replicate the result is what vgx_get_genealogy returns on that replicate's WHOLE chain in the reference's layout, from its final
 * state: the events and multievent rows the model held when the call started (`prefix`, shared by all replicates; NULL or empty
 * when there were none), then the replicate's own steps with their rows in the reference's order and granularity (one row per
 * channel: the tau kernels append a row per drawn transmission, mutant or migrant, in scheduling order).  A replicate that
 * restarted (vgx_counters.restarts > 0) has no prefix.  A canonicalise kernel (one workgroup per replicate) sorts every step's
 * rows by the reference's channel order in LDS and merges equal channels into compact rows in the pass's workspace — the
 * multievent log itself is only read — and a walk kernel (one replicate per wavefront) takes the rows from the last step back,
 * then the prefix, then the closing pass.  Prefix events of direct type take the single-event rule of vgx_get_genealogies.
 * The two-call protocol, the outputs and the passes are those of vgx_get_genealogies (VGX_GENEALOGY_CHUNK_BYTES included), with
 * these differences:
 *   - rng_state / rng_out are [n][6]: the PCG64 words, then numpy's buffered 32-bit half (rng_has_uint32, rng_uinteger of
 *     vgx_genealogy_io): the hypergeometric sampler draws 32-bit halves;
 *   - capacities of the sizing call: 2 sCounter - 1 nodes; mutation records: the sum of min(num, sCounter) over the replicate's
 *     MUTATION rows as the device holds them, plus the prefix's (an event counts 1); migration records likewise, plus the nodes;
 *   - THE STEP BOUND: the sort of a step holds a 16-byte key and a 2-byte row index per raw row in the 160 KiB of LDS a workgroup
 *     may declare: at most 8192 raw rows per step.  A replicate with a longer step gets status 10 (VGX_GW_STEP_ROWS, status_arg =
 *     the step of the call, 0-based) and fails nothing else;
 *   - status 12: a row with an index outside the model, or with more events than the counts of its compartment allow (numpy's
 *     hypergeometric raises on those; vgx_get_genealogy does not check them and must not be given such a chain: tau steps at very
 *     small counts can write one);
 *   - THE LOGARITHM: numpy's hypergeometric sampler (HRUA, from 10 draws on) calls log() in Stirling's ln k! (k >= 126) and in its
 *     acceptance test 2 log U <= T.  The device's library log and the host's are different functions, so the walk uses the
 *     engine's own logarithm (fdlibm's algorithm in +, -, *, / on binary64, no contraction; below 1 ulp): the device and its host
 *     instance (vgx_test_tau_genealogy_walk, vgx_test_hypergeometric) are identical by construction.  vgx_get_genealogy keeps
 *     libm's log: against it a draw — and the tree after it — can differ only where one of HRUA's comparisons is decided within
 *     the last ulp of a logarithm;
 *   - ms[0] is the device time of both kernels, ms[1] the host's conversion of the outputs.
 * Refusals (VGX_ERR_ARG): the last call was not vgx_simulate_tau; it recorded no rows (record_events = 0); a replicate that did
 * not restart continues a log of another length than prefix->ev_ptr; a prefix row with an index outside the model. */
typedef struct vgx_tau_genealogy_prefix {
    int64_t ev_ptr;                          /* events of the model's chain before the call */
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;                        /* multievent rows its MULTITYPE events index as [haplotypes, populations) */
    const int64_t *mev_num; const double *mev_times;   /* mev_times may be NULL: the event's time then */
    const int64_t *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
} vgx_tau_genealogy_prefix;
typedef struct vgx_tau_genealogies_io {
    int64_t n;                               /* selected replicates */
    const int64_t *replicates;               /* [n] */
    const uint64_t *rng_state;               /* [n][6] start of every walk (walk call) */
    int64_t *node_off, *mut_off, *mig_off;   /* [n+1] written by the sizing call, read by the walk call */
    int64_t *tree, *tree_pop; double *times;                         /* [node_off[n]] */
    int64_t *mut_node, *mut_AS, *mut_DS, *mut_site; double *mut_time; /* [mut_off[n]] */
    int64_t *mig_node, *mig_old, *mig_new; double *mig_time;         /* [mig_off[n]] */
    int64_t *status, *status_arg, *nodes_used, *mut_n, *mig_n;       /* [n] */
    uint64_t *rng_out;                       /* [n][6] generator state after the walk */
    int64_t passes;                          /* out: device passes the walk took */
    double ms[3];                            /* out: kernels (device time), output conversion, whole call */
} vgx_tau_genealogies_io;
int vgx_get_tau_genealogies(vgx_engine *e, vgx_tau_genealogies_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: the walk of vgx_get_tau_genealogies (same key, merge rule, row rule and sampler, compiled for the host) on the
 * chain, state and generator of a vgx_genealogy_io; same outputs as vgx_get_genealogy.  The chain's trailing MULTITYPE events
 * play the replicate's own steps: their rows may come in any order and granularity (they are brought into the reference's by
 * the device's key; a step of more than 8192 rows is refused with the text of status 10).  Everything before them plays the
 * prefix: its rows are taken as they are.  `sites`: the model's number of sites (hapNum = 4^sites). */
int vgx_test_tau_genealogy_walk(vgx_genealogy_io *io, int64_t sites, char *errbuf, int64_t errcap);
/* Test hook: n draws of numpy's random_hypergeometric(good, bad, sample) as the walk makes them, by the host build of the sampler
 * or the device's; state = PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger (in / out). */
int vgx_test_hypergeometric(int on_device, int64_t good, int64_t bad, int64_t sample, int64_t n, uint64_t state[6], int64_t *out);

/* ---- log replays ---------------------------------------------------------------------------- */
/* Replaces BirthDeathModel.get_data_infectious(pop, hap, step_num) / get_data_susceptible(pop, group, step_num) (pyx:1967-2045)
 * for many replicates of the last vgx_simulate_direct call and many compartments at once, on the device: one pass per
 * replicate over the device event log in place (the log is not copied to the host).  Event times do not exist on the
 * device; the host clock (the times vgx_get_events gives) decides only at which event the grid index advances, from the
 * packed (iteration, rate) logs: 12 bytes per event reach the host, in pinned memory.  Direct chains only: refused after
 * vgx_simulate_tau (MULTITYPE rows are not replayed here) or a call without an event log; every selected replicate's chain
 * must start at log index 0 (vgx_counters.ev_first_new == 0).  T = step_num + 1.
 *   semantics 0 (reference): the reference's replay to the letter, including the operator precedence of pyx:1982 (a DEATH or
 *     SAMPLING in ANY compartment decrements every infectious series and every SAMPLING counts in every Sample); entries after
 *     last_point stay 0 as upstream leaves them.
 *   semantics 1 (compartment): the series of the compartment itself.  Infectious (p, h): BIRTH at (p, h) +1; DEATH / SAMPLING
 *     at (p, h) -1; MUTATION from (p, h) -1, to (p, newHaplotype) +1; MIGRATION with newPopulation == p, haplotype == h +1;
 *     Sample: SAMPLING at (p, h).  Susceptible: as the reference.  Entries after last_point repeat the value at last_point.
 * Every series starts from initial_infectious[pop][hap] / initial_susceptible[pop][group] as the engine holds it (the state an
 * attempt restarts from).  A query may be given once only.  Two calls:
 *   1. sizing: time_points == NULL.  Sets loc_cap to the most lockdown records any selected replicate holds (at least 1).
 *   2. replay: the caller allocates the outputs and calls again with that loc_cap (or a larger one).
 * The per-bin counters of a launch live in a workgroup's LDS: 4 (step_num + 2 T + (2 n_inf + n_sus) T) bytes and a small
 * table.  The budget is 64 KiB per workgroup (VGX_TIMELINES_LDS_BYTES changes it, up to the 160 KiB a workgroup may declare);
 * a call whose queries need more is split over several launches, each re-reading the log.  step_num must leave room for one
 * query (step_num <= 8000 is safe).  Replicates whose staging and outputs exceed half of the free device memory or 1 GiB (or
 * VGX_TIMELINES_CHUNK_BYTES) are replayed in several chunks.  vgx_clock_mismatches counts every selected replicate once, as
 * vgx_get_genealogies does.
 * The pinned (page-locked) host staging of the packed logs, 12 bytes per event of the largest chunk (up to about 1 GiB at the
 * default chunk size), is kept by the engine for the next call and freed by vgx_destroy.
 * A model that had been simulated before (first_simulation != 0) and whose event log was empty when the call started passes the
 * ev_first_new == 0 condition, but its chain starts from the model's state at that time, not from initial_*: 'reference' still
 * equals the reference's replay (which starts from initial_* too), 'compartment' then does not end in the final state.
 * Refusals (VGX_ERR_ARG) carry the wording of Ensemble.timelines' ValueErrors behind "vgx_get_timelines: ". */
typedef struct vgx_timelines_io {
    int64_t n;                               /* selected replicates */
    const int64_t *replicates;               /* [n] */
    int64_t step_num, semantics;
    int64_t n_inf; const int64_t *inf_pop, *inf_hap;    /* infectious queries (population, haplotype) */
    int64_t n_sus; const int64_t *sus_pop, *sus_grp;    /* susceptible queries (population, group) */
    double *time_points;                     /* [n][T] i * currentTime / step_num of every replicate's own final time */
    double *inf_data, *inf_sample;           /* [n][n_inf][T] */
    double *sus_data;                        /* [n][n_sus][T] */
    int64_t *last_point;                     /* [n] last grid index the replay reached */
    int64_t loc_cap;                         /* in (replay) / out (sizing): lockdown records per replicate there is room for */
    int64_t *loc_n, *loc_state, *loc_pop;    /* [n], [n][loc_cap], [n][loc_cap] lockdown records (models.pxi:52-66) */
    double *loc_time;                        /* [n][loc_cap] their host-clock times */
    int64_t passes;                          /* out: launches of the replay kernel */
    double ms[3];                            /* out: pack and replay kernels (device time), host clock, whole call */
} vgx_timelines_io;
int vgx_get_timelines(vgx_engine *e, vgx_timelines_io *io);
/* Test hook: the replay of vgx_get_timelines (same classification, cut rule and query table, compiled for the host) on one
 * chain given as arrays: no device, no engine.  Direct chains only: a MULTITYPE event with rows is refused. */
typedef struct vgx_timelines_chain {
    int64_t popNum, hapNum, susNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    double currentTime;
    int64_t step_num, semantics;
    int64_t n_inf; const int64_t *inf_pop, *inf_hap, *inf_start;   /* inf_start[k] = initial_infectious[pop][hap] */
    int64_t n_sus; const int64_t *sus_pop, *sus_grp, *sus_start;
    double *time_points;                     /* [T] */
    double *inf_data, *inf_sample;           /* [n_inf][T] */
    double *sus_data;                        /* [n_sus][T] */
    int64_t last_point;
} vgx_timelines_chain;
int vgx_test_timelines(vgx_timelines_chain *io, char *errbuf, int64_t errcap);

/* The same replays for many replicates of the last vgx_simulate_tau call (with the event log), on the device: one pass per
 * replicate over its multievent rows where the tau kernels left them (48 bytes each; nothing is copied to the host or compacted).
 * A tau call normally continues a chain, and the reference replays the WHOLE chain: the events the model held when the call
 * started (`prefix`, shared by all replicates; NULL or empty when there were none), then the replicate's own steps, on the grid
 * i * currentTime_r / step_num of the replicate's own final time.  The prefix is flattened once per call into rows of the same
 * layout (a direct event = a row with num 1, a MULTITYPE event of an earlier tau call = its multievent rows), uploaded once,
 * and replayed in front of every replicate's own rows.  A replicate that restarted (vgx_counters.restarts > 0) starts from
 * time 0 without the prefix.  Multievent rows take the rule of the reference's MULTITYPE branch, which differs from the direct
 * one in its susceptible MIGRATION clause (pyx:2037 tests `haplotypes`, pyx:2023 `newHaplotypes`); the order of a step's rows
 * does not matter (they share a bin and every update is an integer sum).  No host clock runs: step times are host doubles.
 * Same structure, two-call protocol, semantics, outputs and environment switches as vgx_get_timelines, with these differences:
 *   - counters are 64-bit in LDS (a bin sums `num` over many steps): 8 (2 T + (2 n_inf + n_sus) T) + 4 step_num bytes and the table;
 *   - every series is exact while its values stay below 2^53 in magnitude (the reference accumulates in float64 and is exact in
 *     the same range);
 *   - lockdown records of a replicate: the prefix's, then the call's (a restarted replicate: the call's only);
 *   - ms[1] is the host's cut search (no clock), ms[0] the replay kernel.
 * Refusals (VGX_ERR_ARG): the last call was not vgx_simulate_tau; it recorded no rows (record_events = 0); a replicate that
 * did not restart continues a log of another length than prefix->ev_ptr; prefix plus own rows reach 2^31. */
typedef struct vgx_timelines_prefix {
    int64_t ev_ptr;                          /* events of the model's chain before the call */
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;                        /* multievent rows its MULTITYPE events index as [haplotypes, populations) */
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t loc_n;                           /* lockdown records before the call */
    const int64_t *loc_state, *loc_pop; const double *loc_time;
} vgx_timelines_prefix;
int vgx_get_tau_timelines(vgx_engine *e, vgx_timelines_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: the replay of vgx_get_tau_timelines (same classification, flattening, cut search and query table, compiled for the
 * host) on one chain given as arrays, multievent rows included (dense logs with num == 0 rows are accepted): no device, no
 * engine.  The chain's trailing MULTITYPE events play the replicate's own steps, everything before them the prefix. */
typedef struct vgx_tau_timelines_chain {
    vgx_timelines_chain chain;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
} vgx_tau_timelines_chain;
int vgx_test_tau_timelines(vgx_tau_timelines_chain *io, char *errbuf, int64_t errcap);

/* ---- summaries across replicates ------------------------------------------------------------ */
/* What a user reads off an ensemble's trajectories: for every group of replicates (a scenario, or all of them) and every column
 * n = (point, population, compartment) of the [R][N] block vgx_get_trajectories gives (N = traj_points * popNum * 2), from the m
 * values the group's members hold there: count, min, max, the exact sum, the exact sum of squares (below 2^76: two 64-bit words,
 * low then high) and the order statistics at K ranks per group: element ranks[g][k] in [0, m_g) of the values sorted ascending,
 * ties included.  The block stays on the device and is only read: a transpose kernel narrows a chunk of columns to 32-bit keys
 * with every group's members contiguous, then every (column, group) segment is sorted by a wavefront (groups of up to 64) or by
 * a workgroup in LDS (larger ones).  All of it is integer arithmetic: no result depends on launch geometry or summation order.
 * group_of[r] in [-1, G): the group of replicate r, -1 leaves it out.  An empty group is no error: count 0, every output 0 (its
 * ranks are not read).  Refusals (VGX_ERR_ARG): the last call recorded no trajectories; a population size of 2^31 or more; a
 * label or rank out of range; a group of more than VGX_COLSUMMARY_MAX_GROUP members (the message names the group, its size and
 * the limit: such a group is not split across passes).  When the call returns an error the output arrays, passes and ms are
 * undefined (count may already be written).  Device memory, freed before the call returns: the outputs below in
 * their device form (G N (32 + 4 K) bytes) and the transposed scratch, 4 bytes per (member, column of a chunk), at most
 * VGX_COLSUMMARY_CHUNK_BYTES (default 2^28) or 64 columns, whichever is more. */
#define VGX_COLSUMMARY_MAX_GROUP 16384       /* u32 keys a workgroup sorts in LDS: 64 KiB of the 160 KiB it may declare */
typedef struct vgx_traj_summary_io {
    int64_t G;                               /* groups */
    const int64_t *group_of;                 /* [R] */
    int64_t K;                               /* ranks per group (0: none) */
    const int64_t *ranks;                    /* [G][K] */
    int64_t *count;                          /* [G] out: members */
    int64_t *sum;                            /* [G][N] out */
    uint64_t *sumsq;                         /* [G][N][2] out: low, high word */
    int64_t *min, *max;                      /* [G][N] out */
    int64_t *stat;                           /* [G][K][N] out (may be NULL when K == 0) */
    int64_t passes;                          /* out: chunks of columns */
    double ms[3];                            /* out: kernels (device time), uploads, read-out and widening of the results, whole call */
} vgx_traj_summary_io;
int vgx_get_trajectory_summary(vgx_engine *e, vgx_traj_summary_io *io);
/* Test hook: the same kernels on a host matrix x[R][N] (uploaded; no engine).  Every entry must be a whole number in [0, 2^31):
 * checked on the host, VGX_ERR_ARG otherwise.  The message of a refusal is written to errbuf. */
int vgx_test_column_summary(const double *x, int64_t R, int64_t N, vgx_traj_summary_io *io, char *errbuf, int64_t errcap);

/* ---- incidence: event counts per time bin --------------------------------------------------- */
/* What is compared with surveillance data: how many events of every kind happened per time bin and population, on ONE grid
 * for all replicates.  The caller gives the bin edges edges[0 .. T] (strictly increasing, finite, T >= 1); bin b holds the
 * events with edges[b] <= t < edges[b + 1] as the literal loop over the chain sees them: with the event times vgx_get_events
 * gives, cut[k] = first event index i with edges[k] <= t_i (n_ev if none; the loop's position never goes back, whatever the
 * times do), event i is in bin b when cut[b] <= i < cut[b + 1], and outside[r] = (cut[0], n_ev - cut[T]) counts the events
 * before and after the window.  A log record (type, haplotype, population, newHaplotype, newPopulation) counts in channel
 *   0 BIRTH, 1 DEATH, 2 SAMPLING, 3 MUTATION, 4 SUSCCHANGE            keyed by population
 *   5 MIGRATION as an arrival (the new infection)                      keyed by newPopulation
 *   6 MIGRATION as a departure (its source)                            keyed by population
 * so a MIGRATION counts twice and new infections in p are channels 0 + 5.  A key outside [0, popNum) or a type outside 0..5
 * counts nowhere.  hap_mask (bit h of word h / 32 = haplotype h, ceil(hapNum / 32) words) restricts the count to records whose
 * judged haplotype is in the mask: `haplotype` for BIRTH, DEATH, SAMPLING and MIGRATION, `newHaplotype` (the variant that arises)
 * for MUTATION; SUSCCHANGE carries none and is not counted under a mask.
 * The device reads every selected replicate's log in place: a workgroup takes one replicate and a tile of consecutive events
 * (VGX_INCIDENCE_TILE_EVENTS, default 4096), finds its first bin by a search in the replicate's cuts, counts into a histogram
 * of popNum * 7 int32 in LDS and adds the nonzero cells to the block counts[n][T][popNum][7] in device memory at every bin
 * change and at the tile's end.  All of it is integer work: no result depends on the tile size or the launch geometry.  The
 * host clock runs as in vgx_get_timelines (12 bytes per event staged in pinned memory, in chunks of replicates:
 * VGX_TIMELINES_CHUNK_BYTES); the log itself is never copied.  `summary`, when given, is the column summary of
 * vgx_get_trajectory_summary over the block as a matrix [n][T * popNum * 7] where it lies (group_of has n entries, one per
 * SELECTED replicate in the order of `replicates`); `counts` may then be NULL and the block is not copied to the host.
 * Preconditions as vgx_get_timelines: the last call was direct and recorded events; every selected chain starts at log index 0.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_incidence: "): those; replicates out of range or given twice; edges
 * that are not finite or do not increase; popNum * 28 bytes of counters above the 65536 bytes of LDS a counting workgroup may
 * use; a block above half of the free device memory (the message gives the bytes: select fewer replicates); a chain of 2^30
 * events or more.  vgx_clock_mismatches counts every selected replicate once. */
#define VGX_INC_CHANNELS 7
typedef struct vgx_incidence_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *edges;              /* [T + 1] strictly increasing */
    const uint32_t *hap_mask;                    /* NULL or ceil(hapNum / 32) words */
    int32_t *counts;                             /* NULL or host [n][T][P][7] */
    int64_t *outside;                            /* [n][2] events before / after the window */
    vgx_traj_summary_io *summary;                /* NULL or the summary of the [n][T*P*7] block; group_of has n entries */
    int64_t passes; double ms[3];                /* out: launches of the counting kernel; kernels, host clock, whole call */
} vgx_incidence_io;
int vgx_get_incidence(vgx_engine *e, vgx_incidence_io *io);
/* Test hook: the rule and the tile walk of vgx_get_incidence compiled for the host, on one chain given as arrays (no device, no
 * engine), tile after tile with `tile` events each (0: the default).  counts [T][P][7] and outside [2] are overwritten.  The
 * same limits: P * 28 bytes above the LDS budget, a chain of 2^30 events and bad edges are refused with the message in errbuf. */
int vgx_test_incidence(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                       const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                       const double *edges, int64_t T, const uint32_t *hap_mask, int64_t tile, int32_t *counts, int64_t *outside,
                       char *errbuf, int64_t errcap);

/* ---- flows: who infects whom per time bin and variant class ------------------------------------ */
/* What a multi-population model is built for: who seeds whom.  Every new infection in the log names its source, so the whole
 * transmission matrix per time bin and variant class is one pass over the records vgx_get_incidence streams.
 * The caller gives the bin edges of vgx_get_incidence (edges[0 .. T], the same cuts, bins and outside[r] = (cut[0], n_ev - cut[T]))
 * and the map of vgx_get_prevalence (variant_of[hapNum] with values in [-1, V), -1 = not tracked).  A log record
 * (type, haplotype, population, newHaplotype, newPopulation) counts +1, with c = variant_of[haplotype], in the cell
 *   BIRTH       (src, dst, c) = (population, population, c)        a transmission within; skipped when `within` is 0
 *   MIGRATION   (src, dst, c) = (population, newPopulation, c)     a transmission across, literally: equal keys land on the diagonal
 * of its bin and every other type nowhere.  A type outside 0..5, c < 0, a haplotype outside [0, hapNum) or either key outside
 * [0, popNum) counts nowhere.  The block is counts[n][T][popNum][popNum][V] in src, dst, class order.  With hap_mask = the members
 * of class c, its margins are vgx_get_incidence's channels: the sum over src is 0 + 5, the off-diagonal sum over dst is 6, and
 * the diagonal is 0 unless a MIGRATION has equal keys.
 * The device reads every selected replicate's log in place with the geometry of vgx_get_incidence: a workgroup takes one
 * replicate and a tile of consecutive events (VGX_FLOWS_TILE_EVENTS, default 4096), finds its first bin by a search in the
 * replicate's cuts, and adds the nonzero cells it keeps in LDS to the block in device memory at every bin change and at the
 * tile's end.  Two forms of that walk: dense keeps all popNum^2 * V int32 cells in LDS (possible up to 65536 bytes), split keeps
 * the popNum * V cells of the diagonal and adds a record off the diagonal to its cell in device memory at once.  Dense runs where
 * it fits, else split; VGX_FLOWS_FORM=dense|split forces one; `form` reports the one that ran (1 dense, 2 split).  All of it is
 * integer work: no result depends on the form, the tile size, the launch geometry or the chunking.  The host clock runs as in
 * vgx_get_incidence (VGX_TIMELINES_CHUNK_BYTES); the log itself is never copied.  `summary`, when given, is the column summary
 * of vgx_get_trajectory_summary over the block as a matrix [n][T * popNum * popNum * V] where it lies (group_of has n entries,
 * one per SELECTED replicate in the order of `replicates`); `counts` may then be NULL and the block is not copied to the host.
 * Preconditions as vgx_get_incidence: the last call was direct and recorded events; every selected chain starts at log index 0.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_flows: "): those; replicates out of range or given twice; edges that are
 * not finite or do not increase; T outside [1, 2^24); V < 1 or a variant_of value outside [-1, V); popNum * V * 4 bytes of
 * diagonal cells above the 65536 bytes of LDS a counting workgroup may use, or the dense form forced where popNum^2 * V * 4
 * bytes are (the message gives the bytes); a value of VGX_FLOWS_FORM that is neither; a block of n x T x P x P x V counts above
 * half of the free device memory (the message gives the bytes: select fewer replicates); a chain of 2^30 events or more.
 * vgx_clock_mismatches counts every selected replicate once. */
typedef struct vgx_flows_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *edges;              /* [T + 1] strictly increasing */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t within;                              /* 1: births count on the diagonal; 0: migrations alone */
    int32_t *counts;                             /* NULL or host [n][T][P][P][V] */
    int64_t *outside;                            /* [n][2] events before / after the window */
    vgx_traj_summary_io *summary;                /* NULL or the summary of the [n][T*P*P*V] block; group_of has n entries */
    int64_t form, passes; double ms[3];          /* out: the form that ran (1 dense, 2 split); launches of the counting kernel; kernels, host clock, whole call */
} vgx_flows_io;
int vgx_get_flows(vgx_engine *e, vgx_flows_io *io);
/* Test hook: the rule and the tile walk of vgx_get_flows compiled for the host, on one chain given as arrays (no device, no
 * engine), tile after tile with `tile` events each (0: the default), in the form `form` asks for (0: the automatic choice,
 * 1 dense, 2 split; the hist of a tile holds that form's cells).  counts [T][P][P][V] and outside [2] are overwritten, *form_ran
 * (may be NULL) gets the form that ran.  The same limits: a form that does not fit the LDS budget, a chain of 2^30 events, bad
 * edges, V or variant_of are refused with the message in errbuf. */
int vgx_test_flows(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                   const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                   const double *edges, int64_t T, const int32_t *variant_of, int64_t V, int32_t within, int64_t tile, int64_t form,
                   int32_t *counts, int64_t *outside, int64_t *form_ran, char *errbuf, int64_t errcap);

/* ---- prevalence: infectious hosts per variant class on a common grid --------------------------- */
/* How many hosts carry which variant, when: the stock where vgx_get_incidence gives the flows, on ONE grid for all replicates
 * (DESIGN.md §18).  The caller gives the grid times grid[0 .. T-1] (strictly increasing, finite, 1 <= T < 2^24) and a map
 * variant_of[hapNum] with values in [-1, V): the class of every haplotype, -1 = not tracked.  With the event times vgx_get_events
 * gives, cut[j] = first event index i with grid[j] < t_i (n_ev if none; the loop's position never goes back, whatever the times
 * do).  The comparison is strict, as the trajectories' is: a grid point gets the state before the event that takes the time past
 * it, and an event at exactly grid[j] is applied before point j.  Interval j = 0 .. T holds the events cut[j-1] <= i < cut[j]
 * (cut[-1] = 0, cut[T] = n_ev; interval T is the tail after the last grid point), and outside[r] = (cut[0], n_ev - cut[T-1]).
 * A log record (type, haplotype, population, newHaplotype, newPopulation) changes, with c = variant_of[haplotype],
 *   BIRTH              +1 at (population, c)
 *   DEATH, SAMPLING    -1 at (population, c)
 *   MUTATION           -1 at (population, c), +1 at (population, variant_of[newHaplotype]); equal classes change nothing
 *   MIGRATION          +1 at (newPopulation, c)
 *   SUSCCHANGE         nothing
 * each side only if its class is tracked (the 'compartment' semantics of vgx_get_timelines folded through variant_of).  A type
 * outside 0..5, a population key outside [0, popNum) or a haplotype outside [0, hapNum) counts nowhere.
 *   values[r][j] = start_r + the sum of the changes of the intervals 0 .. j,   final[r] = the same over all T + 1 intervals
 * where start_r is the state the call started from (the host state after its first-call preparation, the index case included)
 * folded through variant_of, or the initial state for a replicate that restarted (vgx_counters.restarts > 0).  With every
 * haplotype tracked final[r] is the replicate's final infectious state (vgx_get_state) folded through variant_of.
 * The device reads every selected replicate's log in place: a workgroup takes one replicate and a tile of consecutive events
 * (VGX_PREVALENCE_TILE_EVENTS, default 4096), finds its first interval by a search in the replicate's cuts, accumulates the
 * signed changes in popNum * V int32 cells in LDS and adds the nonzero cells to a block of net changes in device memory at every
 * interval change and at the tile's end; a scan kernel then turns every (replicate, population, class) column into running sums where
 * it lies.  All of it is integer work: no result depends on the tile size, the launch geometry or the chunking.  The host clock
 * runs as in vgx_get_incidence (VGX_TIMELINES_CHUNK_BYTES); the log itself is never copied.  `summary`, when given, is the
 * column summary of vgx_get_trajectory_summary over `values` as a matrix [n][T * popNum * V] where it lies (`final` is not part
 * of it; group_of has n entries, one per SELECTED replicate in the order of `replicates`); it needs whole numbers in
 * [0, 2^31), which a device min/max pass checks: if it fails the summary is refused with the offending value in the message,
 * after values and final, if asked for, have been written (a negative value can come only from a log with records outside
 * the model).  `values` may be NULL: the block is then not copied to the host.
 * Preconditions as vgx_get_incidence: the last call was direct and recorded events; every selected chain starts at log index 0.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_prevalence: "): those; replicates out of range or given twice; a grid
 * that is not finite or does not increase; T outside [1, 2^24); V < 1 or a variant_of value outside [-1, V); a population size
 * of 2^31 or more; popNum * V * 4 bytes of cells above the 65536 bytes of LDS a counting workgroup may use; a block
 * (4 n (T + 1) popNum V bytes) above half of the free device memory (the message gives the bytes: select fewer replicates); a
 * chain of 2^30 events or more.  vgx_clock_mismatches counts every selected replicate once. */
typedef struct vgx_prevalence_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t *values;                             /* NULL or host [n][T][P][V] */
    int32_t *final;                              /* NULL or host [n][P][V] */
    int64_t *outside;                            /* [n][2]: events before cut[0] / from cut[T-1] on */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*V]; group_of has n entries */
    int64_t passes; double ms[3];                /* out: launches of the counting kernel; kernels, host clock, whole call */
} vgx_prevalence_io;
int vgx_get_prevalence(vgx_engine *e, vgx_prevalence_io *io);
/* Test hook: the rule, the tile walk and the scan of vgx_get_prevalence compiled for the host, on one chain given as arrays (no
 * device, no engine), tile after tile with `tile` events each (0: the default).  start [P][V]: whole numbers in [0, 2^31).
 * values [T][P][V], final [P][V] and outside [2] are overwritten.  The same limits: the LDS budget, a chain of 2^30 events, a bad
 * grid, V or variant_of are refused with the message in errbuf. */
int vgx_test_prevalence(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                        const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                        const double *grid, int64_t T, const int32_t *variant_of, int64_t V, const int64_t *start, int64_t tile,
                        int32_t *values, int32_t *final, int64_t *outside, char *errbuf, int64_t errcap);

/* ---- lineages: ancestral lineages of the sample per population and variant class on a common grid --- */
/* The tree's counterpart of vgx_get_prevalence: how many ancestral lineages of the sampled cases are alive at each
 * grid time, in which population, carrying which variant, for many replicates of the last vgx_simulate_direct call at once.  It
 * cannot be rebuilt from what vgx_get_genealogies returns (a migration that moves a lineage without coalescing writes no record at
 * its own event, and the haplotype a lineage carries between nodes appears nowhere), so it comes out of the walk itself.
 * The walk is that of vgx_get_genealogies: the same draws in the same order from rng_state, the same status and the same
 * generator state afterwards (rng_out).  Whenever it changes a lineage list it appends one lineage record of six int32 words,
 * kind, hap, pop, newHap, newPop, ev (the event index), to a per-replicate log on the device.  Read forward in time, with
 * c(h) = variant_of[h] and a side of class -1 skipped, a record changes
 *   TIP       a SAMPLING pushes a lineage                                -1 at (pop, c(hap))
 *   SPLIT     a BIRTH coalesces                                          +1 at (pop, c(hap))
 *   SPLIT     a MIGRATION coalesces, pop = the event's newPopulation     +1 at (pop, c(hap))
 *   MUTATION  a MUTATION takes a lineage                                 -1 at (pop, c(hap)), +1 at (pop, c(newHap)); equal classes change nothing
 *   MOVE      a MIGRATION moves a lineage without coalescing             -1 at (pop, c(hap)), +1 at (newPop, c(hap))
 * (the migration records vgx_get_genealogies' closing pass adds are no lineage records).  A replicate's log holds at most
 * (2 sCounter - 1) + its MUTATION events + its MIGRATION events records, counted on the device; a full log sets status 9 and is
 * never written past its end.
 * The grid is vgx_get_prevalence's: grid[0 .. T-1] strictly increasing and finite, cut[j] = first event index i with
 * grid[j] < t_i (strict; the position never goes back), from the host clock; a record with event index ev lies in interval k =
 * 0 .. T when cut[k-1] <= ev < cut[k] (cut[-1] = 0, cut[T] = n_ev).  No lineage is alive after the last event, so
 *   values[r][j][p][c] = -(net change of the intervals j+1 .. T),   root[r][p][c] = -(net change of all intervals)
 * or values[j] = root + net of the intervals 0 .. j: prevalence's formula with `root` as the start.  With every haplotype tracked
 * root sums to 1 for a walk that succeeded.  A replicate whose walk fails gets its status (vgx_genealogy_message gives the text)
 * and zeros; it does not fail the call.
 * On the device a pass is three kernels on the engine's stream: the walk (one replicate per wavefront), a binning kernel in
 * vgx_get_prevalence's geometry over the lineage logs (a workgroup takes one replicate and a tile of VGX_LINEAGES_TILE_RECORDS
 * consecutive records, default 4096, and keeps popNum * V int32 cells in LDS) and a suffix-sum kernel that turns the net block
 * into values and root in place.  All work after the cuts is integer work: no result depends on the tile size, the launch
 * geometry or the number of passes.  Replicates whose workspace exceeds half of the free device memory (or
 * VGX_GENEALOGY_CHUNK_BYTES) are walked in several passes.  `summary`, when given, is the column summary of
 * vgx_get_trajectory_summary over `values` as a matrix [n][T * popNum * V] where it lies (group_of has n entries, one per
 * SELECTED replicate); if a replicate with group_of >= 0 has a nonzero status the summary is refused with their number in the
 * message, after values, root, status, status_arg, records and rng_out have been written.  `values` may be NULL: the block is
 * then not copied to the host.
 * Preconditions as vgx_get_genealogies: the last call was direct and recorded events; every selected chain starts at log index 0.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_lineages: "): those; replicates out of range or given twice; a grid that is
 * not finite or does not increase; T outside [1, 2^24); V < 1 or a variant_of value outside [-1, V); popNum * V * 4 bytes of cells
 * above the 65536 bytes of LDS a binning workgroup may use; a block (4 n (T + 1) popNum V bytes) above half of the free device
 * memory; a chain of 2^30 events or more.  vgx_clock_mismatches counts every selected replicate once. */
typedef struct vgx_lineages_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][4] PCG64 start of every walk: state hi, lo, increment hi, lo */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t *values;                             /* NULL or host [n][T][P][V] */
    int32_t *root;                               /* host [n][P][V] */
    int64_t *status, *status_arg;                /* [n] 0 or why the walk stopped, as vgx_genealogies_io */
    int64_t *records;                            /* [n] lineage records of the walk (0 for a walk that failed) */
    uint64_t *rng_out;                           /* [n][4] generator state after the walk */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*V]; group_of has n entries */
    int64_t passes;                              /* out: walk passes */
    double ms[3];                                /* out: kernels (device time), host clock, whole call */
    double kernel_ms[3];                         /* out: the walk, binning and suffix-sum kernels of ms[0] apart */
} vgx_lineages_io;
int vgx_get_lineages(vgx_engine *e, vgx_lineages_io *io);
/* Test hook: the walk of vgx_get_lineages with its observer, the tile walk and the suffix sum compiled for the host, on the chain,
 * state and generator of a vgx_genealogy_io (its tree, mutation and migration outputs are not read or written; infectious is walked
 * back in place and rng_state advanced as vgx_test_genealogy_walk does), tile after tile of `tile` records (0: the default).
 * values [T][P][V] and root [P][V] are overwritten, *records gets the number of lineage records.  A walk that fails is refused with
 * the message vgx_get_genealogy reports; a bad grid, V or variant_of and the LDS budget are refused as vgx_get_lineages does. */
int vgx_test_lineages(vgx_genealogy_io *io, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                      int32_t *values, int32_t *root, int64_t *records, char *errbuf, int64_t errcap);

/* The same lineages for many replicates of the last vgx_simulate_tau call (with the event log), on the device.
 * The walk is that of vgx_get_tau_genealogies over the same chain (`prefix` as that call takes it: the model's chain before the
 * tau call, shared by every replicate that did not restart, then the replicate's own steps as canonical rows): the same draws in
 * the same order from rng_state, the same status and status_arg and the same six generator words afterwards (rng_out).  Where the
 * row rule changes a lineage list it appends a lineage record with the meanings above: a BIRTH row a SPLIT per coalescence, a
 * SAMPLING row a TIP per tip, a MUTATION row a MUTATION per lineage taken, a MIGRATION row a SPLIT (pop = the row's newPopulation)
 * per coalescence and a MOVE per lineage moved without coalescing; prefix events of direct type as vgx_get_lineages.  `ev` is the
 * chain's EVENT index: prefix events 0 .. prefix->ev_ptr - 1, the replicate's own step k is prefix->ev_ptr + k (k alone for a
 * replicate that restarted), so all records of a step carry the same ev.  A log holds at most (2 sCounter - 1) records plus, per
 * MUTATION and MIGRATION row, min(num, sCounter), summed over the replicate's raw rows on the device, plus the same over the prefix's
 * rows (a direct event counts 1); a full log sets status 9.
 * The grid's cuts are formed in event-index space: cut[j] = first event index i with grid[j] < t_i (strict; the position never
 * goes back) over the prefix's event times, then the replicate's own step times, so a grid time exactly at a step's time has the
 * whole step applied, as vgx_get_tau_prevalence has it.  The prefix part of the loop runs once per call.  values, root, summary,
 * `values == NULL`, VGX_LINEAGES_TILE_RECORDS and VGX_GENEALOGY_CHUNK_BYTES as vgx_get_lineages; the binning and suffix-sum kernels
 * are that call's.  kernel_ms: the canonicalise, walk, binning and suffix-sum kernels of ms[0] apart; ms[1] is the host's cuts.
 * Preconditions and their refusals as vgx_get_tau_genealogies (the last call was vgx_simulate_tau, it recorded rows, the prefix
 * length, prefix rows inside the model); the grid, class and LDS refusals of vgx_get_lineages; replicates out of range or given
 * twice; a chain of 2^30 events or more.  All worded behind "vgx_get_tau_lineages: ". */
typedef struct vgx_tau_lineages_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][6] start of every walk: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t *values;                             /* NULL or host [n][T][P][V] */
    int32_t *root;                               /* host [n][P][V] */
    int64_t *status, *status_arg;                /* [n] 0 or why the walk stopped, as vgx_tau_genealogies_io */
    int64_t *records;                            /* [n] lineage records of the walk (0 for a walk that failed) */
    uint64_t *rng_out;                           /* [n][6] generator state after the walk */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*V]; group_of has n entries */
    int64_t passes;                              /* out: walk passes */
    double ms[3];                                /* out: kernels (device time), host cuts, whole call */
    double kernel_ms[4];                         /* out: the canonicalise, walk, binning and suffix-sum kernels of ms[0] apart */
} vgx_tau_lineages_io;
int vgx_get_tau_lineages(vgx_engine *e, vgx_tau_lineages_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: the walk of vgx_get_tau_lineages with its observer, the tile walk and the suffix sum compiled for the host, on the
 * chain, state and generator of a vgx_genealogy_io, with the chain handling of vgx_test_tau_genealogy_walk (the trailing MULTITYPE
 * events play the own steps, their rows in any order and granularity; `sites` as there).  The cuts come from the chain's event
 * times.  infectious is walked back in place and the generator (all six words) advanced as vgx_test_tau_genealogy_walk does; the
 * tree, mutation and migration outputs are not read or written.  values [T][P][V] and root [P][V] are overwritten, *records gets
 * the number of lineage records.  A walk that fails is refused with the message vgx_test_tau_genealogy_walk reports; a bad grid, V
 * or variant_of and the LDS budget are refused as vgx_get_tau_lineages does. */
int vgx_test_tau_lineages(vgx_genealogy_io *io, int64_t sites, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                          int32_t *values, int32_t *root, int64_t *records, char *errbuf, int64_t errcap);

/* ---- tree events: samples, coalescences, mutations and moves of the sampled trees per interval of a common grid --- */
/* The tree's counterpart of vgx_get_incidence and vgx_get_flows: the lineage log of vgx_get_lineages, written by the
 * same walk, binned with the kinds kept apart.  With c(h) = variant_of[h], read forward in time, a lineage record counts +1 at the
 * cells (pop, class, channel)
 *   0 samples           TIP                                                      (pop, c(hap))
 *   1 coalescences      SPLIT (pop of a coalescing MIGRATION: its newPopulation) (pop, c(hap))
 *   2 mutations_within  MUTATION with c(hap) == c(newHap) >= 0                   (pop, c(hap))
 *   3 mutations_out     MUTATION with c(hap) >= 0 and c(newHap) != c(hap)        (pop, c(hap))
 *   4 mutations_in      MUTATION with c(newHap) >= 0 and c(newHap) != c(hap)     (pop, c(newHap))
 *   5 departures        MOVE with c(hap) >= 0                                    (pop, c(hap))
 *   6 arrivals          MOVE with c(hap) >= 0 and newPop inside [0, popNum)      (newPop, c(hap))
 * and nowhere for a class of -1, a population or haplotype outside the model or another kind, so that for every interval and cell
 *   coalescences - samples + mutations_in - mutations_out + arrivals - departures == the net change vgx_get_lineages sums up:
 * lineages' root = -(net of all intervals), values[j] = root + net of the intervals 0 .. j.
 * The grid, its cuts and the intervals are vgx_get_lineages': interval i = 0 .. T holds the records with cut[i-1] <= ev < cut[i],
 * interval T being the tail after the last grid time, an ordinary row of
 *   counts[r][i][p][c][k]   int32 [n][T + 1][popNum][V][7]
 * (int32: no cell counts more than a log holds, and the calls bound a log below 2^31 records).  A replicate whose walk fails gets
 * its status and a row of zeros.  On the device a pass is the walk kernel of vgx_get_lineages and one binning kernel in its tile
 * scheme (VGX_LINEAGES_TILE_RECORDS; 7 popNum V int32 cells in LDS); no scan follows.  All work after the cuts is integer addition:
 * no value depends on the tile size, the launch geometry or the number of passes (VGX_GENEALOGY_CHUNK_BYTES).  `summary` is the
 * column summary over `counts` as a matrix [n][(T + 1) * popNum * V * 7] where it lies, refused as vgx_get_lineages refuses it;
 * `counts` may be NULL.  Preconditions, checks and refusals are those of vgx_get_lineages, worded behind "vgx_get_tree_events: ",
 * and 7 * popNum * V * 4 bytes of cells above the 65536 bytes of LDS a binning workgroup may use. */
typedef struct vgx_tree_events_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][4] PCG64 start of every walk */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t *counts;                             /* NULL or host [n][T + 1][P][V][7] */
    int64_t *status, *status_arg;                /* [n] 0 or why the walk stopped, as vgx_genealogies_io */
    int64_t *records;                            /* [n] lineage records of the walk (0 for a walk that failed) */
    uint64_t *rng_out;                           /* [n][4] generator state after the walk */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][(T+1)*P*V*7]; group_of has n entries */
    int64_t passes;                              /* out: walk passes */
    double ms[3];                                /* out: kernels (device time), host clock, whole call */
    double kernel_ms[2];                         /* out: the walk and binning kernels of ms[0] apart */
} vgx_tree_events_io;
int vgx_get_tree_events(vgx_engine *e, vgx_tree_events_io *io);
/* Test hook: vgx_test_lineages with the binning of vgx_get_tree_events (the same walk and observer, the host tile walk of
 * vgx_tree_events.h, tile after tile of `tile` records, 0: the default).  counts [T + 1][P][V][7] is overwritten. */
int vgx_test_tree_events(vgx_genealogy_io *io, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                         int32_t *counts, int64_t *records, char *errbuf, int64_t errcap);

/* The same counts for many replicates of the last vgx_simulate_tau call: the walk, chain, event indices, cuts, checks and refusals of
 * vgx_get_tau_lineages (worded behind "vgx_get_tau_tree_events: ") with the binning kernel and the LDS limit of vgx_get_tree_events.
 * All records of a step carry the step's event index, so a grid time exactly at a step's time has the whole step in the intervals
 * up to it.  kernel_ms: the canonicalise, walk and binning kernels of ms[0] apart; ms[1] is the host's cuts. */
typedef struct vgx_tau_tree_events_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][6] start of every walk, as vgx_tau_lineages_io */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t *counts;                             /* NULL or host [n][T + 1][P][V][7] */
    int64_t *status, *status_arg;                /* [n] 0 or why the walk stopped, as vgx_tau_genealogies_io */
    int64_t *records;                            /* [n] lineage records of the walk (0 for a walk that failed) */
    uint64_t *rng_out;                           /* [n][6] generator state after the walk */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][(T+1)*P*V*7]; group_of has n entries */
    int64_t passes;                              /* out: walk passes */
    double ms[3];                                /* out: kernels (device time), host cuts, whole call */
    double kernel_ms[3];                         /* out: the canonicalise, walk and binning kernels of ms[0] apart */
} vgx_tau_tree_events_io;
int vgx_get_tau_tree_events(vgx_engine *e, vgx_tau_tree_events_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: vgx_test_tau_lineages with the binning of vgx_get_tau_tree_events.  counts [T + 1][P][V][7] is overwritten. */
int vgx_test_tau_tree_events(vgx_genealogy_io *io, int64_t sites, const double *grid, int64_t T, const int32_t *variant_of, int64_t V, int64_t tile,
                             int32_t *counts, int64_t *records, char *errbuf, int64_t errcap);

/* ---- tree shapes: balance, depth and branch statistics of every replicate's sampled tree ---------------------------------- */
/* One row of scalars per selected replicate of the last vgx_simulate_direct call: the walk of vgx_get_genealogies
 * (same draws, status and generator afterwards), then one kernel that reduces every tree where the walk left it.  A tree of a walk
 * with status 0 has N = 2 sCounter - 1 nodes in creation order: tree[N - 1] == -1 is the root, i < tree[i] < N otherwise, every node
 * has no children (a tip) or two, and node times do not increase with the id.  With n_v the tips below node v, minkid_v the smaller
 * of its two children's n, tipkids_v its tip children, and lad_v = 1 + max over children of lad_c where tipkids_v == 1, else 0:
 *   stats[r][k]  int64 [n][12]: 0 tips, 1 internal, 2 cherries (tipkids == 2), 3 pitchforks (n_v == 3), 4 sackin (sum of the tips'
 *                depths), 5 colless (sum over internal nodes of n_v - 2 minkid_v), 6 max_depth (edges), 7 depth_sumsq (sum of the
 *                tips' squared depths: wraps beyond about 2 * 10^6 tips of a caterpillar tree), 8 ladder_nodes (tipkids == 1),
 *                9 max_ladder (max lad_v), 10 root_event, 11 last_tip_event (the event indices of node N - 1 and node 0)
 *   lengths[r][k] f64 [n][7]: with b_i = times[i] - times[tree[i]] >= 0: 0 root_time, 1 last_tip_time (times of node N - 1 and node
 *                0), 2 length (sum b_i), 3 external_length (sum over tips), 4 length_sumsq (sum b_i^2), 5 tip_height_sum (sum over
 *                tips of times[i] - root_time), 6 max_branch.  0, 1 and 6 are exact; the four sums are taken in the kernel's order,
 *                within 2 (N + 2) 2^-53 of their value of any other order.
 * A replicate whose walk fails gets its status (as vgx_genealogies_io), zeros and NaN lengths and does not fail the call; a tree
 * that breaks the structure above gets status 13 (status_arg = the first offending node; vgx_genealogy_message has its text).  There
 * is no sizing call: the walk's record capacities are counted inside.  Per pass (sized as vgx_get_genealogies sizes its passes, the
 * node times and 44 bytes of accumulators per node added; VGX_GENEALOGY_CHUNK_BYTES) only the 4-byte node event indices come to the
 * host and the 8-byte node times of the host clock go back.  Preconditions and refusals are those of vgx_get_genealogies, worded
 * behind "vgx_get_tree_shapes: "; replicates must be distinct. */
typedef struct vgx_tree_shapes_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][4] PCG64 start of every walk */
    int64_t *stats;                              /* [n][12] */
    double *lengths;                             /* [n][7] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][4] generator state after the walk */
    int64_t passes;                              /* out: device passes */
    double ms[4];                                /* out: walk kernel, shape kernel (device time), host clock with the two node copies, whole call */
} vgx_tree_shapes_io;
int vgx_get_tree_shapes(vgx_engine *e, vgx_tree_shapes_io *io);
/* Test hook: the sequential sweep of vgx_tree_shape.h on one tree of `nodes` nodes on the host.  Refuses (message in errbuf, naming
 * the first offending node) a tree that breaks the structure above. */
int vgx_test_tree_shape(const int32_t *tree, const int32_t *node_ev, const double *times, int64_t nodes, int64_t *stats, double *lengths,
                        char *errbuf, int64_t errcap);
/* Test hook: n given trees (tree t: nodes node_off[t] .. node_off[t + 1] of the three arrays) through the kernel of
 * vgx_get_tree_shapes on the current device's default stream; no engine.  stats [n][12], lengths [n][7], status [n][2] (status and
 * its argument: 0, or 13 and the node; that tree's row holds zeros and NaN).  Parents outside i < tree[i] < N (-1 at the last node)
 * and node counts that are even or below 3 are refused before anything is uploaded. */
int vgx_test_tree_shape_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int32_t *node_ev, const double *times,
                               int64_t *stats, double *lengths, int64_t *status, char *errbuf, int64_t errcap);

/* The same rows for many replicates of the last vgx_simulate_tau call (with the event log), with nothing of a tree crossing to the
 * host.  The walk is that of vgx_get_tau_genealogies over the same chain (`prefix` as that call takes it): the same
 * draws in the same order from rng_state, the same status and status_arg and the same six generator words afterwards (rng_out).  A
 * tau chain needs no clock.  A node carries the chain's EVENT index: prefix events 0 .. prefix->ev_ptr - 1, the replicate's own step
 * k is prefix->ev_ptr + k (k alone for a replicate that restarted), -1 for a node no event made.  Its time is
 *   0.0 for -1;  the prefix event's time (a MULTITYPE event of an earlier tau call: the time of its first row);  the time of the
 *   step's MULTITYPE record otherwise,
 * the lookup of vgx_get_tau_genealogies with its branches in its order, so every time has the bits that call delivers.  All rows of
 * a step share the step's time: coalescences inside one step give branches of length 0 (they count in the integer statistics as
 * any other branch and add 0 to the sums; max_branch stays >= 0).  Per pass (sized as vgx_get_tau_genealogies sizes its passes, 8
 * bytes of node time and 44 bytes of accumulators per node and the step times added; VGX_GENEALOGY_CHUNK_BYTES): the canonicalise
 * kernel, the one synchronisation that sizes the walk's workspace from its report, then the walk kernel, the node-time kernel
 * (vgx_tau_tree_shapes.hip) and the shape kernel of vgx_get_tree_shapes on one stream with no host step between them.  stats,
 * lengths, status 13 and a failed walk's row as vgx_tree_shapes_io; statuses 10 .. 12 as vgx_tau_genealogies_io.  There is no
 * sizing call: the record capacities are those the sizing call of vgx_get_tau_genealogies gives, counted inside.  An event index
 * outside a chain (no healthy walk leaves one) fails the call with "vgx_get_tau_tree_shapes: an event index outside the chain".
 * Preconditions and refusals as vgx_get_tau_genealogies (the last call was vgx_simulate_tau, it recorded rows, the prefix length,
 * replicates distinct and in range, contiguous row ranges, the chain's length, prefix rows inside the model), worded behind
 * "vgx_get_tau_tree_shapes: ". */
typedef struct vgx_tau_tree_shapes_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][6] start of every walk: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger */
    int64_t *stats;                              /* [n][12] */
    double *lengths;                             /* [n][7] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][6] generator state after the walk */
    int64_t passes;                              /* out: device passes */
    double ms[3];                                /* out: kernels (device time), host part (descriptors and step-time tables), whole call */
    double kernel_ms[4];                         /* out: the canonicalise, walk, node-time and shape kernels of ms[0] apart */
} vgx_tau_tree_shapes_io;
int vgx_get_tau_tree_shapes(vgx_engine *e, vgx_tau_tree_shapes_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: the node-time rule (vgx_tau_tree_shape.h) over one tree's node event indices on the host: times[k] for node_ev[k] in a
 * chain of n_pre prefix events (times pre_times[n_pre]) and n_steps own steps (step_times[n_steps]).  An index below 0 gives 0.0; an
 * index of n_pre + n_steps or more is refused (message in errbuf, naming the node). */
int vgx_test_tau_node_times(const int32_t *node_ev, int64_t nodes, int64_t n_pre, const double *pre_times, int64_t n_steps,
                            const double *step_times, double *times, char *errbuf, int64_t errcap);
/* Test hook: n given trees (tree t: nodes node_off[t] .. node_off[t + 1] of node_ev and times, n_pre[t] prefix events out of the
 * shared table pre_times[n_pre_times], own step times step_times[step_off[t] .. step_off[t + 1]]) through the node-time kernel of
 * vgx_get_tau_tree_shapes on the current device's default stream; no engine.  bad [n]: the lowest node of tree t whose index lies
 * outside its chain (its time is 0.0), INT32_MAX for none.  Unlike vgx_test_tree_shape_device such an index does reach the device:
 * the kernel compares every index with the lengths of its two tables before it loads.  Offsets that decrease and an n_pre outside
 * the shared table are refused before anything is uploaded. */
int vgx_test_tau_node_times_device(int64_t n, const int64_t *node_off, const int32_t *node_ev, const int64_t *n_pre, int64_t n_pre_times,
                                   const double *pre_times, const int64_t *step_off, const double *step_times, double *times, int32_t *bad,
                                   char *errbuf, int64_t errcap);

/* ---- mutation spectrum: clade sizes of every replicate's mutation records ------------------------------------------------- */
/* One row of integers per selected replicate of the last vgx_simulate_direct call: the walk of vgx_get_genealogies
 * (same draws, status and generator afterwards), then one kernel that reduces the walk's mutation records (mut_node, mut_AS, mut_DS,
 * mut_site) over the tree where the walk left both.  The tree is that of vgx_tree_shapes_io (N = 2 sCounter - 1 nodes, parents of a
 * higher id, none or two children).  clade[i] is the number of tips below node i; record k sits on the branch above mut_node[k], so
 * its frequency in the sample is c_k = clade[mut_node[k]]; a record on the root has c = tips.  Every record is one mutation event
 * (the infinite-sites reading of a model with recurrent mutation).  With S = the model's sites (0 .. 15; a model without sites has empty per-site blocks):
 *   spectrum[r][s][b]        int64 [n][S][32]: records of site s with floor(log2 c) == b (bin 0: the singletons; bin 31 stays 0)
 *   substitutions[r][s][a][d] int64 [n][S][4][4]: records by site, AS and DS
 *   sums[r][s][k]            int64 [n][S][3]: 0 clade_sum (sum c), 1 clade_sumsq (sum c^2), 2 pair_sum (sum c (tips - c)); wrapping:
 *                            clade_sumsq is below mutations * tips^2 and wraps only beyond 2^63 / tips^2 records (8 * 10^6 records
 *                            on the root at 10^6 tips)
 *   stats[r][k]              int64 [n][4]: 0 tips, 1 mutations, 2 fixed (records with c == tips), 3 max_clade (0 without records)
 * Sums, counts and one maximum of integers: every path gives the same bits.  No node time is read and no host clock runs: only the
 * rows, the status pairs and the generator words come to the host (vgx_clock_mismatches is not touched).  A replicate whose walk
 * fails gets its status (as vgx_genealogies_io) and zeros and does not fail the call; a tree that breaks the structure gets status
 * 13 (status_arg = the first offending node); a record with mut_node outside [0, N), mut_site outside [0, S) or mut_AS / mut_DS
 * outside 0 .. 3 (no healthy walk leaves one) gives status 14 (status_arg = the lowest such record index) and zeros;
 * vgx_genealogy_message has both texts.  There is no sizing call: the walk's record capacities are counted inside.  Passes are sized
 * as vgx_get_genealogies sizes its passes, 16 bytes of workspace per node and the rows added (VGX_GENEALOGY_CHUNK_BYTES).
 * Preconditions and refusals are those of vgx_get_tree_shapes, worded behind "vgx_get_mutation_spectrum: "; replicates must be
 * distinct. */
typedef struct vgx_mutation_spectrum_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][4] PCG64 start of every walk */
    int64_t *spectrum;                           /* [n][sites][32] */
    int64_t *substitutions;                      /* [n][sites][4][4] */
    int64_t *sums;                               /* [n][sites][3] */
    int64_t *stats;                              /* [n][4] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][4] generator state after the walk */
    int64_t sites;                               /* out: the model's sites (the caller sizes the blocks with vgx_dims.sites) */
    int64_t passes;                              /* out: device passes */
    double ms[3];                                /* out: walk kernel, spectrum kernel (device time), whole call */
} vgx_mutation_spectrum_io;
int vgx_get_mutation_spectrum(vgx_engine *e, vgx_mutation_spectrum_io *io);
/* The same rows for many replicates of the last vgx_simulate_tau call (with the event log).  The walk is that of
 * vgx_get_tau_genealogies over the same chain (`prefix` as that call takes it): the same draws from rng_state, the same status and
 * status_arg and the same six generator words afterwards.  Per pass (sized as vgx_get_tau_genealogies sizes its passes, 16 bytes of
 * workspace per node and the rows added; VGX_GENEALOGY_CHUNK_BYTES): the canonicalise kernel, the one synchronisation that sizes the
 * walk's workspace from its report, then the walk kernel and the spectrum kernel on one stream with no host step between them; no
 * node-time kernel and no step times.  Rows, statuses 13 and 14 and a failed walk's row as vgx_mutation_spectrum_io; statuses
 * 10 .. 12 as vgx_tau_genealogies_io.  Preconditions and refusals as vgx_get_tau_tree_shapes, worded behind
 * "vgx_get_tau_mutation_spectrum: ". */
typedef struct vgx_tau_mutation_spectrum_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][6] start of every walk: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger */
    int64_t *spectrum;                           /* [n][sites][32] */
    int64_t *substitutions;                      /* [n][sites][4][4] */
    int64_t *sums;                               /* [n][sites][3] */
    int64_t *stats;                              /* [n][4] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][6] generator state after the walk */
    int64_t sites;                               /* out: the model's sites */
    int64_t passes;                              /* out: device passes */
    double ms[3];                                /* out: kernels (device time), host part (descriptors), whole call */
    double kernel_ms[3];                         /* out: the canonicalise, walk and spectrum kernels of ms[0] apart */
} vgx_tau_mutation_spectrum_io;
int vgx_get_tau_mutation_spectrum(vgx_engine *e, vgx_tau_mutation_spectrum_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: the sequential sweep of vgx_mutation_spectrum.h (the definition) on one tree of `nodes` nodes and `muts` records on the
 * host.  spectrum [sites][32], substitutions [sites][4][4], sums [sites][3], stats [4]; clade NULL or [nodes].  Refuses (message in
 * errbuf) a tree that breaks the structure, naming the node, and a record outside the tree or the model, naming the record. */
int vgx_test_mutation_spectrum(const int32_t *tree, int64_t nodes, const int32_t *mut_node, const int32_t *mut_AS, const int32_t *mut_DS,
                               const int32_t *mut_site, int64_t muts, int64_t sites, int64_t *spectrum, int64_t *substitutions, int64_t *sums,
                               int64_t *stats, int32_t *clade, char *errbuf, int64_t errcap);
/* Test hook: n given trees (tree t: nodes node_off[t] .. node_off[t + 1] of `tree`, records mut_off[t] .. mut_off[t + 1] of the four
 * record arrays) through the kernel of vgx_get_mutation_spectrum on the current device's default stream; no engine.  walk_status NULL,
 * or [n][2] a walk status and its argument per tree: a tree whose status is not 0 is skipped as the calls skip a failed walk.
 * spectrum [n][sites][32], substitutions [n][sites][4][4], sums [n][sites][3], stats [n][4], status [n][2] (0; the given walk status;
 * 13 and the node; 14 and the record: the last three with an all-zero row); clade NULL or [node_off[n]] (zeros for a tree that was
 * skipped, unspecified for one that got 13).  Offsets that decrease, node counts that are even or below 3 and parents outside i < tree[i] < N (-1 at the
 * last node) are refused before anything is uploaded.  A bad RECORD does reach the device: the kernel compares every record with
 * N, sites and 0 .. 3 before it uses it. */
int vgx_test_mutation_spectrum_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int64_t *mut_off, const int32_t *mut_node,
                                      const int32_t *mut_AS, const int32_t *mut_DS, const int32_t *mut_site, int64_t sites,
                                      const int64_t *walk_status, int64_t *spectrum, int64_t *substitutions, int64_t *sums, int64_t *stats,
                                      int64_t *status, int32_t *clade, char *errbuf, int64_t errcap);

/* ---- introductions: the transmission lineages of every replicate's tree ------------------------------------------------------- */
/* One row of integers per selected replicate of the last vgx_simulate_direct call: the walk of vgx_get_genealogies
 * (same draws, status and generator afterwards), then one kernel that reduces the walk's node labels (tree_pop) over the tree
 * where the walk left both.  The tree is that of vgx_tree_shapes_io (N = 2 sCounter - 1 nodes, parents of a higher id, none or two
 * children).  The branch above node i crosses when pop[tree[i]] != pop[i]: it is then one NET introduction from src = pop[tree[i]]
 * into dst = pop[i] (moves along a branch that left no node are invisible: 0 -> 2 -> 1 counts as 0 -> 1, 0 -> 1 -> 0 not at all;
 * the walk's migration records are not read).  clade[i] is the number of tips below node i, local[i] the number of those reached
 * without passing a crossing branch.  The root and every node below a crossing branch head a transmission lineage of size
 * local[i] (possibly 0) in population pop[i]; every tip lies in exactly one.  With P = the model's populations (1 .. 1024: a row
 * holds P^2 + 39 P + 8 cells, 8.7 MB at 1024; more is refused with VGX_ERR_ARG):
 *   tips_by_pop[r][p]       int64 [n][P]: tips by population
 *   imports[r][src][dst]    int64 [n][P][P]: crossing branches by source and destination; the diagonal is 0
 *   into[r][dst][k]         int64 [n][P][6] over the introductions into dst: 0 count, 1 clade_sum, 2 local_sum, 3 local_sumsq, 4 empty
 *                           (local == 0), 5 max_local.  local_sumsq <= tips^2 <= 2^60 and clade_sum < 2 tips^2: nothing wraps on a
 *                           tree the walk can make (tips <= 2^30); the sums are wrapping adds regardless
 *   spectrum[r][dst][b]     int64 [n][P][32]: introductions into dst with floor(log2 local) == b, local >= 1 (bin 0: the singletons;
 *                           the empty ones are counted in into alone; bin 31 stays 0)
 *   stats[r][k]             int64 [n][8]: 0 tips, 1 introductions, 2 root_pop, 3 root_local, 4 max_local (the root's lineage
 *                           included), 5 max_clade (over the introductions), 6 empty, 7 populations with at least one tip
 * Counts, sums and maxima of integers: every path gives the same bits.  No node time is read and no host clock runs: only the
 * rows, the status pairs, the walk's result and the generator words come to the host (vgx_clock_mismatches is not touched).  A
 * replicate whose walk fails gets its status (as vgx_genealogies_io) and zeros and does not fail the call; a tree that breaks the
 * structure gets status 13 (status_arg = the first offending node); a node label outside [0, P) (no healthy walk leaves one) gives
 * status 15 (status_arg = the lowest such node) and zeros; the tree is judged before the labels; vgx_genealogy_message has both
 * texts.  There is no sizing call: the walk's record capacities are counted inside.  Passes are sized as vgx_get_genealogies sizes
 * its passes, 16 bytes of workspace per node and the rows added (VGX_GENEALOGY_CHUNK_BYTES).  Preconditions and refusals are those
 * of vgx_get_mutation_spectrum, worded behind "vgx_get_introductions: "; replicates must be distinct. */
typedef struct vgx_introductions_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][4] PCG64 start of every walk */
    int64_t *tips_by_pop;                        /* [n][pops] */
    int64_t *imports;                            /* [n][pops][pops] */
    int64_t *into;                               /* [n][pops][6] */
    int64_t *spectrum;                           /* [n][pops][32] */
    int64_t *stats;                              /* [n][8] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][4] generator state after the walk */
    int64_t pops;                                /* out: the model's populations (the caller sizes the blocks with vgx_dims.popNum) */
    int64_t passes;                              /* out: device passes */
    double ms[3];                                /* out: walk kernel, lineage kernel (device time), whole call */
} vgx_introductions_io;
int vgx_get_introductions(vgx_engine *e, vgx_introductions_io *io);
/* The same rows for many replicates of the last vgx_simulate_tau call (with the event log).  The walk is that of
 * vgx_get_tau_genealogies over the same chain (`prefix` as that call takes it): the same draws from rng_state, the same status and
 * status_arg and the same six generator words afterwards.  Per pass (sized as vgx_get_tau_genealogies sizes its passes, 16 bytes of
 * workspace per node and the rows added; VGX_GENEALOGY_CHUNK_BYTES): the canonicalise kernel, the one synchronisation that sizes the
 * walk's workspace from its report, then the walk kernel and the lineage kernel on one stream with no host step between them; no
 * node-time kernel and no step times.  Rows, statuses 13 and 15 and a failed walk's row as vgx_introductions_io; statuses
 * 10 .. 12 as vgx_tau_genealogies_io.  Preconditions and refusals as vgx_get_tau_mutation_spectrum, worded behind
 * "vgx_get_tau_introductions: ". */
typedef struct vgx_tau_introductions_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    const uint64_t *rng_state;                   /* [n][6] start of every walk: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger */
    int64_t *tips_by_pop;                        /* [n][pops] */
    int64_t *imports;                            /* [n][pops][pops] */
    int64_t *into;                               /* [n][pops][6] */
    int64_t *spectrum;                           /* [n][pops][32] */
    int64_t *stats;                              /* [n][8] */
    int64_t *status, *status_arg;                /* [n] */
    uint64_t *rng_out;                           /* [n][6] generator state after the walk */
    int64_t pops;                                /* out: the model's populations */
    int64_t passes;                              /* out: device passes */
    double ms[3];                                /* out: kernels (device time), host part (descriptors), whole call */
    double kernel_ms[3];                         /* out: the canonicalise, walk and lineage kernels of ms[0] apart */
} vgx_tau_introductions_io;
int vgx_get_tau_introductions(vgx_engine *e, vgx_tau_introductions_io *io, const vgx_tau_genealogy_prefix *prefix);
/* Test hook: the sequential sweep of vgx_introductions.h (the definition) on one tree of `nodes` nodes with labels `pop` on the
 * host.  tips_by_pop [pops], imports [pops][pops], into [pops][6], spectrum [pops][32], stats [8]; clade and local NULL or [nodes].
 * Refuses (message in errbuf) a tree that breaks the structure, naming the node, and a label outside [0, pops), naming the node. */
int vgx_test_introductions(const int32_t *tree, const int32_t *pop, int64_t nodes, int64_t pops, int64_t *tips_by_pop, int64_t *imports,
                           int64_t *into, int64_t *spectrum, int64_t *stats, int32_t *clade, int32_t *local, char *errbuf, int64_t errcap);
/* Test hook: n given trees (tree t: nodes node_off[t] .. node_off[t + 1] of `tree` and `pop`) through the kernel of
 * vgx_get_introductions on the current device's default stream; no engine.  walk_status NULL, or [n][2] a walk status and its
 * argument per tree: a tree whose status is not 0 is skipped as the calls skip a failed walk.  tips_by_pop [n][pops], imports
 * [n][pops][pops], into [n][pops][6], spectrum [n][pops][32], stats [n][8], status [n][2] (0; the given walk status; 13 and the
 * node; 15 and the node: the last three with an all-zero row).  Offsets that decrease, node counts that are even or below 3 and
 * parents outside i < tree[i] < N (-1 at the last node) are refused before anything is uploaded.  A bad LABEL does reach the device:
 * the kernel compares every label with pops before anything indexes by it. */
int vgx_test_introductions_device(int64_t n, const int64_t *node_off, const int32_t *tree, const int32_t *pop, int64_t pops,
                                  const int64_t *walk_status, int64_t *tips_by_pop, int64_t *imports, int64_t *into, int64_t *spectrum,
                                  int64_t *stats, int64_t *status, char *errbuf, int64_t errcap);

/* The same counts for many replicates of the last vgx_simulate_tau call (with the event log), on the device.
 * A tau replicate's chain is a list of weighted rows (num, type, haplotype, population, newHaplotype, newPopulation), six int64:
 * the events the model held when the call started (`prefix`, as vgx_get_tau_timelines takes it; its lockdown columns are not
 * read), flattened (a direct event = a row with num 1, a MULTITYPE event of an earlier tau call = its multievent rows), then the
 * replicate's own rows where the tau kernels left them (nothing of them is copied or compacted).  A replicate that restarted
 * (vgx_counters.restarts > 0) has no prefix.  An EVENT is a direct event or a step, and a step's time is the time of its MULTITYPE
 * record: this is where the reference's own replays place a step's events.  The cuts are row indices:
 * cut[k] = first row of the first event i with edges[k] <= t_i (the row count if none), by the same literal loop over events (an
 * event without rows still advances it; its cut is the first row after it); row j is in bin b when cut[b] <= j < cut[b + 1], so
 * all rows of a step share a bin.  A row counts `num` times in the cells of vgx_get_incidence (same channels, keys, double count
 * of MIGRATION and haplotype filter; num <= 0 counts nothing; a field that is not a 32-bit index matches nothing).
 * outside[r] = (sum of num over the rows before cut[0], over the rows from cut[T] on), over num > 0, unfiltered.
 * Counts are int64: a bin sums num over many steps.  The LDS histogram is popNum * 56 bytes (popNum <= 1170).
 * No host clock runs (step times are host doubles).  With one grid the prefix is the same part of every chain that carries it: it
 * is flattened, uploaded and counted ONCE per call into a block of its own; the block of every replicate that did not restart
 * starts from it, and the replicate's own rows are added (a workgroup per replicate and tile of VGX_INCIDENCE_TILE_EVENTS rows).
 * Replicates go in chunks under VGX_TIMELINES_CHUNK_BYTES.  `summary` as in vgx_get_incidence: a device pass narrows the block to
 * int32 for it; if a count is 2^31 or more the summary is refused (VGX_ERR_ARG, the largest count in the message) after `counts`,
 * if asked for, has been written.  ms[1] is the host's cut search.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_tau_incidence: "): the last call was not vgx_simulate_tau; it recorded no
 * rows; a replicate that did not restart continues a log of another length than prefix->ev_ptr; prefix plus own rows reach 2^31;
 * a null prefix column; bad edges; T outside [1, 2^24); replicates out of range or given twice; the block (8 bytes per cell, 4
 * more with a summary) above half of the free device memory; the LDS limit. */
typedef struct vgx_tau_incidence_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *edges;              /* [T + 1] strictly increasing, finite */
    const uint32_t *hap_mask;                    /* NULL or ceil(hapNum / 32) words */
    int64_t *counts;                             /* NULL or host [n][T][P][7] */
    int64_t *outside;                            /* [n][2] */
    vgx_traj_summary_io *summary;                /* NULL or the summary of the [n][T*P*7] block; group_of has n entries */
    int64_t passes; double ms[3];                /* out: counting launches; kernels, host cut search, whole call */
} vgx_tau_incidence_io;
int vgx_get_tau_incidence(vgx_engine *e, vgx_tau_incidence_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: the flattening, cuts, cells and tile walk of vgx_get_tau_incidence compiled for the host, on one chain given as
 * event columns and multievent columns (no device, no engine), tile after tile of `tile` rows (0: the default).  The last
 * n_own_events events play the replicate's own steps (-1: the chain's trailing MULTITYPE events), everything before them the
 * prefix; the prefix is counted once as a chain of its own and added, as on the device.  Prefix rows pass the checks of the
 * flattening (a negative num or a field outside 32 bits is refused); own rows are taken as they are, as the device reads them.
 * counts [T][P][7] and outside [2] are overwritten.  Refused with the message in errbuf: bad edges, P * 56 bytes above the LDS
 * budget, a MULTITYPE row range outside the multievent log. */
typedef struct vgx_tau_incidence_chain {
    int64_t popNum, hapNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t T; const double *edges;              /* [T + 1] */
    const uint32_t *hap_mask;
    int64_t tile, n_own_events;
    int64_t *counts;                             /* out [T][P][7] */
    int64_t *outside;                            /* out [2] */
} vgx_tau_incidence_chain;
int vgx_test_tau_incidence(vgx_tau_incidence_chain *io, char *errbuf, int64_t errcap);

/* vgx_get_flows for many replicates of the last vgx_simulate_tau call (with the event log), on the device.
 * The chain, the events, the cuts in row index space and `outside` are vgx_get_tau_incidence's, unchanged: `prefix` flattened,
 * then the replicate's own rows where the tau kernels left them; a replicate that restarted has no prefix; an event is a direct
 * event or a whole step at the time of its MULTITYPE record; outside[r] = (sum of num over the rows before cut[0], over the rows
 * from cut[T] on), over num > 0, unfiltered.  A row (num, type, haplotype, population, newHaplotype, newPopulation) counts `num`
 * times in the one cell vgx_get_flows gives for its five fields (VGX_TL_ROW_DIRECT masked off the type; variant_of, `within`, a
 * BIRTH on the diagonal, a MIGRATION at (population, newPopulation) literally); num <= 0 counts nothing, a field that is not a
 * 32-bit index matches nothing.  The block is int64 counts[n][T][popNum][popNum][V]; with hap_mask = the members of class c its
 * margins are vgx_get_tau_incidence's channels (sum over src = 0 + 5, off-diagonal sum over dst = 6, diagonal = 0 unless a
 * MIGRATION has equal keys).
 * The two forms of vgx_get_flows with 8-byte cells: dense keeps popNum^2 * V int64 cells in LDS (popNum <= 90 at V = 1), split
 * the popNum * V cells of the diagonal, a row off the diagonal then adding num to its cell in device memory at once.  Dense runs
 * where it fits, else split; VGX_FLOWS_FORM=dense|split forces one; `form` reports the one that ran (1 dense, 2 split).  A
 * workgroup takes one chain and a tile of VGX_FLOWS_TILE_EVENTS consecutive rows (default 4096).  All of it is integer work: no
 * result depends on the form, the tile size, the launch geometry or the chunking.  No host clock runs.  The prefix is flattened,
 * uploaded and counted ONCE per call into a block of its own; the block of every replicate that did not restart starts from it.
 * Replicates go in chunks under VGX_TIMELINES_CHUNK_BYTES.  `summary` as in vgx_get_tau_incidence: a device pass narrows the block
 * to int32 for it; if a count is 2^31 or more the summary is refused (VGX_ERR_ARG, the largest count in the message) after
 * `counts`, if asked for, has been written; with counts = NULL no block is copied to the host.  ms[1] is the host's cut search.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_tau_flows: "): the last call was not vgx_simulate_tau; it recorded no rows;
 * a replicate that did not restart continues a log of another length than prefix->ev_ptr; prefix plus own rows reach 2^31; a null
 * prefix column; bad edges; T outside [1, 2^24); replicates out of range or given twice; V < 1 or a variant_of value outside
 * [-1, V); popNum * V * 8 bytes of diagonal cells above the 65536 bytes of LDS a counting workgroup may use, or the dense form
 * forced where popNum^2 * V * 8 bytes are (the message gives the bytes); a value of VGX_FLOWS_FORM that is neither; a block of
 * 2^40 cells or more; the block (8 bytes per cell, 4 more with a summary) and the prefix block above half of the free device
 * memory (the message gives the bytes: select fewer replicates). */
typedef struct vgx_tau_flows_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *edges;              /* [T + 1] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int32_t within;                              /* 1: births count on the diagonal; 0: migrations alone */
    int64_t *counts;                             /* NULL or host [n][T][P][P][V] */
    int64_t *outside;                            /* [n][2] */
    vgx_traj_summary_io *summary;                /* NULL or the summary of the [n][T*P*P*V] block; group_of has n entries */
    int64_t form, passes; double ms[3];          /* out: the form that ran (1 dense, 2 split); counting launches; kernels, host cut search, whole call */
} vgx_tau_flows_io;
int vgx_get_tau_flows(vgx_engine *e, vgx_tau_flows_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: the flattening, cuts, cell and tile walk of vgx_get_tau_flows compiled for the host, on one chain given as event
 * columns and multievent columns (no device, no engine), tile after tile of `tile` rows (0: the default), in the form `form` asks
 * for (0: the automatic choice, 1 dense, 2 split).  n_own_events, the prefix and the own rows as in vgx_test_tau_incidence: the
 * prefix is counted once as a chain of its own and added, as on the device.  counts [T][P][P][V] and outside [2] are overwritten,
 * form_ran gets the form that ran.  Refused with the message in errbuf: bad edges, V or variant_of, a form that does not fit the
 * LDS budget, a negative tile, a MULTITYPE row range outside the multievent log, a prefix row the flattening refuses. */
typedef struct vgx_tau_flows_chain {
    int64_t popNum, hapNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t T; const double *edges;              /* [T + 1] */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int64_t within;                              /* 0: migrations alone */
    int64_t tile, form, n_own_events;
    int64_t *counts;                             /* out [T][P][P][V] */
    int64_t *outside;                            /* out [2] */
    int64_t form_ran;                            /* out: 1 dense, 2 split */
} vgx_tau_flows_chain;
int vgx_test_tau_flows(vgx_tau_flows_chain *io, char *errbuf, int64_t errcap);

/* vgx_get_prevalence for many replicates of the last vgx_simulate_tau call (with the event log), on the device.
 * The chain is that of vgx_get_tau_incidence: weighted rows (num, type, haplotype, population, newHaplotype, newPopulation), six
 * int64: `prefix` flattened, then the replicate's own rows where the tau kernels left them; a replicate that restarted has no
 * prefix.  An EVENT is a direct event or a step, with the time of its log record.  The bounds are row indices:
 * cut[j] = first row of the first event i with grid[j] < t_i (the row count if none), by the literal loop over events (an event
 * without rows still advances it; its cut is the first row after it).  The comparison is strict, as vgx_get_prevalence's and the
 * tau trajectories' is: all rows of a step share an interval, and a grid point at exactly a step's time has the step applied.
 * A row changes the cells of vgx_get_prevalence's table with sign * num: VGX_TL_ROW_DIRECT is masked off the type, a field that
 * is not a 32-bit index matches nothing, a row with num <= 0 changes nothing.
 *   values[r][j] = start_r + the sum of the changes of the intervals 0 .. j,   final[r] = the same over all T + 1 intervals
 * outside[r] = (sum of num over the rows before cut[0], over the rows from cut[T-1] on), over num > 0.
 * start_r is the state the chain starts from, folded through variant_of: the model's initial state (what vgx_get_state gives as
 * initial_infectious) when the replicate restarted (vgx_counters.restarts > 0) or the prefix is not empty, since the chain then
 * starts at the beginning of the model's history; otherwise the state the call started from (the host state after its first-call
 * preparation, the index case included), which is the source vgx_get_prevalence uses for its rows that did not restart.  With
 * every haplotype tracked final[r] is the replicate's final infectious state (vgx_get_tau_states_all).
 * Cells and values are int64: an interval sums num over many steps.  A counting workgroup takes one chain and a tile of
 * VGX_PREVALENCE_TILE_EVENTS rows (default 4096), finds its first interval by a search in the chain's bounds, accumulates the
 * signed num in popNum * V int64 cells in LDS and adds the nonzero cells to a block of net changes in device memory at every
 * interval change and at the tile's end; rows outside [cut[0], cut[T-1]) still count, in interval 0 or the tail.  With one grid
 * the prefix is the same part of every chain that carries it: it is flattened, uploaded and counted ONCE per call into a net block
 * of its own; the net block of every replicate that did not restart starts from it (value intervals, tail and `outside`), the
 * replicate's own rows are added, and a scan kernel turns every (replicate, population, class) column into running sums (wrapping
 * as unsigned 64-bit integers).  All of it is integer work: no result depends on the tile size, the launch geometry or the
 * chunking.  No host clock runs (step times are host doubles); replicates go in chunks under VGX_TIMELINES_CHUNK_BYTES.
 * `summary` as in vgx_get_prevalence, over `values` as a matrix [n][T * popNum * V]: one device pass narrows the block to int32
 * and finds its minimum and maximum; a value below 0 or of 2^31 or more refuses the summary (VGX_ERR_ARG, the offending value in
 * the message) after values and final, if asked for, have been written.  ms[1] is the host's cut search.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_tau_prevalence: "): the last call was not vgx_simulate_tau; it recorded no
 * rows; a replicate that did not restart continues a log of another length than prefix->ev_ptr; prefix plus own rows reach 2^31;
 * a null prefix column; replicates out of range or given twice; a grid that is not finite or does not increase; T outside
 * [1, 2^24); V < 1 or a variant_of value outside [-1, V); popNum * V * 8 bytes of cells above the 65536 bytes of LDS a counting
 * workgroup may use; a block (8 n (T + 1) popNum V bytes, 4 more per cell with a summary) above half of the free device memory
 * (the message gives the bytes: select fewer replicates). */
typedef struct vgx_tau_prevalence_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int64_t *values;                             /* NULL or host [n][T][P][V] */
    int64_t *final;                              /* NULL or host [n][P][V] */
    int64_t *outside;                            /* [n][2] */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*V]; group_of has n entries */
    int64_t passes; double ms[3];                /* out: counting launches; kernels, host cut search, whole call */
} vgx_tau_prevalence_io;
int vgx_get_tau_prevalence(vgx_engine *e, vgx_tau_prevalence_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: the flattening, bounds, tile walk, prefix-plus-own sum and scan of vgx_get_tau_prevalence compiled for the host, on
 * one chain given as event columns and multievent columns (no device, no engine), tile after tile of `tile` rows (0: the default).
 * The last n_own_events events play the replicate's own steps (-1: the chain's trailing MULTITYPE events), everything before them
 * the prefix; the prefix is counted once as a chain of its own and the own rows' net changes are added, as on the device.  Prefix
 * rows pass the checks of the flattening (a negative num or a field outside 32 bits is refused); own rows are taken as they are,
 * as the device reads them.  start [P][V]: the state the chain starts from, folded.  values [T][P][V], final [P][V] and outside
 * [2] are overwritten.  Refused with the message in errbuf: a bad grid, V or variant_of, P * V * 8 bytes above the LDS budget, a
 * MULTITYPE row range outside the multievent log. */
typedef struct vgx_tau_prevalence_chain {
    int64_t popNum, hapNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t T; const double *grid;               /* [T] */
    int64_t V; const int32_t *variant_of;        /* [hapNum] */
    const int64_t *start;                        /* [P][V] */
    int64_t tile, n_own_events;
    int64_t *values;                             /* out [T][P][V] */
    int64_t *final;                              /* out [P][V] */
    int64_t *outside;                            /* out [2] */
} vgx_tau_prevalence_chain;
int vgx_test_tau_prevalence(vgx_tau_prevalence_chain *io, char *errbuf, int64_t errcap);

/* ---- susceptibles: hosts per immunity group on a common grid ------------------------------------ */
/* How many hosts are immune to what, when: the other half of the state vgx_get_prevalence counts, on the same kind of grid
 * (DESIGN.md §20).  The caller gives grid[0 .. T-1] as for vgx_get_prevalence and a map class_of[susNum] with values in [-1, G):
 * the class of every susceptibility group, -1 = not tracked.  Cuts, intervals, the strict comparison and `outside` are
 * vgx_get_prevalence's, literally.  A log record (type, haplotype, population, newHaplotype, newPopulation) changes
 *   BIRTH              -1 at (population, class_of[newHaplotype])
 *   DEATH, SAMPLING    +1 at (population, class_of[newHaplotype])
 *   SUSCCHANGE         +1 at (population, class_of[newHaplotype]), -1 at (population, class_of[haplotype]); equal classes change nothing
 *   MIGRATION          -1 at (newPopulation, class_of[newHaplotype])
 *   MUTATION           nothing
 * each side only if its class is tracked (the susceptible side of the 'compartment' semantics of vgx_get_timelines folded through
 * class_of: the log keeps the group of the host that leaves or joins the susceptibles in newHaplotype).  A type outside 0..5, a
 * population key outside [0, popNum) or a group outside [0, susNum) counts nowhere; a record changes at most two cells.
 *   values[r][j] = start_r + the sum of the changes of the intervals 0 .. j,   final[r] = the same over all T + 1 intervals
 * where start_r is the susceptible state the call started from folded through class_of, or the initial susceptible state for a
 * replicate that restarted (vgx_counters.restarts > 0).  With every group tracked final[r] is the replicate's final susceptible
 * state (vgx_get_state) folded through class_of, and with every haplotype tracked in a vgx_get_prevalence call on the same grid
 * the two blocks add up to the population sizes at every grid point.
 * The device pass is vgx_get_prevalence's with a counting kernel of its own for this rule (popNum * G int32 cells in LDS,
 * class_of staged behind them when it fits, VGX_PREVALENCE_TILE_EVENTS events per tile) and the same scan, min/max pass and
 * column summary; the host clock runs as there (VGX_TIMELINES_CHUNK_BYTES).  No result depends on the tile size, the launch
 * geometry or the chunking.  `summary` and a NULL `values` as in vgx_get_prevalence.
 * Preconditions and refusals are vgx_get_prevalence's, worded alike behind "vgx_get_susceptibles: " with G and class_of in place
 * of V and variant_of: popNum * G * 4 bytes of cells above the 65536 bytes of LDS a counting workgroup may use, T outside
 * [1, 2^24), a chain of 2^30 events or more, a block above half of the free device memory.  vgx_clock_mismatches counts every
 * selected replicate once. */
typedef struct vgx_susceptibles_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t G; const int32_t *class_of;          /* [susNum], values in [-1, G) */
    int32_t *values;                             /* NULL or host [n][T][P][G] */
    int32_t *final;                              /* NULL or host [n][P][G] */
    int64_t *outside;                            /* [n][2]: events before cut[0] / from cut[T-1] on */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*G]; group_of has n entries */
    int64_t passes; double ms[3];                /* out: launches of the counting kernel; kernels, host clock, whole call */
} vgx_susceptibles_io;
int vgx_get_susceptibles(vgx_engine *e, vgx_susceptibles_io *io);
/* Test hook: the rule, the tile walk and the scan of vgx_get_susceptibles compiled for the host, on one chain given as arrays (no
 * device, no engine), tile after tile with `tile` events each (0: the default).  start [P][G]: whole numbers in [0, 2^31).
 * values [T][P][G], final [P][G] and outside [2] are overwritten.  The same limits: the LDS budget, a chain of 2^30 events, a bad
 * grid, G or class_of are refused with the message in errbuf. */
int vgx_test_susceptibles(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                          const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t susNum,
                          const double *grid, int64_t T, const int32_t *class_of, int64_t G, const int64_t *start, int64_t tile,
                          int32_t *values, int32_t *final, int64_t *outside, char *errbuf, int64_t errcap);

/* vgx_get_susceptibles for many replicates of the last vgx_simulate_tau call (with the event log), on the device: vgx_get_tau_prevalence
 * over the table above.  Rows, bounds, `outside`, the prefix counted once, int64 cells and values, the chunking
 * and the summary are vgx_get_tau_prevalence's: a row changes the cells of the table with sign * num, VGX_TL_ROW_DIRECT is masked
 * off the type, a field that is not a 32-bit index matches nothing, a row with num <= 0 changes nothing.  A MIGRATION row's group
 * is its newHaplotype field, as for a direct record.  start_r is the model's initial susceptible state (initial_susceptible of
 * vgx_get_state) when the replicate restarted or the prefix is not empty, otherwise the susceptible state the call started from,
 * folded through class_of.  With every group tracked final[r] is the replicate's final susceptible state
 * (vgx_get_tau_states_all).  Refusals as vgx_get_tau_prevalence's behind "vgx_get_tau_susceptibles: ", with popNum * G * 8 bytes
 * of cells against the LDS budget. */
typedef struct vgx_tau_susceptibles_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t T; const double *grid;               /* [T] strictly increasing, finite */
    int64_t G; const int32_t *class_of;          /* [susNum], values in [-1, G) */
    int64_t *values;                             /* NULL or host [n][T][P][G] */
    int64_t *final;                              /* NULL or host [n][P][G] */
    int64_t *outside;                            /* [n][2] */
    vgx_traj_summary_io *summary;                /* NULL or the summary of [n][T*P*G]; group_of has n entries */
    int64_t passes; double ms[3];                /* out: counting launches; kernels, host cut search, whole call */
} vgx_tau_susceptibles_io;
int vgx_get_tau_susceptibles(vgx_engine *e, vgx_tau_susceptibles_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: vgx_test_tau_prevalence over the table above (the flattening, bounds, tile walk, prefix-plus-own sum and scan of
 * vgx_get_tau_susceptibles compiled for the host).  start [P][G], values [T][P][G], final [P][G], outside [2]. */
typedef struct vgx_tau_susceptibles_chain {
    int64_t popNum, susNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t T; const double *grid;               /* [T] */
    int64_t G; const int32_t *class_of;          /* [susNum] */
    const int64_t *start;                        /* [P][G] */
    int64_t tile, n_own_events;
    int64_t *values;                             /* out [T][P][G] */
    int64_t *final;                              /* out [P][G] */
    int64_t *outside;                            /* out [2] */
} vgx_tau_susceptibles_chain;
int vgx_test_tau_susceptibles(vgx_tau_susceptibles_chain *io, char *errbuf, int64_t errcap);

/* ---- milestones: peaks, first passages and extinctions ------------------------------------------ */
/* What a grid cannot answer: how high a variant peaks and when, when it first reaches a number of hosts, whether and when it dies
 * out, per population and over all populations, exactly and on the device.
 * Cells.  Keys are 0 .. P-1 for the populations and P for all populations together; classes are 0 .. V-1 through
 * variant_of[hapNum] (values in [-1, V), -1 = not tracked), as vgx_get_prevalence takes it: cells = (P + 1) * V.  A log record
 * changes the population cells exactly as vgx_get_prevalence's table says, and every change to cell (p, c) is also made to
 * (P, c): a migration adds one host to (newPopulation, c) and to (P, c), a mutation between two classes changes both classes in
 * row P too.
 * Values.  x[-1] is the start: the state the call started from, or the initial state for a replicate that restarted, folded
 * through variant_of; row P of the start is the sum over the populations.  x[i] is the value after event i, for i in [0, n_ev).
 * Every step is +1, 0 or -1 per cell.  Values are signed int32 and are compared as such.
 * Results per (replicate, key, class), with event indices as int32:
 *   final          = x[n_ev - 1]; for an empty chain it is x[-1]
 *   peak           = the maximum of x[i] over i in [-1, n_ev); peak_event is the smallest i that attains it, -1 means the start
 *   first_event[k] = for each of the K thresholds theta_k (int32, any sign, 0 <= K <= 16) the smallest i >= -1 with
 *                    x[i] >= theta_k; VGX_MS_NEVER = INT32_MAX if there is none
 *   last_positive  = the largest i in [-1, n_ev) with x[i] > 0; -2 if there is none
 * Times are doubles, formed on the host from the replicate's clock: index i >= 0 becomes the time of event i, the same double
 * vgx_get_events gives; index -1 becomes the time the chain starts from; VGX_MS_NEVER and -2 become NaN.  The chains this call
 * accepts hold no event before the last call's log, and their clock starts where the call started: at the model's time when the
 * ensemble's first call began (0.0 for a model that had not run) for a first attempt, at 0.0 for a replicate that restarted,
 * which is what the host clock opens its run with; index -1 gets that value.  extinction_time is the time of event
 * last_positive + 1, the record that emptied the cell for good, where last_positive >= -1 and final == 0, NaN elsewhere (a chain
 * that stops at its iteration cap with hosts left is not extinct).
 * The device passes.  Pass A forms the net change of every (tile, population, class) with vgx_get_prevalence's counting kernel
 * over the tile edges as bounds, bound[j] = min(j * tile, n_ev), and its scan turns them into running sums: the values at every
 * tile's first event, the base of that tile (m * tiles * popNum * V * 4 bytes per chunk, counted in the chunk's share of device
 * memory).  Pass B, the ordered walk: one wavefront takes a (replicate, tile); its LDS holds one record per cell (the current
 * value, the peak and its event, the last positive event, K first events: 4 (4 + K) bytes per cell); the population rows start
 * from the tile's base, row P from their sum; it walks its events in log order, 64 consecutive events per round, one per lane.
 * Within a round, for one cell, pos is the ballot of the lanes that add to it and neg of those that take from it, and the value
 * after lane l's event is cur + popcount(pos & le(l)) - popcount(neg & le(l)).  A loop over the distinct cells of the round (a
 * wave has no match instruction) forms the two ballots of every cell and hands the j-th cell to lane j; every lane then settles
 * its cell from the masks alone: the first lane at or above theta_k, the last lane above zero and the maximum with its first
 * lane, all cells of the round at once.  When its tile ends the workgroup merges its records into the replicate's block with integer atomics: the peak as a
 * 64-bit atomicMax of the value biased to unsigned in the high word and 0xFFFFFFFF - (event + 1) in the low word, first events
 * with atomicMin, the last positive event with atomicMax.  The host initialises the block from the start state first (peak =
 * x[-1] at event -1, thresholds already met at -1, last_positive = -1 where the start is positive), so a chain of zero events
 * gets its answer without a walk.  final of a population row is the last running sum, row P their sum.  No result depends on the
 * tile size (VGX_MILESTONES_TILE_EVENTS, default 4096), the launch geometry, the chunking (VGX_TIMELINES_CHUNK_BYTES) or the
 * order in which workgroups finish.  The log is never copied; the host clock runs as in vgx_get_prevalence.
 * Any output pointer may be NULL (not written).  passes counts the launches of the walk; ms: kernels, host clock, whole call.
 * Preconditions as vgx_get_prevalence.  Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_milestones: "): those; replicates
 * out of range or given twice; V < 1 or a variant_of value outside [-1, V); K outside [0, 16]; a population size of 2^31 or more;
 * (popNum + 1) * V * 4 * (4 + K) bytes of records above the 65536 bytes of LDS a walking workgroup may use (the message names
 * popNum, V, K and the bytes); a replicate whose tile bases alone do not fit in the call's share of device memory; a chain of
 * 2^30 events or more.  vgx_clock_mismatches counts every selected replicate once. */
#define VGX_MS_NEVER 2147483647
typedef struct vgx_milestones_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int64_t K; const int32_t *thresholds;        /* [K], 0 <= K <= 16 */
    int32_t *final;                              /* NULL or host [n][P+1][V] */
    int32_t *peak;                               /* NULL or host [n][P+1][V] */
    int32_t *peak_event;                         /* NULL or host [n][P+1][V] */
    int32_t *last_positive_event;                /* NULL or host [n][P+1][V] */
    int32_t *first_event;                        /* NULL or host [n][K][P+1][V] */
    double *peak_time;                           /* NULL or host [n][P+1][V] */
    double *extinction_time;                     /* NULL or host [n][P+1][V] */
    double *first_time;                          /* NULL or host [n][K][P+1][V] */
    int64_t passes; double ms[3];                /* out: launches of the walk; kernels, host clock, whole call */
} vgx_milestones_io;
int vgx_get_milestones(vgx_engine *e, vgx_milestones_io *io);
/* Test hook: the rule, pass A, the walk in rounds of 64 emulated lanes with the same mask arithmetic and the merge of
 * vgx_get_milestones compiled for the host, on one chain given as arrays (no device, no engine), tile after tile with `tile`
 * events each (0: the default).  start [P][V]: whole numbers in [0, 2^31), their sums too.  t_start: the time of index -1.  The
 * outputs ([P+1][V], first_* [K][P+1][V]) are overwritten.  The same limits: the LDS budget, K, a chain of 2^30 events, a bad V or
 * variant_of are refused with the message in errbuf. */
int vgx_test_milestones(const double *times, const int64_t *types, const int64_t *haplotypes, const int64_t *populations,
                        const int64_t *newHaplotypes, const int64_t *newPopulations, int64_t n_ev, int64_t P, int64_t hapNum,
                        const int32_t *variant_of, int64_t V, const int64_t *start, const int32_t *thresholds, int64_t K, int64_t tile,
                        double t_start, int32_t *final, int32_t *peak, int32_t *peak_event, int32_t *last_positive_event,
                        int32_t *first_event, double *peak_time, double *extinction_time, double *first_time, char *errbuf,
                        int64_t errcap);

/* ---- milestones of tau replicates ---------------------------------------------------------------- */
/* vgx_get_milestones for the replicates of the last vgx_simulate_tau call that recorded its multievent rows.
 * Chain and events.  The chain is vgx_get_tau_prevalence's: a replicate that did not restart and whose model held events carries
 * the prefix (vgx_timelines_prefix, flattened: a direct event is one row with num = 1), its own steps follow; a restarted
 * replicate has its own steps only.  An EVENT is a direct event of the prefix or one step.  Events are numbered from 0 along the
 * chain: own step k of a replicate with a prefix of pre_ev events is event pre_ev + k.  An event's time is the time of its log
 * record, prefix->ev_times[i] or the step's.
 * Cells.  vgx_get_milestones's: keys 0 .. P-1 and key P for all populations together, classes through variant_of, (P + 1) * V
 * cells.  A row changes the population cells exactly as vgx_get_tau_prevalence says (sign * num, VGX_TL_ROW_DIRECT masked off, a
 * field that is not a 32-bit index matches nothing, num <= 0 changes nothing), and every change to (p, c) is also made to (P, c).
 * Values.  x[-1] is start_r of vgx_get_tau_prevalence (the initial state for a replicate that restarted or a prefix that is not
 * empty, else the state the call started from), row P the sum over the populations.  x[i] is the value after ALL rows of event
 * i; the state inside a step is not a value: a step whose rows add 5 to a cell and take 5 from it leaves x unchanged, meets no
 * threshold and moves no peak, and a cell at 1 that gets -1 and +1 in one step has not gone extinct.  Values are int64, compared
 * signed; sums wrap as unsigned 64-bit integers do.
 * Results per (replicate, key, class), defined as in vgx_get_milestones over this x: final and peak int64; peak_event (int32) the
 * smallest i >= -1 that attains the peak; first_event[k] (int32) for each of the K thresholds theta_k (int64, any sign,
 * 0 <= K <= 16) the smallest i >= -1 with x[i] >= theta_k, else VGX_MS_NEVER; last_positive_event (int32) the largest i with
 * x[i] > 0, -2 if there is none.  Times are doubles: index i >= 0 gives event i's time; index -1 gives 0.0 for a chain that starts
 * at the beginning of the model's history (a restart, or a prefix that is not empty), else the time the call's first step started
 * from; VGX_MS_NEVER and -2 give NaN.  extinction_time is the time of event last_positive + 1 where last_positive >= -1 and
 * final == 0, NaN elsewhere.  No host clock runs: step times are host doubles already.
 * The device passes.  Tiles are runs of whole events: the host cuts every chain so that a tile holds about
 * VGX_TAU_MILESTONES_TILE_ROWS rows (default 4096) and at most as many events; a tile never splits an event, a step with more
 * rows is a tile of its own.  Pass A: vgx_get_tau_prevalence's int64 counting and scan kernels with the tile edges in row space
 * as bounds give every tile its base, the values at its first event.  Pass B, the walk: one workgroup takes a (chain, tile); LDS
 * holds one record per cell (value, the event's net change, peak: int64; the peak's event, the last positive event, K first
 * events, a touched-list entry and its mark: int32; (P + 1) * V * (40 + 4 K) + 16 bytes).  The events of the tile run in order;
 * for each, the threads stride over its rows and add the signed num to the net change of its cells with LDS atomics, noting a
 * cell the first time it is hit; behind a barrier they stride over the touched population cells, settle each (new value, peak,
 * first events, last positive event; a cell taken from above zero to zero or below offers the event before) and pass its net
 * change on to row P, whose touched cells are settled behind another barrier.  Events without rows are not visited.  At the
 * tile's end event indices are merged into the chain's block with 32-bit atomicMin / atomicMax; the tile's peak and its event go
 * to a slot [chain][tile][cell], and a small kernel reduces the slots in tile order, a strictly greater value winning, so among
 * equals the earliest event stays.  The prefix is walked ONCE per call as a chain of its own from the initial state; its block
 * and its final values are what every replicate that carries it starts from.  The host initialises the other blocks from the
 * start (peak = x[-1] at event -1, thresholds met at -1, last_positive = -1 where the start is positive) and gives a cell that
 * ends positive last_positive = events - 1.  Every result is an extremum over candidates that hold whatever tile offers them: no
 * result depends on the tile size, the workgroup shape (VGX_TAU_MILESTONES_WAVES), the chunking (VGX_TIMELINES_CHUNK_BYTES: the
 * event tables, tile bases and peak slots of a chunk of replicates fit the share) or the order in which workgroups finish.
 * Any output pointer may be NULL (not written).  passes counts the launches of the walk, the prefix's as one; ms: kernels, the
 * host's tile and row tables, whole call.
 * Refusals (VGX_ERR_ARG, worded alike behind "vgx_get_tau_milestones: "): the last call was not vgx_simulate_tau; it recorded no
 * rows; a replicate that did not restart continues a log of another length than prefix->ev_ptr; prefix plus own rows reach 2^31;
 * a null prefix column; replicates out of range or given twice; V < 1 or a variant_of value outside [-1, V); K outside [0, 16];
 * a chain of 2^30 events or more; records above the 65536 bytes of LDS a walking workgroup may use (the message names popNum, V,
 * K and the bytes); a replicate whose tile bases and peak slots alone do not fit the call's share of device memory. */
typedef struct vgx_tau_milestones_io {
    int64_t n; const int64_t *replicates;        /* selected replicates, distinct */
    int64_t V; const int32_t *variant_of;        /* [hapNum], values in [-1, V) */
    int64_t K; const int64_t *thresholds;        /* [K], 0 <= K <= 16 */
    int64_t *final;                              /* NULL or host [n][P+1][V] */
    int64_t *peak;                               /* NULL or host [n][P+1][V] */
    int32_t *peak_event;                         /* NULL or host [n][P+1][V] */
    int32_t *last_positive_event;                /* NULL or host [n][P+1][V] */
    int32_t *first_event;                        /* NULL or host [n][K][P+1][V] */
    double *peak_time;                           /* NULL or host [n][P+1][V] */
    double *extinction_time;                     /* NULL or host [n][P+1][V] */
    double *first_time;                          /* NULL or host [n][K][P+1][V] */
    int64_t passes; double ms[3];                /* out: launches of the walk; kernels, host tile and row tables, whole call */
} vgx_tau_milestones_io;
int vgx_get_tau_milestones(vgx_engine *e, vgx_tau_milestones_io *io, const vgx_timelines_prefix *prefix);
/* Test hook: the flattening, tile edges, pass A, the walk (the same settle, event by event over the touched cells), the merge in
 * tile order and the outputs of vgx_get_tau_milestones compiled for the host, on one chain given as event columns and multievent
 * columns as vgx_tau_prevalence_chain gives them (no device, no engine), tile after tile of about `tile` rows (0: the default).
 * The last n_own_events events play the replicate's own steps (-1: the chain's trailing MULTITYPE events), everything before
 * them the prefix, which is walked once as a chain of its own; the own events start from its block and its final values, as on
 * the device.  start [P][V]: x[-1] of the population rows.  t_start: the time of index -1.  The outputs ([P+1][V], first_*
 * [K][P+1][V]) are overwritten.  Refused with the message in errbuf: K outside [0, 16], the LDS budget, a chain of 2^30 events, a
 * bad V or variant_of, a MULTITYPE row range outside the multievent log, a prefix row out of range. */
typedef struct vgx_tau_milestones_chain {
    int64_t popNum, hapNum;
    int64_t ev_ptr;
    const double *ev_times;
    const int64_t *ev_types, *ev_haplotypes, *ev_populations, *ev_newHaplotypes, *ev_newPopulations;
    int64_t mev_rows;
    const int64_t *mev_num, *mev_types, *mev_haplotypes, *mev_populations, *mev_newHaplotypes, *mev_newPopulations;
    int64_t V; const int32_t *variant_of;        /* [hapNum] */
    const int64_t *start;                        /* [P][V] */
    int64_t K; const int64_t *thresholds;        /* [K] */
    int64_t tile, n_own_events;
    double t_start;
    int64_t *final, *peak;                       /* out [P+1][V] */
    int32_t *peak_event, *last_positive_event;   /* out [P+1][V] */
    int32_t *first_event;                        /* out [K][P+1][V] */
    double *peak_time, *extinction_time;         /* out [P+1][V] */
    double *first_time;                          /* out [K][P+1][V] */
} vgx_tau_milestones_chain;
int vgx_test_tau_milestones(vgx_tau_milestones_chain *io, char *errbuf, int64_t errcap);

/* ---- kernel choice of the direct path ------------------------------------------------------- */
/* What the choice of a direct call's kernel reads: the model's dimensions, the state the call starts from and two diagnostic
 * switches.  vgx_simulate_direct fills one from the engine; the choice itself is a pure function of it and of the options. */
typedef struct vgx_direct_shape {
    int64_t P, H, S, sites;          /* popNum, hapNum, susNum, sites */
    int64_t R;                       /* replicates */
    int64_t C, CB;                   /* rate classes; birth classes (transmission rate x susceptibility row) */
    int64_t cap;                     /* entries an occupancy list can hold */
    int64_t n_seg, n_solo_seg;       /* chain segments of the BirthRate program; (group, non-zero susceptibility) pairs */
    int64_t solo_npass0, solo_npass1;   /* passes of the single-trajectory kernel without / with the migration sum (< 0: too many) */
    int64_t solo_ncls, solo_maxnnz;  /* susceptibility classes; most non-zero groups of one class */
    int64_t start_lone_rows;         /* heap rows of vgx_lone.hip the start state needs */
    int64_t start_max_nocc;          /* longest occupancy list of the start state */
    int64_t max_size;                /* largest population size */
    int64_t hosts_below_2p53;        /* the population sizes, summed as doubles, stay below 2^53 */
    int64_t ld_possible;             /* some population can switch its lockdown state */
    int64_t recomb;                  /* recombination probability != 0 */
    int64_t fresh_state;             /* the call starts from the state of vgx_set_state (it does not continue the device's) */
    int64_t suscep_cumul0_zero;      /* no immunity loss from group 0: suscepCumulTransition[0] == 0 */
    int64_t have_counts32;           /* the device state keeps the 4-byte copy of the counts */
    int64_t tot_sus_is_sus;          /* one group, and totalSusceptible == susceptible in every population */
    int64_t no_lone, solo_general;   /* diagnostics: VGX_NO_LONE, VGX_SOLO_GENERAL are set */
    int64_t param_sets;              /* parameter sets installed (vgx_set_param_sets); 0 or 1: one shared copy.  More: kernel 1 for
                                        opts.kernel 0 or 1 in mode 0, everything else refused; C and CB are the largest over the sets */
} vgx_direct_shape;
/* What the rest of the call needs from the choice.  The fields of a kernel that was not chosen are 0. */
typedef struct vgx_direct_plan {
    int64_t kernel;                  /* a value of vgx_run_opts.kernel, 1 .. 6, or 7: the FAST row kernel (vgx_quadf.hip) */
    int64_t mode;                    /* the mode the call runs in: 0 where an exact kernel serves a FAST request */
    int64_t fast, philox;            /* order-free arithmetic; counter-based stream */
    int64_t solo_mig_in_lds;         /* 5: migrationRates fit the LDS budget */
    int64_t solo_compact;            /* 5: 0 general layout, 1 / 2 compact layout with one / two registers of terms */
    int64_t lone_general;            /* 6: its general form */
    int64_t lone_lds_bytes;          /* 6: dynamic LDS of the launch */
    int64_t long_lists;              /* 3: the exact row kernel's form for lists beyond one tile */
    int64_t leaves32;                /* the kernel leaves only the 4-byte counts current */
    int64_t fallback_kernel, fallback_mode;   /* 6 as the automatic choice: the request the call repeats when the LDS heap fills up */
} vgx_direct_plan;
/* Test hook: the choice for a shape and options given as numbers: no device, no engine.  Returns the code vgx_simulate_direct would
 * return for a refused request, with that call's vgx_last_error text in errbuf. */
int vgx_test_direct_plan(const vgx_direct_shape *shape, const vgx_run_opts *opts, vgx_direct_plan *plan, char *errbuf, int64_t errcap);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Device time of the last simulate call's kernels, from HIP events on the engine's stream (ms). */
double vgx_last_kernel_ms(const vgx_engine *e);
/* The kernel the last vgx_simulate_direct call ran on, as a value of vgx_run_opts.kernel (1 .. 6; 3 also for the FAST row kernel). */
int vgx_last_direct_kernel(const vgx_engine *e);
/* Number of kernel launches timed by the last simulate call. */
int64_t vgx_last_kernel_launches(const vgx_engine *e);
/* Bytes of device memory held by the engine. */
int64_t vgx_device_bytes(const vgx_engine *e);
/* Diagnostic build only (libvgx built with -DVGX_PROFILE): 16 per-phase shader-cycle sums of the last direct
 * call for one replicate (phase list: tools/profile_phases.py); all zeros in the product build. */
int vgx_get_profile(vgx_engine *e, int64_t replicate, int64_t *out16);
/* Diagnostics / tests: the first `count` entries of the 4-byte count copy of one occupancy list as the last call of the
 * four-replicates-per-wavefront kernel left it (list order = haplotype order), and the capacity of every list in *list_cap
 * (0 without device state).  count = 0 asks for the capacity alone; VGX_ERR_ARG when that copy is not current. */
int vgx_get_list_counts_quad(vgx_engine *e, int64_t replicate, int64_t population, int64_t count, int32_t *out, int64_t *list_cap);
/* Diagnostics / tests: the first `count` tile sums of one occupancy list as the last direct call left them: the sum of the counts of
 * every 64-entry tile of a list longer than one tile, 0 behind the list (what the kernels choose a migrant's haplotype by), and the
 * number of tile sums every list has room for in *tile_cap (0 without device state).  count = 0 asks for that number alone. */
int vgx_get_list_tile_sums(vgx_engine *e, int64_t replicate, int64_t population, int64_t count, int64_t *out, int64_t *tile_cap);

/* ---- the dense propensity row pass (K3) ------------------------------------------------------- */
/* For callers that hold the reference's dense per-population arrays: the infect branch of UpdateRates (pyx:518-528:
 * BirthRate, tEventHapPopRate, hapPopRate, infectPopRate) followed by fastChoose over hapPopRate (fast_choose.pxi:18-31)
 * for `rows` independent (replicate, population) rows at once.  FAST-mode arithmetic: BirthRate factored
 * through rowContact = sum_pn m[pi,pn]^2 * cd[pn] / actualSizes[pn], tree-order sums.  All pointers are host arrays.
 * The chosen entry always has a positive hapPopRate: u = 0 gives the row's first positive entry (rnOut 0), an r that rounding
 * leaves above every running sum its last positive one.  A row whose rowTotal is 0 has nothing to choose: chosen is H - 1 and
 * rnOut is NaN there, and neither may be used.  rows, H or S below 1: VGX_ERR_ARG, the message names the three. */
typedef struct vgx_rowscan {
    int64_t rows, H, S;
    const int64_t *infectious;       /* [rows][H]      infectious[pi, :]                                   in  */
    const double *eventRates123;     /* [rows][H][3]   eventHapPopRate[pi, :, 1:4] (pyx:311-314)          in  */
    const int64_t *numToHap;         /* [H]            pyx:105-125 (identity without memory_optimization)  in  */
    const double *bRate;             /* [H]                                                                in  */
    const double *susceptibility;    /* [H][S]                                                             in  */
    const double *rowSusceptible;    /* [rows][S]      susceptible[pi, :] as doubles                       in  */
    const double *rowContact;        /* [rows]                                                             in  */
    const double *u;                 /* [rows]         the random number of fastChoose                     in  */
    double *birthRate, *tEvent, *hapPopRate;   /* [rows][H]  eventHapPopRate[pi,:,0], tEventHapPopRate, hapPopRate  out */
    double *susceptHapPopRate;       /* [rows][H][S]                                                       out */
    double *rowTotal;                /* [rows]         infectPopRate[pi]                                   out */
    int64_t *chosen;                 /* [rows]         index returned by fastChoose                        out */
    double *rnOut;                   /* [rows]         rescaled random number (fc:31)                      out */
} vgx_rowscan;
int vgx_propensity_scan(const vgx_rowscan *io);
/* Measurement: `rows` copies of the caller's first row resident in HBM, `repeats` timed passes after a warm-up; average
 * device time (HIP events) of the row update and of the choice; the first row's outputs are returned. */
int vgx_propensity_scan_bench(const vgx_rowscan *first_row, int64_t rows, int repeats, double *ms_update, double *ms_choose);
const char *vgx_propensity_scan_error(void);

/* ---- test hooks: the samplers of the tau-leap kernels on their own -------------------------------- */
/* Philox4x32-10 (Salmon et al. 2011) for one (counter, key): the host build of the same function, or the device's. */
int vgx_test_philox(int on_device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* n independent draws of the device's Poisson(lam) sampler (what replaces numpy's random_poisson, pyx:2531-2532:
 * inversion below a mean of 10, PTRS from 10 on), draw i from the Philox stream of compartment i under `seed`. */
int vgx_test_poisson(double lam, int64_t n, uint64_t seed, int64_t *out);

/* count quotients n[i] / b[i] formed on the device three ways: q_seq = through the correctly rounded reciprocal of b with two residual
 * corrections (how the single-trajectory kernel divides BirthRate's terms by actualSizes, pyx:390), q_lean = its division sequence
 * without range scaling and special-case fix-up (fastChoose's rescalings, fast_choose.pxi:31), q_div = the division. */
int vgx_test_div_by_const(const double *n, const double *b, int64_t count, double *q_seq, double *q_lean, double *q_div);

/* the serial prefix chains of the row kernels on `rows` rows of 64 weights w[row][0..63] (finite, >= +0.0) from carry[row], formed on
 * the device: pre16[row][l] = carry + w[0] + ... + w[l] for l < 16 and tot16[row][l] = pre16[row][15] in every lane (row_scan16),
 * pre64[row][k] = carry + w[0] + ... + w[k] for k < 64 (row_scan64), every sum left to right. */
int vgx_test_row_scans(const double *w, const double *carry, int64_t rows, double *pre16, double *tot16, double *pre64);

/* the haplotype choice of the four-replicates-per-wavefront kernel over lists longer than one 64-entry tile, on its own: `rows` lists
 * (counts[row][0 .. n[row]-1] >= 0 and haps[row][..] ascending, rows of `maxlen` entries), one per 16-lane row and four to a wavefront.
 * Each row's rate refresh sums tE[row] * count left to right and keeps the running sum at the end of every tile; the choice for
 * r[row] then runs twice, [0][row] from those kept sums and [1][row] streaming the tiles again: the list index chosen (the first k
 * whose prefix sum is not below r; none: n - 1 if that entry is haplotype H - 1, else -1), the prefix sum at that index (none: the
 * list's total), its weight tE * count and its count.  All outputs are [2][rows]. */
int vgx_test_quad_tile_choice(const int32_t *counts, const int32_t *haps, const int32_t *n, const double *tE, const double *r, int64_t rows,
                              int64_t maxlen, int H, int32_t *k_hit, double *pre_hit, double *w_hit, int64_t *cnt_hit);

#ifdef __cplusplus
}
#endif
#endif /* VGX_H */
