// vgx_tau_lineages.h — ancestral lineages per (population, variant class) of a TAU chain at grid times the caller gives
// (vgx_get_tau_lineages, vgx_test_tau_lineages): the tau walk of vgx_gwalk_tau.h with the logging observer of
// vgx_lineages.h, whose record rule, tile walk, binning and suffix sum it takes as they are.  A record's `ev` is the chain's EVENT
// index as the walk numbers it: prefix events 0 .. n_pre - 1, the replicate's own step k is n_pre + k, so all records of a step
// carry the same ev and a replicate's records still lie in descending ev order.  The bounds are VgxPrevCutter's over
// (event index, event time): the prefix's event times, then the replicate's own step times.
#pragma once
#include <stdint.h>
#include "vgx_gwalk_tau.h"
#include "vgx_lineages.h"

// ---- device plumbing (host side <-> walk kernel of vgx_tau_lineages.hip) ------------------------------------------------------
// one selected replicate of a walk launch: offsets into the pass's workspace (elements; rec_off in records)
struct VgxTauLnDesc {
    int64_t rep, n_pre, n_steps, sCounter, tsize, tab_off, arena_off, arena_cap, node_off, rec_off, rec_cap;
    int64_t row_off, off_off;     // as in its VgxGtCanonDesc
    int64_t status, arg;          // what the canonicalise kernel reported (a replicate that failed there is not walked)
    uint64_t rng[4];
    int64_t has32, spare;
};
struct VgxTauLnLaunch {
    int64_t n;
    const VgxTauLnDesc *desc;
    const VgxGtRow *pre;          // the flattened prefix, shared by the replicates that did not restart
    const int32_t *pre_off;
    const VgxGtRow *can;
    const int32_t *can_off;
    const int32_t *I;             // t_I: [R][P][H] final infectious counts
    int64_t P, H;
    int64_t *key, *cnt;
    int32_t *base, *len, *lcap, *arena;
    int32_t *fresh, *tree;        // [node_off ...]: the arrivals of a row, the parents
    int32_t *rec;                 // lineage logs of the pass, [sum of rec_cap][6]
    int64_t *res;                 // [n][5] VgxGwResult
    uint64_t *rng_out;            // [n][6] generator state after the walk: PCG64 words, has32, spare
    int64_t *n_rec;               // [n] records the binning reads: those written, 0 for a walk that failed
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_tau_ln_walk(const VgxTauLnLaunch *a, hipStream_t s);
// vgx_tau_genealogies.hip: the canonicalise launch and the counting launch (out[3 i ..]: sums of min(num, sCounter) over replicate
// i's raw MUTATION rows, MIGRATION rows, rows that can push a lineage)
extern "C" hipError_t vgxi_tg_canon(const VgxGtCanonLaunch *a, hipStream_t s);
// (and its walk launch, for vgx_tau_tree_shapes.hip)
extern "C" hipError_t vgxi_tg_walk(const VgxGtLaunch *a, hipStream_t s);
extern "C" hipError_t vgxi_tg_count(const int64_t *mev, int64_t mev_cap, const int64_t *reps, const int64_t *n_rows, const int64_t *sC, int64_t n,
                                    int64_t *out, hipStream_t s);
#pragma GCC visibility pop
#endif
