// vgx_mutation_spectrum.h — the mutation records of one sampled tree reduced to their clade sizes: a log2-binned site-frequency
// spectrum, the substitution counts and the sums the scalar estimators (pi, Watterson's theta, theta_H, Tajima's D, Fay and Wu's H)
// are made of, written once for the host and the device.  vgx_mutation_spectrum.hip runs it over the trees and records the walks of
// vgx_gwalk.h / vgx_gwalk_tau.h left on the device (vgx_get_mutation_spectrum, vgx_get_tau_mutation_spectrum) and over hand-made
// trees (vgx_test_mutation_spectrum_device); the host hook vgx_test_mutation_spectrum (vgx_genealogy.cpp) runs the sequential sweep
// below, which is the definition.  DESIGN.md §31.
//
// Input, one tree of N nodes under the precondition of vgx_tree_shape.h (N odd and >= 3, tree[N - 1] == -1, i < tree[i] < N
// otherwise, every node 0 or 2 children), M records (mut_node, mut_AS, mut_DS, mut_site) and the model's sites S, 0 <= S <= 15
// (a model without sites, hapNum = 1: no record can be accepted and the three per-site blocks are empty; stats still holds tips).
// No node time and no event index is read.
//
//   clade[i]   tips below node i: 1 for a tip, else the sum over its children;  tips = clade[N - 1]
//   c_k        = clade[mut_node[k]]: record k sits on the branch above mut_node[k].  A record on the root (mut_node == N - 1: the walk
//              runs on to event 0 after the last coalescence) has c = tips; it is counted like any other and also in `fixed`.
//              Several records on one node are several records.
// The reading: the model has finitely many sites and recurrent mutation; every record is ONE mutation event and c is the clade below
// it, whether or not a later event at the same site lies inside that clade: the infinite-sites reading of the events.
//
// Outputs, all int64, the sums wrapping (vgx_ts_wrap_add):
//   spectrum[S][32]          records of site s with floor(log2 c) == b: bin 0 = the singletons; bin 31 stays 0 (c is an int32)
//   substitutions[S][4][4]   records by (site, AS, DS)
//   sums[S][3]               per site: sum c, sum c^2, sum c (tips - c).  Each term is below tips^2 <= 2^60 (tips <= 2^30), so a sum
//                            is below M tips^2: sum c^2 can wrap only beyond 2^63 / tips^2 records, 8 * 10^6 records of clade size
//                            tips at 10^6 tips (2^23 at 2^20); with M < 2^30 it cannot wrap below 92681 tips (tips^2 < 2^33).
//   stats[4]                 tips, mutations (M), fixed (records with c == tips), max_clade (max c; 0 without records)
// A record with mut_node outside [0, N), mut_site outside [0, S) or mut_AS / mut_DS outside 0 .. 3 is rejected: the tree gets status
// VGX_GW_BAD_RECORD with arg = the lowest such record index, and an all-zero row.  No healthy walk leaves such a record.  A tree that
// breaks the structure gets VGX_GW_BAD_TREE (13) with the first offending node, as vgx_tree_shape.h defines it; the tree is judged
// before the records.
#pragma once
#include <stdint.h>
#include "vgx_tree_shape.h"   // VGX_HD, vgx_ts_wrap_add, vgx_ts_check_parents, VGX_GW_BAD_TREE

#define VGX_MSP_BINS 32          // log2 bins of a clade size
#define VGX_MSP_SUMS 3           // clade_sum, clade_sumsq, pair_sum
#define VGX_MSP_STATS 4          // tips, mutations, fixed, max_clade
#define VGX_MSP_SITES_MAX 15     // include/vgx.h: sites <= 15
#define VGX_MSP_NODE_BYTES 16    // workspace of one node: kids, got, n, clade (int32)
enum { VGX_MSP_CLADE_SUM = 0, VGX_MSP_CLADE_SUMSQ = 1, VGX_MSP_PAIR_SUM = 2 };
enum { VGX_MSP_TIPS = 0, VGX_MSP_MUTATIONS = 1, VGX_MSP_FIXED = 2, VGX_MSP_MAX_CLADE = 3 };

// status of a replicate with a record outside the tree or the model (arg = the lowest offending record index): appended to the walk
// statuses 0 .. 12 and VGX_GW_BAD_TREE
enum { VGX_GW_BAD_RECORD = 14 };

// per-node workspace of one tree (pointers private to it); clade[] is also a result
struct VgxMspWork {
    int32_t *kids, *got, *n, *clade;
};

// whether record (node, AS, DS, site) may be used with a tree of N nodes and S sites: checked before anything indexes by it
VGX_HD bool vgx_msp_record_ok(int32_t node, int32_t AS, int32_t DS, int32_t site, int64_t N, int64_t S) {
    return node >= 0 && node < N && site >= 0 && site < S && AS >= 0 && AS <= 3 && DS >= 0 && DS <= 3;
}

// floor(log2 c) for c >= 1
VGX_HD int vgx_msp_bin(int32_t c) {
    int b = 0;
    for (uint32_t v = (uint32_t)c; v > 1; v >>= 1) b++;
    return b;
}

// The sequential sweep over one tree whose parents satisfy i < tree[i] < N (tree[N - 1] == -1) and whose S lies in 0 .. 15: the caller
// has checked both, so no access leaves the arrays.  Returns 0 and the four blocks, or VGX_GW_BAD_TREE / VGX_GW_BAD_RECORD with *arg
// the first offending node / the lowest offending record; the four blocks are then zeros.  `w` is overwritten; after a return other
// than VGX_GW_BAD_TREE w.clade[N] holds every node's clade size.
VGX_HD int vgx_ms_sweep(const int32_t *tree, int64_t N, const VgxMspWork &w, const int32_t *mut_node, const int32_t *mut_AS, const int32_t *mut_DS,
                        const int32_t *mut_site, int64_t M, int64_t S, int64_t *spectrum, int64_t *substitutions, int64_t *sums, int64_t *stats,
                        int64_t *arg) {
    for (int64_t k = 0; k < S * VGX_MSP_BINS; k++) spectrum[k] = 0;
    for (int64_t k = 0; k < S * 16; k++) substitutions[k] = 0;
    for (int64_t k = 0; k < S * VGX_MSP_SUMS; k++) sums[k] = 0;
    for (int k = 0; k < VGX_MSP_STATS; k++) stats[k] = 0;
    *arg = 0;
    for (int64_t i = 0; i < N; i++) { w.kids[i] = 0; w.got[i] = 0; w.n[i] = 0; w.clade[i] = 0; }
    for (int64_t i = 0; i < N - 1; i++) w.kids[tree[i]] += 1;
    for (int64_t i = 0; i < N; i++) {
        const int32_t kids = w.kids[i];
        if (kids != 0 && kids != 2) { *arg = i; return VGX_GW_BAD_TREE; }
        const int32_t c = kids == 0 ? 1 : w.n[i];
        w.clade[i] = c;
        if (i == N - 1) break;
        w.n[tree[i]] += c;
        w.got[tree[i]] += 1;
    }
    for (int64_t k = 0; k < M; k++)
        if (!vgx_msp_record_ok(mut_node[k], mut_AS[k], mut_DS[k], mut_site[k], N, S)) { *arg = k; return VGX_GW_BAD_RECORD; }
    const int64_t tips = w.clade[N - 1];
    int64_t fixed = 0, max_clade = 0;
    for (int64_t k = 0; k < M; k++) {
        const int64_t c = w.clade[mut_node[k]], s = mut_site[k];
        spectrum[s * VGX_MSP_BINS + vgx_msp_bin((int32_t)c)] += 1;
        substitutions[s * 16 + mut_AS[k] * 4 + mut_DS[k]] += 1;
        int64_t *q = sums + s * VGX_MSP_SUMS;
        q[VGX_MSP_CLADE_SUM] = vgx_ts_wrap_add(q[VGX_MSP_CLADE_SUM], c);
        q[VGX_MSP_CLADE_SUMSQ] = vgx_ts_wrap_add(q[VGX_MSP_CLADE_SUMSQ], c * c);
        q[VGX_MSP_PAIR_SUM] = vgx_ts_wrap_add(q[VGX_MSP_PAIR_SUM], c * (tips - c));
        fixed += c == tips;
        if (c > max_clade) max_clade = c;
    }
    stats[VGX_MSP_TIPS] = tips; stats[VGX_MSP_MUTATIONS] = M; stats[VGX_MSP_FIXED] = fixed; stats[VGX_MSP_MAX_CLADE] = max_clade;
    return 0;
}

// ---- device plumbing (vgx_api.hip, vgx_mutation_spectrum.hip) --------------------------------------------------------------------
// where a tree and its records lie in the pass's arrays.  With a walk result (VgxMspLaunch.res) the records are the walk's mut_n,
// bounded by `muts` (the capacity the walk was given); without one they are `muts`.
struct VgxMspDesc { int64_t node_off, nodes, mut_off, muts; };

struct VgxMspLaunch {
    int64_t n;                    // trees of this pass
    const VgxMspDesc *desc;        // [n]
    const int64_t *res;           // NULL, or [n][5] the walk's VgxGwResult: a tree whose walk status is not 0 is skipped
    const int32_t *tree;          // node array of the pass
    const int32_t *mut_node, *mut_AS, *mut_DS, *mut_site;   // record arrays of the pass
    int64_t S;                    // sites, 0 .. VGX_MSP_SITES_MAX
    VgxMspWork w;                  // workspace of the pass, indexed like the node array
    int64_t *spectrum;            // [n][S][32]
    int64_t *substitutions;       // [n][S][4][4]
    int64_t *sums;                // [n][S][3]
    int64_t *stats;               // [n][4]
    int64_t *status;              // [n][2] status and its argument: the walk's, VGX_GW_BAD_TREE and the node, VGX_GW_BAD_RECORD and the record
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_ms_spectrum(const VgxMspLaunch *a, hipStream_t s);
#pragma GCC visibility pop
#endif
