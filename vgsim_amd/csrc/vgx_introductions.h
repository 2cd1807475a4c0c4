// vgx_introductions.h — the population labels of one sampled tree reduced to its transmission lineages: the introductions every
// population received, by source and destination, and the sizes of the lineages they seeded, written once for the host and the
// device.  vgx_introductions.hip runs it over the trees and labels the walks of vgx_gwalk.h / vgx_gwalk_tau.h left on the device
// (vgx_get_introductions, vgx_get_tau_introductions) and over hand-made trees (vgx_test_introductions_device); the host hook
// vgx_test_introductions (vgx_genealogy.cpp) runs the sequential sweep below, which is the definition.  DESIGN.md §32.
//
// Input, one tree of N nodes under the precondition of vgx_tree_shape.h (N odd and >= 3, tree[N - 1] == -1, i < tree[i] < N
// otherwise, every node 0 or 2 children), pop[N] the walk's tree_pop, and the model's populations P >= 1.  No node time, no event
// index and none of the walk's migration records is read.
//
//   crossing(i)   for i < N - 1: pop[tree[i]] != pop[i].  The branch above i is then ONE NET introduction from src = pop[tree[i]]
//                 into dst = pop[i] (the direction of the walk's closing pass).  Net: moves along the branch that left no node are
//                 invisible, so a branch that went 0 -> 2 -> 1 counts as 0 -> 1 and one that went 0 -> 1 -> 0 does not count.
//   clade[i]      tips below node i: 1 for a tip, else the sum over its children;  tips = clade[N - 1]
//   local[i]      tips below i reached without passing a crossing branch: 1 for a tip, else the sum of local[j] over the children
//                 j with !crossing(j).  May be 0 (both children crossed).
//   head          node i heads a transmission lineage if it is the root or crossing(i): its size is local[i], its population
//                 pop[i].  Every tip lies in exactly one lineage.
//
// Outputs, all int64, the sums wrapping (vgx_ts_wrap_add):
//   tips_by_pop[P]    tips by pop
//   imports[P][P]     crossing branches by (src, dst); the diagonal is 0
//   into[P][6]        per dst over its introductions: count, sum clade, sum local, sum local^2, empty (local == 0), max local.
//                     Each local^2 is below tips^2 <= 2^60 (tips <= 2^30) and a tree has fewer than 2 tips introductions, so
//                     sum local^2 <= (sum local)^2 <= tips^2 cannot wrap; sum clade is below 2 tips^2 <= 2^61: nothing wraps
//                     on a tree the walk can make, the wrapping add only fixes what a sum beyond that would give.
//   spectrum[P][32]   introductions into dst with floor(log2 local) == b, local >= 1: bin 0 = the singletons; the empty ones are
//                     counted in into alone; bin 31 stays 0 (local is an int32)
//   stats[8]          tips, introductions, root_pop, root_local, max_local (the root's lineage included), max_clade (over the
//                     introductions; 0 without one), empty, populations with at least one tip
// A tree that breaks the structure gets VGX_GW_BAD_TREE (13) with the first offending node, as vgx_tree_shape.h defines it; the
// tree is judged before the labels.  A pop[i] outside [0, P) gives VGX_GW_BAD_LABEL with arg = the lowest such node; the blocks
// are then zeros.  No healthy walk leaves such a label.
#pragma once
#include <stdint.h>
#include "vgx_mutation_spectrum.h"   // VGX_GW_BAD_RECORD (the status before ours); vgx_tree_shape.h: VGX_HD, vgx_ts_wrap_add, vgx_ts_check_parents

#define VGX_IN_BINS 32          // log2 bins of a lineage size
#define VGX_IN_INTO 6           // count, clade_sum, local_sum, local_sumsq, empty, max_local
#define VGX_IN_STATS 8          // tips, introductions, root_pop, root_local, max_local, max_clade, empty, pops_with_tips
#define VGX_IN_NODE_BYTES 16    // workspace of one node: kids, got, n, ln (int32)
#define VGX_IN_POPS_MAX 1024    // a row holds P^2 + 39 P + 8 cells of 8 bytes: 8.7 MB at 1024 populations
#define VGX_IN_LDS_POPS 32      // the per-destination cells of a tree lie in LDS up to this P, in its row in global memory beyond
enum { VGX_IN_COUNT = 0, VGX_IN_CLADE_SUM = 1, VGX_IN_LOCAL_SUM = 2, VGX_IN_LOCAL_SUMSQ = 3, VGX_IN_EMPTY = 4, VGX_IN_MAX_LOCAL = 5 };
enum { VGX_IN_TIPS = 0, VGX_IN_INTRODUCTIONS = 1, VGX_IN_ROOT_POP = 2, VGX_IN_ROOT_LOCAL = 3, VGX_IN_ST_MAX_LOCAL = 4, VGX_IN_ST_MAX_CLADE = 5,
       VGX_IN_ST_EMPTY = 6, VGX_IN_POPS_WITH_TIPS = 7 };

// status of a replicate with a node label outside the model (arg = the lowest offending node): appended to the walk statuses
// 0 .. 12, VGX_GW_BAD_TREE and VGX_GW_BAD_RECORD
enum { VGX_GW_BAD_LABEL = 15 };

// per-node workspace of one tree (pointers private to it): children, children that pushed, tips pushed, local tips pushed
struct VgxInWork {
    int32_t *kids, *got, *n, *ln;
};

// floor(log2 v) for v >= 1
VGX_HD int vgx_in_bin(int32_t v) {
    int b = 0;
    for (uint32_t u = (uint32_t)v; u > 1; u >>= 1) b++;
    return b;
}

// cells of one row
VGX_HD int64_t vgx_in_row_cells(int64_t P) { return P * P + P * (1 + VGX_IN_INTO + VGX_IN_BINS) + VGX_IN_STATS; }

// The sequential sweep over one tree whose parents satisfy i < tree[i] < N (tree[N - 1] == -1) and whose P lies in
// 1 .. VGX_IN_POPS_MAX: the caller has checked both, so no access leaves the arrays.  Returns 0 and the five blocks, or
// VGX_GW_BAD_TREE / VGX_GW_BAD_LABEL with *arg the first offending node / the lowest node with a label outside [0, P); the five
// blocks are then zeros.  `w` is overwritten; clade and local, NULL or [N], hold every node's values after a return of 0.
VGX_HD int vgx_in_sweep(const int32_t *tree, const int32_t *pop, int64_t N, int64_t P, const VgxInWork &w, int32_t *clade, int32_t *local,
                        int64_t *tips_by_pop, int64_t *imports, int64_t *into, int64_t *spectrum, int64_t *stats, int64_t *arg) {
    for (int64_t k = 0; k < P; k++) tips_by_pop[k] = 0;
    for (int64_t k = 0; k < P * P; k++) imports[k] = 0;
    for (int64_t k = 0; k < P * VGX_IN_INTO; k++) into[k] = 0;
    for (int64_t k = 0; k < P * VGX_IN_BINS; k++) spectrum[k] = 0;
    for (int k = 0; k < VGX_IN_STATS; k++) stats[k] = 0;
    *arg = 0;
    for (int64_t i = 0; i < N; i++) { w.kids[i] = 0; w.got[i] = 0; w.n[i] = 0; w.ln[i] = 0; }
    for (int64_t i = 0; i < N - 1; i++) w.kids[tree[i]] += 1;
    for (int64_t i = 0; i < N; i++)
        if (w.kids[i] != 0 && w.kids[i] != 2) { *arg = i; return VGX_GW_BAD_TREE; }
    for (int64_t i = 0; i < N; i++)
        if (pop[i] < 0 || pop[i] >= P) { *arg = i; return VGX_GW_BAD_LABEL; }
    int64_t intro = 0, empty = 0, max_local = 0, max_clade = 0, with_tips = 0;
    for (int64_t i = 0; i < N; i++) {   // ascending ids: both children of i come before it
        const bool tip = w.kids[i] == 0;
        const int64_t c = tip ? 1 : w.n[i], l = tip ? 1 : w.ln[i], dst = pop[i];
        if (clade) clade[i] = (int32_t)c;
        if (local) local[i] = (int32_t)l;
        if (tip) tips_by_pop[dst] += 1;
        if (i == N - 1) {
            stats[VGX_IN_TIPS] = c; stats[VGX_IN_ROOT_POP] = dst; stats[VGX_IN_ROOT_LOCAL] = l;
            if (l > max_local) max_local = l;
            break;
        }
        const int64_t p = tree[i], src = pop[p];
        w.n[p] += (int32_t)c;
        w.got[p] += 1;
        if (src == dst) { w.ln[p] += (int32_t)l; continue; }
        imports[src * P + dst] += 1;
        int64_t *q = into + dst * VGX_IN_INTO;
        q[VGX_IN_COUNT] += 1;
        q[VGX_IN_CLADE_SUM] = vgx_ts_wrap_add(q[VGX_IN_CLADE_SUM], c);
        q[VGX_IN_LOCAL_SUM] = vgx_ts_wrap_add(q[VGX_IN_LOCAL_SUM], l);
        q[VGX_IN_LOCAL_SUMSQ] = vgx_ts_wrap_add(q[VGX_IN_LOCAL_SUMSQ], l * l);
        q[VGX_IN_EMPTY] += l == 0;
        if (l > q[VGX_IN_MAX_LOCAL]) q[VGX_IN_MAX_LOCAL] = l;
        if (l >= 1) spectrum[dst * VGX_IN_BINS + vgx_in_bin((int32_t)l)] += 1;
        intro += 1;
        empty += l == 0;
        if (c > max_clade) max_clade = c;
        if (l > max_local) max_local = l;
    }
    for (int64_t k = 0; k < P; k++) with_tips += tips_by_pop[k] > 0;
    stats[VGX_IN_INTRODUCTIONS] = intro; stats[VGX_IN_ST_MAX_LOCAL] = max_local; stats[VGX_IN_ST_MAX_CLADE] = max_clade;
    stats[VGX_IN_ST_EMPTY] = empty; stats[VGX_IN_POPS_WITH_TIPS] = with_tips;
    return 0;
}

// ---- device plumbing (vgx_api.hip, vgx_introductions.hip) --------------------------------------------------------------------------
// where a tree lies in the pass's node arrays
struct VgxInDesc { int64_t node_off, nodes; };

struct VgxInLaunch {
    int64_t n;                    // trees of this pass
    const VgxInDesc *desc;        // [n]
    const int64_t *res;           // NULL, or [n][5] the walk's VgxGwResult: a tree whose walk status is not 0 is skipped
    const int32_t *tree, *pop;    // node arrays of the pass: parents and the walk's tree_pop
    int64_t P;                    // populations, 1 .. VGX_IN_POPS_MAX
    VgxInWork w;                  // workspace of the pass, indexed like the node arrays
    int64_t *tips_by_pop;         // [n][P]          every block ZEROED by the caller before the launch: imports, and past
    int64_t *imports;             // [n][P][P]       VGX_IN_LDS_POPS the other per-destination blocks too, are counted in place
    int64_t *into;                // [n][P][6]
    int64_t *spectrum;            // [n][P][32]
    int64_t *stats;               // [n][8]
    int64_t *status;              // [n][2] status and its argument: the walk's, VGX_GW_BAD_TREE / VGX_GW_BAD_LABEL and the node
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_in_lineages(const VgxInLaunch *a, hipStream_t s);
#pragma GCC visibility pop
#endif
