// vgx_tree_shape.h — the shape of one sampled tree as a row of scalars: balance (Sackin, Colless, cherries, pitchforks, ladders),
// depth, height and branch lengths, written once for the host and the device.  vgx_tree_shapes.hip runs it over the trees the walk
// of vgx_gwalk.h left on the device (vgx_get_tree_shapes) and over hand-made trees (vgx_test_tree_shape_device); the host hook
// vgx_test_tree_shape (vgx_genealogy.cpp) runs the sequential sweep below.  DESIGN.md §29.
//
// Input, one tree of N nodes: tree[N] int32 parents, node_ev[N] int32 event indices, times[N] f64 node times.
// Precondition (what a walk with status 0 leaves: node() hands out ids in creation order, all 2 sCounter - 1 nodes are used, every
// coalescence joins two lineages): N is odd and >= 3, tree[N - 1] == -1, i < tree[i] < N for every other node, and every node has 0
// or 2 children.  Then every child has a lower id than its parent and ONE ascending sweep over the ids finds every node with all
// its children done.  Node times do not increase with the id, so every branch b_i = times[i] - times[tree[i]] is >= 0.
//
// A tip is a node without children.  Every per-node quantity is what the children push into the parent:
//   n_v        tips below                        tip 1   node: sum_c n_c
//   A_v        sum of the tip depths from v      tip 0   node: sum_c (A_c + n_c)
//   B_v        sum of the squared tip depths     tip 0   node: sum_c (B_c + 2 A_c + n_c)
//   h_v        height in edges                   tip 0   node: 1 + max_c h_c
//   tipkids_v  tip children                              node: their number
//   minkid_v   the smaller child                         node: min_c n_c
//   lad_v      ladder ending at v                tip 0   node: 1 + max_c lad_c if tipkids_v == 1, else 0
// sums, maxima and minima only: the order of the pushes does not matter, which is what lets 64 lanes push with atomics.
//
// stats[VGX_TS_K] int64 (wrapping sums): tips, internal, cherries (tipkids == 2), pitchforks (n_v == 3), sackin (A_root), colless
// (sum over internal nodes of n_v - 2 minkid_v), max_depth (h_root), depth_sumsq (B_root), ladder_nodes (tipkids == 1), max_ladder
// (max_v lad_v), root_event (node_ev[N - 1]), last_tip_event (node_ev[0]).  depth_sumsq is of the order of tips^3 (tips^3 / 3 for a
// caterpillar tree): it wraps beyond about 2 * 10^6 tips of a caterpillar tree (2^63 at 3 * 10^6); every other sum stays below tips^2.
// lengths[VGX_TS_L] f64: root_time (times[N - 1]), last_tip_time (times[0]), length (sum b_i), external_length (sum over tips of
// b_i), length_sumsq (sum b_i^2), tip_height_sum (sum over tips of times[i] - root_time), max_branch (max b_i).  Indices 0, 1 and 6
// are exact: the same bits on every path.  The four sums may be taken in any order: two orders differ by at most
// 2 (m + 2) 2^-53 S for m non-negative terms of sum S.
#pragma once
#include <stdint.h>
#include "vgx_rng.h"   // VGX_HD

#define VGX_TS_K 12   // integer statistics
#define VGX_TS_L 7    // lengths
enum { VGX_TS_TIPS = 0, VGX_TS_INTERNAL = 1, VGX_TS_CHERRIES = 2, VGX_TS_PITCHFORKS = 3, VGX_TS_SACKIN = 4, VGX_TS_COLLESS = 5,
       VGX_TS_MAX_DEPTH = 6, VGX_TS_DEPTH_SUMSQ = 7, VGX_TS_LADDER_NODES = 8, VGX_TS_MAX_LADDER = 9, VGX_TS_ROOT_EVENT = 10,
       VGX_TS_LAST_TIP_EVENT = 11 };
enum { VGX_TS_ROOT_TIME = 0, VGX_TS_LAST_TIP_TIME = 1, VGX_TS_LENGTH = 2, VGX_TS_EXTERNAL_LENGTH = 3, VGX_TS_LENGTH_SUMSQ = 4,
       VGX_TS_TIP_HEIGHT_SUM = 5, VGX_TS_MAX_BRANCH = 6 };

// status of a replicate whose tree breaks the precondition (arg = the first offending node): appended to the walk statuses of
// vgx_gwalk.h (0 .. 9) and vgx_gwalk_tau.h (10 .. 12)
enum { VGX_GW_BAD_TREE = 13 };

#define VGX_TS_NODE_BYTES 44   // accumulators of one node: seven int32 and two int64

// per-node accumulators of one tree (pointers private to it)
struct VgxTsWork {
    int32_t *n, *h, *lad, *tipkids, *minkid, *kids, *got;
    int64_t *A, *B;
};

VGX_HD int64_t vgx_ts_wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// what node i is once all its children have pushed (kids = 0 or 2)
struct VgxTsNode {
    int32_t n, h, lad, tipkids, minkid;
    int64_t A, B;
};

// node i's row of the integer block: what it adds to the sums and maxima
VGX_HD void vgx_ts_count(const VgxTsNode &v, bool tip, int64_t *stats) {
    if (tip) { stats[VGX_TS_TIPS] += 1; return; }
    stats[VGX_TS_INTERNAL] += 1;
    stats[VGX_TS_CHERRIES] += v.tipkids == 2;
    stats[VGX_TS_PITCHFORKS] += v.n == 3;
    stats[VGX_TS_COLLESS] += (int64_t)v.n - 2 * (int64_t)v.minkid;
    stats[VGX_TS_LADDER_NODES] += v.tipkids == 1;
    if (v.lad > stats[VGX_TS_MAX_LADDER]) stats[VGX_TS_MAX_LADDER] = v.lad;
}

// branch i (i < N - 1) into the float block's sums and maximum
VGX_HD void vgx_ts_branch(double t, double t_parent, double t_root, bool tip, double *len) {
    const double b = t - t_parent;
    len[VGX_TS_LENGTH] += b;
    len[VGX_TS_LENGTH_SUMSQ] += b * b;
    if (tip) {
        len[VGX_TS_EXTERNAL_LENGTH] += b;
        len[VGX_TS_TIP_HEIGHT_SUM] += t - t_root;
    }
    if (b > len[VGX_TS_MAX_BRANCH]) len[VGX_TS_MAX_BRANCH] = b;
}

// The sequential sweep over one tree whose parents satisfy i < tree[i] < N (tree[N - 1] == -1): the caller has checked that, so no
// access leaves the arrays.  Returns -1 and the two blocks, or the first node with one child or more than two (the blocks are then
// undefined).  `w` is overwritten.
VGX_HD int64_t vgx_ts_sweep(const int32_t *tree, const int32_t *node_ev, const double *times, int64_t N, const VgxTsWork &w, int64_t *stats,
                            double *len) {
    for (int64_t i = 0; i < N; i++) {
        w.n[i] = 0; w.h[i] = 0; w.lad[i] = 0; w.tipkids[i] = 0; w.minkid[i] = INT32_MAX; w.kids[i] = 0; w.got[i] = 0;
        w.A[i] = 0; w.B[i] = 0;
    }
    for (int64_t i = 0; i < N - 1; i++) w.kids[tree[i]] += 1;
    for (int k = 0; k < VGX_TS_K; k++) stats[k] = 0;
    for (int k = 0; k < VGX_TS_L; k++) len[k] = 0.0;
    const double t_root = times[N - 1];
    for (int64_t i = 0; i < N; i++) {
        const int32_t kids = w.kids[i];
        if (kids != 0 && kids != 2) return i;
        const bool tip = kids == 0;
        VgxTsNode v;
        if (tip) { v.n = 1; v.h = 0; v.lad = 0; v.tipkids = 0; v.minkid = 0; v.A = 0; v.B = 0; }
        else {
            v.n = w.n[i]; v.h = w.h[i]; v.tipkids = w.tipkids[i]; v.minkid = w.minkid[i]; v.A = w.A[i]; v.B = w.B[i];
            v.lad = v.tipkids == 1 ? w.lad[i] : 0;
        }
        vgx_ts_count(v, tip, stats);
        if (i == N - 1) {
            stats[VGX_TS_SACKIN] = v.A; stats[VGX_TS_MAX_DEPTH] = v.h; stats[VGX_TS_DEPTH_SUMSQ] = v.B;
            break;
        }
        const int32_t p = tree[i];
        w.n[p] += v.n;
        w.A[p] = vgx_ts_wrap_add(w.A[p], vgx_ts_wrap_add(v.A, v.n));
        w.B[p] = vgx_ts_wrap_add(w.B[p], vgx_ts_wrap_add(vgx_ts_wrap_add(v.B, (int64_t)(2 * (uint64_t)v.A)), v.n));
        if (v.h + 1 > w.h[p]) w.h[p] = v.h + 1;
        w.tipkids[p] += tip;
        if (v.n < w.minkid[p]) w.minkid[p] = v.n;
        if (v.lad + 1 > w.lad[p]) w.lad[p] = v.lad + 1;
        w.got[p] += 1;
        vgx_ts_branch(times[i], times[p], t_root, tip, len);
    }
    stats[VGX_TS_ROOT_EVENT] = node_ev[N - 1];
    stats[VGX_TS_LAST_TIP_EVENT] = node_ev[0];
    len[VGX_TS_ROOT_TIME] = t_root;
    len[VGX_TS_LAST_TIP_TIME] = times[0];
    return -1;
}

// The precondition on the parents alone.  Returns -1, or the first node that breaks it (N for a node count that is even or below 3).
VGX_HD int64_t vgx_ts_check_parents(const int32_t *tree, int64_t N) {
    if (N < 3 || N % 2 == 0 || N > INT32_MAX) return N;
    for (int64_t i = 0; i < N - 1; i++)
        if (tree[i] <= i || tree[i] >= N) return i;
    return tree[N - 1] == -1 ? -1 : N - 1;
}

// ---- device plumbing (vgx_api.hip <-> vgx_tree_shapes.hip) ----------------------------------------------------------------------
struct VgxTsDesc { int64_t node_off, nodes; };   // where a tree lies in the pass's node arrays; nodes = 2 sCounter - 1

struct VgxTsLaunch {
    int64_t n;                    // trees of this pass
    const VgxTsDesc *desc;        // [n]
    const int64_t *res;           // NULL, or [n][5] the walk's VgxGwResult: a tree whose walk status is not 0 is skipped
    const int32_t *tree, *node_ev;   // node arrays of the pass
    const double *times;
    VgxTsWork w;                  // accumulators of the pass, indexed like the node arrays
    int64_t *stats;               // [n][VGX_TS_K]
    double *lengths;              // [n][VGX_TS_L]
    int64_t *status;              // [n][2] status and its argument: the walk's, or VGX_GW_BAD_TREE and the node
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_ts_shape(const VgxTsLaunch *a, hipStream_t s);
#pragma GCC visibility pop
#endif
