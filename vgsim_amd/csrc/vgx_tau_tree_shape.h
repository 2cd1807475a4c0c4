// vgx_tau_tree_shape.h — the time of a node of a TAU chain's tree, written once for the host and the device, and the plumbing of the
// node-time kernel of vgx_tau_tree_shapes.hip (vgx_get_tau_tree_shapes, vgx_test_tau_node_times, vgx_test_tau_node_times_device;
// DESIGN.md §30).
//
// The walk of vgx_gwalk_tau.h leaves every node the chain's EVENT index: prefix events 0 .. n_pre - 1 (the model's chain before the
// tau call; n_pre = 0 for a replicate that restarted), the replicate's own step k is n_pre + k, and -1 for a node no event made.
// A tau chain needs no clock: a prefix event's time is the prefix's (pre_time[ev]), a step's time is the time of its MULTITYPE
// record (step_time[ev - n_pre], tau_log's), and all rows of a step share it, so two coalescences inside one step give a branch of
// length 0.  The branches and their order are those of the lookup in vgx_get_tau_genealogies: the same bits on every path.
#pragma once
#include <stdint.h>
#include "vgx_rng.h"   // VGX_HD

// the time of the node with event index ev; an index at or beyond n_pre + n_steps gives 0.0 and clears *ok.  Nothing is read
// outside pre_time[0, n_pre) and step_time[0, n_steps).
VGX_HD double vgx_tts_time_of(int32_t ev, int64_t n_pre, const double *pre_time, int64_t n_steps, const double *step_time, bool *ok) {
    if (ev < 0) return 0.0;
    if (ev < n_pre) return pre_time[ev];
    if (ev - n_pre < n_steps) return step_time[ev - n_pre];
    *ok = false;
    return 0.0;
}

// ---- device plumbing (host side <-> node-time kernel of vgx_tau_tree_shapes.hip) ---------------------------------------------------
// one tree of a launch: where its nodes lie in the pass's node arrays and its step times in the pass's step-time array (elements)
struct VgxTtsDesc {
    int64_t node_off, nodes;
    int64_t n_pre;                // prefix events of its chain: the length of the shared table, or 0 for a replicate that restarted
    int64_t step_off, n_steps;
};
struct VgxTtsLaunch {
    int64_t n;                    // trees of this launch
    const VgxTtsDesc *desc;       // [n]
    const int64_t *res;           // NULL, or [n][5] the walk's VgxGwResult: a tree whose walk status is not 0 is skipped
    const int32_t *node_ev;       // node event indices of the pass
    const double *pre_time;       // the prefix's event times, shared by every tree with n_pre > 0
    const double *step_time;      // step times of the pass's replicates, one behind the other
    double *times;                // out: node times, indexed like node_ev
    int32_t *bad;                 // out [n]: the lowest node whose index lies outside the chain, INT32_MAX for none
};

#ifdef __HIPCC__
#pragma GCC visibility push(hidden)
extern "C" hipError_t vgxi_tts_times(const VgxTtsLaunch *a, hipStream_t s);
#pragma GCC visibility pop
#endif
