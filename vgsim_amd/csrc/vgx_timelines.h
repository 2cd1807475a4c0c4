// vgx_timelines.h — launch arguments of the replay kernel (vgx_timelines.hip), filled by vgx_get_timelines (vgx_api.hip).
#pragma once
#include <stdint.h>

struct VgxTlLaunch {
    int64_t m;               // replicates of this pass = workgroups
    const int32_t *log;      // r_evcols: [R][evcap][6]
    int64_t evcap;
    const int64_t *rep;      // [m] replicate of every row
    const int32_t *n_ev;     // [m] events of its chain
    const int32_t *last;     // [m] last_point
    const int32_t *cut;      // [m][step]
    int step, semantics;
    int ni, ns;              // queries of this launch
    int i0, s0;              // ... their first index among all queries of the call
    int n_inf, n_sus;        // all queries of the call (row strides of the outputs)
    int tsize;               // slots of the query table
    const int32_t *tab;      // [3][tsize] major, minor', row
    const int64_t *start;    // [ni + ns] initial_infectious / initial_susceptible of the queried compartments
    double *inf, *smp, *sus; // [m][n_inf][T], [m][n_inf][T], [m][n_sus][T]
};
