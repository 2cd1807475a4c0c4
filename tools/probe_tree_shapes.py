"""Measurement of Ensemble.tree_shapes (vgx_get_tree_shapes) next to what a user did before it: genealogies() and a host sweep over
every replicate's tree.

Workload: that of tools/probe_lineages.py: c3_s5_p16 (16 populations, 1024 haplotypes), R = 4096 replicates x 10^5 events each in
one direct call with the event log.  In one process, ROUNDS times in alternation: tree_shapes(seed=None), and genealogies(seed=None)
followed by _capi.tree_shape over every healthy replicate.  Reported per round and as median [min, max]: the walk kernel, the shape
kernel, the host clock with the two node copies and the whole call of tree_shapes(); the kernel, host and whole call of
genealogies() and the time of the host loop after it.  Before anything is timed every row is compared with the host sweep over the
tree genealogies() returns.

    python tools/probe_tree_shapes.py [--rounds 6] [--out profiles/tree_shapes.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v), "rounds": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator, _capi
    from vgsim_amd.ensemble import Ensemble

    R = a.replicates
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)

    def old_route():
        t0 = time.perf_counter()
        b = ens.genealogies(seed=None)
        t1 = time.perf_counter()
        rows = {}
        for i in np.nonzero(b.status == 0)[0]:
            o0, o1 = b.node_offsets[i], b.node_offsets[i + 1]
            rows[int(i)] = _capi.tree_shape(b.tree[o0:o1], np.zeros(o1 - o0, dtype=np.int64), b.times[o0:o1])
        t2 = time.perf_counter()
        return b, rows, (t1 - t0) * 1e3, (t2 - t1) * 1e3

    # warm-up (code objects, allocator), and the checks
    ts = ens.tree_shapes(seed=None)
    b, rows, _, _ = old_route()
    assert np.array_equal(ts.status, b.status) and np.array_equal(ts.rng_raw, b.rng_raw)
    worst = 0.0
    for i, (st, ln) in rows.items():
        assert np.array_equal(ts.stats[i, :10], st[:10]), "row %d differs from the host sweep" % i
        assert all(ts.lengths[i, k] == ln[k] for k in (0, 1, 6)), "row %d: exact lengths" % i
        N = 2 * int(ts.tips[i]) - 1
        for k in (2, 3, 4, 5):
            assert abs(ts.lengths[i, k] - ln[k]) <= 2 * (N + 2) * 2.0 ** -53 * ln[k], "row %d: sum %d" % (i, k)
            if ln[k] > 0:
                worst = max(worst, abs(ts.lengths[i, k] - ln[k]) / (2 * (N + 2) * 2.0 ** -53 * ln[k]))
    names = ("walk_ms", "shape_ms", "clock_ms", "wall_ms")
    t_r = {k: [] for k in names}
    t_old = {k: [] for k in ("genealogies_kernel_ms", "genealogies_host_ms", "genealogies_wall_ms", "host_sweep_ms", "route_wall_ms")}
    for rnd in range(a.rounds):
        ts = ens.tree_shapes(seed=None)
        b, _, g_ms, h_ms = old_route()
        for k, v in zip(names, tuple(ts.kernel_ms) + (ts.clock_ms, ts.wall_ms)):
            t_r[k].append(v)
        for k, v in zip(t_old, (b.kernel_ms, b.clock_ms, b.wall_ms, h_ms, g_ms + h_ms)):
            t_old[k].append(v)
        print("round", rnd, "tree_shapes walk %.3f ms, shape %.3f ms, clock %.1f ms, call %.1f ms;  genealogies %.1f ms + host sweep %.1f ms"
              % (ts.kernel_ms[0], ts.kernel_ms[1], ts.clock_ms, ts.wall_ms, g_ms, h_ms), flush=True)
    ok = ts.ok
    out = {"workload": "c3_s5_p16", "replicates": R, "events_asked": a.events, "total_events": int(res.events.sum()), "rounds": a.rounds,
           "kernel": ens.engine.last_kernel, "passes": ts.passes, "healthy_walks": int(ok.sum()),
           "nodes": int((2 * ts.tips[ok] - 1).sum()), "tips_median": float(np.median(ts.tips[ok])), "tips_max": int(ts.tips[ok].max()),
           "max_depth_median": float(np.median(ts.max_depth[ok])), "colless_normalized_median": float(np.nanmedian(ts.colless_normalized())),
           "worst_sum_error_over_bound": worst,
           "tree_shapes": {k: stats(v) for k, v in t_r.items()},
           "genealogies_then_host_sweep": {k: stats(v) for k, v in t_old.items()}}
    sr = out["tree_shapes"]
    out["shape_over_walk"] = sr["shape_ms"]["median"] / sr["walk_ms"]["median"]
    out["route_over_call"] = out["genealogies_then_host_sweep"]["route_wall_ms"]["median"] / sr["wall_ms"]["median"]
    ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
