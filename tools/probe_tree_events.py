"""Measurement of Ensemble.tree_events (vgx_get_tree_events) next to Ensemble.lineages on the same ensemble and the same logs.

Workload: that of tools/probe_lineages.py: c3_s5_p16 (16 populations, 1024 haplotypes), R = 4096 replicates x 10^5 events each in
one direct call with the event log, T = 100 grid points over [0, the earliest final time among the first 64 replicates], four
variant classes (64 cells for lineages(), 448 for tree_events()).  In one process, ROUNDS times in alternation: lineages(seed=None)
and tree_events(seed=None), both with a summary and without the block on the host.  Reported per round and as median [min, max]:
the walk, binning and suffix-sum kernels of lineages() (Lineages.stage_ms), the walk and binning kernels of tree_events()
(TreeEvents.stage_ms), and the host clock and whole call of both.  The walk kernel is the same in both calls, so the tool also
reports whether the two medians of the walk differ by more than the run-to-run spread (max - min) of either series.  Before
anything is timed a few rows are compared with the host replay of the rule, and tree_events().lineages() with lineages().

    python tools/probe_tree_events.py [--rounds 5] [--out profiles/tree_events.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    R = a.replicates
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    m = ens.model
    t_end = min(float(ens.replicate_state(r).currentTime) for r in range(min(R, 64)))
    window = (0.0, t_end)
    variants = (np.arange(m.hapNum) % 4).astype(np.int64)
    # warm-up (code objects, allocator), and the checks
    ln = ens.lineages(points=a.points, window=window, variants=variants, seed=None)
    te = ens.tree_events(points=a.points, window=window, variants=variants, seed=None)
    got = te.lineages()
    for k in ("values", "root", "status", "status_arg", "records", "rng_raw"):
        assert np.array_equal(getattr(got, k), getattr(ln, k)), "tree_events().lineages() differs from lineages(): " + k
    from test_hip_tree_events import _host_row
    for r in (0, 1, R - 1):
        if te.ok[r]:
            assert np.array_equal(te.counts[r], _host_row(ens, r, None, te.times, te.variant_of, 4)["counts"]), "row %d differs from the host replay" % r
    channel_totals = dict(zip(te.CHANNELS, te.counts.sum(axis=(0, 1, 2, 3), dtype=np.int64).tolist()))
    names_ln = ("walk_ms", "binning_ms", "scan_ms", "kernels_ms", "clock_ms", "wall_ms")
    names_te = ("walk_ms", "binning_ms", "kernels_ms", "clock_ms", "wall_ms")
    t_ln, t_te = {k: [] for k in names_ln}, {k: [] for k in names_te}
    for rnd in range(a.rounds):
        ln = ens.lineages(points=a.points, window=window, variants=variants, seed=None, summary=dict(quantiles=(0.5,)), values=False)
        te = ens.tree_events(points=a.points, window=window, variants=variants, seed=None, summary=dict(quantiles=(0.5,)), values=False)
        for k, v in zip(names_ln, tuple(ln.stage_ms) + (ln.kernel_ms, ln.clock_ms, ln.wall_ms)):
            t_ln[k].append(v)
        for k, v in zip(names_te, tuple(te.stage_ms) + (te.kernel_ms, te.clock_ms, te.wall_ms)):
            t_te[k].append(v)
        print("round", rnd, "lineages walk %.3f ms, binning %.3f ms, scan %.3f ms (clock %.1f ms, call %.1f ms);  "
              "tree_events walk %.3f ms, binning %.3f ms (clock %.1f ms, call %.1f ms)"
              % (tuple(ln.stage_ms) + (ln.clock_ms, ln.wall_ms) + tuple(te.stage_ms) + (te.clock_ms, te.wall_ms)), flush=True)
    w_ln, w_te = stats(t_ln["walk_ms"]), stats(t_te["walk_ms"])
    diff = w_te["median"] - w_ln["median"]
    spread = max(w_ln["max"] - w_ln["min"], w_te["max"] - w_te["min"])
    out = {"workload": "c3_s5_p16", "replicates": R, "events_asked": a.events, "total_events": int(res.events.sum()), "rounds": a.rounds,
           "kernel": ens.engine.last_kernel, "points": a.points, "window": list(window), "classes": 4,
           "cells_lineages": int(m.popNum) * 4, "cells_tree_events": int(m.popNum) * 4 * len(te.CHANNELS), "passes": te.passes,
           "healthy_walks": int(te.ok.sum()), "lineage_records": int(te.records.sum()), "channel_totals": channel_totals,
           "lineages": {k: dict(stats(v), rounds=v) for k, v in t_ln.items()},
           "tree_events": {k: dict(stats(v), rounds=v) for k, v in t_te.items()},
           "walk_tree_events_vs_lineages": {"median_difference_ms": diff, "largest_run_to_run_spread_ms": spread,
                                            "difference_exceeds_spread": bool(abs(diff) > spread)}}
    ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
