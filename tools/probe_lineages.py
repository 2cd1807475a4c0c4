"""Measurement of Ensemble.lineages (vgx_get_lineages) next to Ensemble.genealogies on the same ensemble.

Workload: c3_s5_p16 (16 populations, 1024 haplotypes), R = 4096 replicates x 10^5 events each in one direct call with the event
log (the ensemble of tools/probe_ensemble_genealogy.py and tools/probe_prevalence.py), T = 100 grid points over [0, the earliest
final time among the first 64 replicates], four variant classes (64 cells).  In one process, ROUNDS times in alternation:
genealogies(seed=None) and lineages(seed=None).  Reported per round and as median [min, max]: the device time of the walk kernel
of genealogies() (GenealogyBatch.kernel_ms); the walk, binning and suffix-sum kernels of lineages() apart (Lineages.stage_ms), its
host clock and its whole call.  Before anything is timed a few rows are compared with the host replay of the rule, and status and
generator with those of genealogies().

The shared walk header changed when lineages() was added (an observer template parameter whose default does nothing), so the same
figure of genealogies() is wanted from the commit before: run this tool there with --genealogies-only (it then touches nothing
that commit lacks) and give the result here with --parent FILE.json.  The finding reported is whether the difference of the two
medians exceeds the run-to-run spread (max - min) observed in either series.

    python tools/probe_lineages.py [--rounds 5] [--parent PARENT.json] [--out profiles/lineages.json]
    python tools/probe_lineages.py --genealogies-only [--rounds 5] --out PARENT.json        (on the commit before)
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
    ap.add_argument("--genealogies-only", action="store_true")
    ap.add_argument("--parent", default=None, help="the --genealogies-only result of the commit before")
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
    out = {"workload": "c3_s5_p16", "replicates": R, "events_asked": a.events, "total_events": int(res.events.sum()), "rounds": a.rounds,
           "kernel": ens.engine.last_kernel}
    ens.genealogies(seed=None, replicates=np.arange(min(R, 64)))   # warm-up (code objects, allocator)
    gen_ms = []
    if a.genealogies_only:
        for rnd in range(a.rounds):
            b = ens.genealogies(seed=None)
            gen_ms.append(b.kernel_ms)
            print("round", rnd, "genealogies walk kernel %.3f ms" % b.kernel_ms, flush=True)
        out["genealogies_walk_kernel_ms"] = dict(stats(gen_ms), rounds=gen_ms)
    else:
        m = ens.model
        t_end = min(float(ens.replicate_state(r).currentTime) for r in range(min(R, 64)))
        window = (0.0, t_end)
        variants = (np.arange(m.hapNum) % 4).astype(np.int64)
        ln = ens.lineages(points=a.points, window=window, variants=variants, seed=None)   # warm-up, and the check
        b = ens.genealogies(seed=None)
        assert np.array_equal(ln.status, b.status) and np.array_equal(ln.rng_raw, b.rng_raw), "the walk differs from that of genealogies()"
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_hip_lineages import _host_row
        for r in (0, 1, R - 1):
            if ln.ok[r]:
                want = _host_row(ens, r, None, ln.times, ln.variant_of, 4)
                assert np.array_equal(ln.values[r], want["values"]) and np.array_equal(ln.root[r], want["root"]), "row %d differs from the host replay" % r
        timed = {k: [] for k in ("walk_ms", "binning_ms", "scan_ms", "lineages_kernels_ms", "lineages_clock_ms", "lineages_wall_ms")}
        for rnd in range(a.rounds):
            b = ens.genealogies(seed=None)
            ln = ens.lineages(points=a.points, window=window, variants=variants, seed=None, summary=dict(quantiles=(0.5,)), values=False)
            gen_ms.append(b.kernel_ms)
            for k, v in zip(timed, tuple(ln.stage_ms) + (ln.kernel_ms, ln.clock_ms, ln.wall_ms)):
                timed[k].append(v)
            print("round", rnd, "genealogies walk kernel %.3f ms;  lineages walk %.3f ms, binning %.3f ms, scan %.3f ms (clock %.1f ms, call %.1f ms)"
                  % ((b.kernel_ms,) + tuple(ln.stage_ms) + (ln.clock_ms, ln.wall_ms)), flush=True)
        out.update(points=a.points, window=list(window), classes=4, cells=int(m.popNum) * 4, passes=ln.passes, healthy_walks=int(ln.ok.sum()),
                   lineage_records=int(ln.records.sum()), genealogies_walk_kernel_ms=dict(stats(gen_ms), rounds=gen_ms),
                   lineages={k: dict(stats(v), rounds=v) for k, v in timed.items()})
        if a.parent:
            with open(a.parent) as f:
                parent = json.load(f)["genealogies_walk_kernel_ms"]
            child = out["genealogies_walk_kernel_ms"]
            diff = child["median"] - parent["median"]
            spread = max(parent["max"] - parent["min"], child["max"] - child["min"])
            out["genealogies_walk_parent_vs_child"] = {
                "parent_ms": parent, "child_ms": child, "median_difference_ms": diff, "largest_run_to_run_spread_ms": spread,
                "difference_exceeds_spread": bool(abs(diff) > spread)}
    ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
