"""Measurement of Ensemble.milestones (vgx_get_milestones) next to Ensemble.prevalence on the same ensemble.

Workload: c3_s5_p16 (16 populations, 1024 haplotypes), R = 4096 replicates x 10^5 events each in one direct call with the event
log (the ensemble shape of tools/probe_prevalence.py).  milestones(thresholds=(10, 100, 1000)) and prevalence(points=53) over
[0, the earliest final time among the first 64 replicates], with two variant maps: every haplotype its own class up to the LDS
limit of the walk ((P + 1) * V * 4 * (4 + 3) <= 65536 bytes: the first 137 haplotypes, the rest not tracked) and three classes.
In one process, ROUNDS times in alternation: milestones with one wavefront per (replicate, tile) (the shape kept), milestones with
four wavefronts taking rounds in turn (VGX_MILESTONES_WAVES=4), prevalence, and an incidence call whose window lies behind every
event (it packs the clock inputs and counts nothing: the pack kernel alone, which all of them run first).  Reported, median
[min, max]: kernel, clock and wall ms of the calls, the kernels without the pack kernel, the walk's cost per event next to the
histogram pass's, and the ratio of the two.
Before anything is timed `final` is compared with replicate_state() for a few replicates, the two shapes with each other, and
peak with the largest value prevalence sees on its grid.

    python tools/probe_milestones.py [--rounds 5] [--out profiles/milestones.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

THRESHOLDS = (10, 100, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--points", type=int, default=53)
    ap.add_argument("--tile", type=int, default=0, help="VGX_MILESTONES_TILE_EVENTS for this run (0: the default, 4096)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.tile:
        os.environ["VGX_MILESTONES_TILE_EVENTS"] = str(a.tile)
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    def milestones(waves, variants):
        if waves == 4:
            os.environ["VGX_MILESTONES_WAVES"] = "4"
        try:
            return ens.milestones(variants=variants, thresholds=THRESHOLDS)
        finally:
            os.environ.pop("VGX_MILESTONES_WAVES", None)

    R = a.replicates
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    m = ens.model
    P, H, K = int(m.popNum), int(m.hapNum), len(THRESHOLDS)
    t_end = min(float(ens.replicate_state(r).currentTime) for r in range(min(R, 64)))
    window = (0.0, t_end)
    total = int(res.events.sum())
    behind = [t_end * 1e6, t_end * 2e6]
    v_max = min(65536 // ((P + 1) * 4 * (4 + K)), H)
    own = np.where(np.arange(H) < v_max, np.arange(H), -1)
    out = {"workload": "c3_s5_p16", "replicates": R, "events_asked": a.events, "total_events": total, "points": a.points, "window": list(window),
           "thresholds": list(THRESHOLDS), "rounds": a.rounds, "kernel": ens.engine.last_kernel, "tile_events": a.tile or 4096, "variants": {}}
    for name, variants in (("own_class_up_to_the_lds_limit", own), ("three_classes", np.arange(H) % 3)):
        ms = milestones(1, variants)                                                         # warm-up and checks
        ms4 = milestones(4, variants)
        some = np.arange(min(R, 256), dtype=np.int64)
        pv = ens.prevalence(points=a.points, window=window, variants=variants, replicates=some)
        for k in ("final", "peak", "peak_event", "last_positive_event", "first_event"):
            assert np.array_equal(getattr(ms, k), getattr(ms4, k)), "the two workgroup shapes differ in " + k
        for r in (0, 1, R - 1):
            inf = ens.replicate_state(r).infectious
            want = np.stack([inf[:, ms.variant_of == c].sum(axis=1) for c in range(ms.final.shape[2])], axis=1)
            assert np.array_equal(ms.final[r, :P], want), "final differs from the replicate's state"
        assert np.array_equal(ms.final[some, :P], pv.final) and (ms.peak[some, :P] >= pv.values.max(axis=1)).all()
        del pv
        keys = ("milestones", "milestones_four_waves", "prevalence")
        timed = {k + "_" + f: [] for k in keys for f in ("kernels_ms", "clock_ms", "wall_ms")}
        timed["pack_only_ms"] = []
        for rnd in range(a.rounds):
            got = (milestones(1, variants), milestones(4, variants),
                   ens.prevalence(points=a.points, window=window, variants=variants, summary=dict(quantiles=(0.5,)), values=False))
            for k, g in zip(keys, got):
                timed[k + "_kernels_ms"].append(g.kernel_ms)
                timed[k + "_clock_ms"].append(g.clock_ms)
                timed[k + "_wall_ms"].append(g.wall_ms)
            timed["pack_only_ms"].append(ens.incidence(edges=behind).kernel_ms)
            print(name, "round", rnd, " ".join("%s %.3f ms" % (k, v[-1]) for k, v in timed.items()), flush=True)
        pack = np.asarray(timed["pack_only_ms"])
        walk, walk4, hist = (np.asarray(timed[k + "_kernels_ms"]) - pack for k in keys)
        V = int(ms.final.shape[2])
        out["variants"][name] = dict(
            V=V, cells=(P + 1) * V, lds_record_bytes=(P + 1) * V * 4 * (4 + K), passes=ms.passes, rounds_ms=timed,
            milestones_passes_ms=stats(walk), milestones_four_waves_passes_ms=stats(walk4), prevalence_count_and_scan_ms=stats(hist),
            milestones_ns_per_event=float(np.median(walk)) * 1e6 / total, milestones_four_waves_ns_per_event=float(np.median(walk4)) * 1e6 / total,
            prevalence_ns_per_event=float(np.median(hist)) * 1e6 / total,
            milestones_over_prevalence=stats(walk / hist), four_waves_over_one=stats(walk4 / walk),
            **{k + "_" + f: stats(timed[k + "_" + f]) for k in keys for f in ("clock_ms", "wall_ms")})
        print(name, json.dumps({k: v for k, v in out["variants"][name].items() if k != "rounds_ms"}), flush=True)
        if a.out:    # (written after every variant map: a later one that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    ens.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
