"""Measurement of Ensemble.prevalence (vgx_get_prevalence) next to Ensemble.incidence on the same ensemble and grid.

Workload: c3_s5_p16 (16 populations, 1024 haplotypes), R = 4096 replicates x 10^5 events each in one direct call with the event
log (the ensemble shape of tools/probe_incidence.py), T = 100 grid points / bins over [0, the earliest final time among the first
64 replicates] (--window latest: up to the latest one, so that nearly every event lies inside the window and both calls read
about the same bytes).  Three variant maps: every haplotype its own class (1024 classes: P * V = 16384 cells, the LDS limit),
64 classes (1024 cells) and four classes (64 cells).
In one process, ROUNDS times in alternation: prevalence, incidence, and an incidence call whose window lies behind every event
(it packs the clock inputs and counts nothing: the pack kernel alone, which both calls run first).  Reported, median [min, max]:
ms[0] (all kernels) and ms[1] (host clock) of either call; the counting + scan kernels of prevalence and the counting kernel of
incidence as ms[0] minus the pack kernel; the log bytes either reads (24 per event: prevalence reads every event of a chain,
the tail after the last grid point included, incidence those inside the window) over that time next to the HBM peak; and the
same figure of a prevalence call with ONE grid point, whose block and scan are a hundredth of the full call's: what the counting
pass costs without them.
Before anything is timed the final block is compared with replicate_state() for a few replicates.

    python tools/probe_prevalence.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK_TBS = 8.0    # MI355X, specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--window", choices=("earliest", "latest"), default="earliest")
    ap.add_argument("--tile", type=int, default=0, help="VGX_PREVALENCE_TILE_EVENTS for this run (0: the default, 4096)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.tile:
        os.environ["VGX_PREVALENCE_TILE_EVENTS"] = str(a.tile)
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    R = a.replicates
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    m = ens.model
    t_end = (min if a.window == 'earliest' else max)(float(ens.replicate_state(r).currentTime) for r in range(min(R, 64)))
    window = (0.0, t_end)
    total = int(res.events.sum())
    behind = [t_end * 1e6, t_end * 2e6]
    out = {"workload": "c3_s5_p16", "replicates": R, "events_asked": a.events, "total_events": total, "points": a.points, "window_end": a.window, "window": list(window),
           "rounds": a.rounds, "hbm_peak_TBs": HBM_PEAK_TBS, "kernel": ens.engine.last_kernel, "tile_events": a.tile or 4096, "variants": {}}
    for name, variants in (("identity", None), ("sixty_four_classes", np.arange(m.hapNum) % 64), ("four_classes", np.arange(m.hapNum) % 4)):
        pv = ens.prevalence(points=a.points, window=window, variants=variants, summary=dict(quantiles=(0.5,)), values=False)   # warm-up
        for r in (0, 1, R - 1):
            inf = ens.replicate_state(r).infectious
            want = np.stack([inf[:, pv.variant_of == c].sum(axis=1) for c in range(pv.final.shape[2])], axis=1)
            assert np.array_equal(pv.final[r], want), "final differs from the replicate's state"
        ens.incidence(bins=a.points, window=window, summary=dict(quantiles=(0.5,)), counts=False)
        timed = {k: [] for k in ("prevalence_kernels_ms", "prevalence_clock_ms", "incidence_kernels_ms", "incidence_clock_ms", "pack_only_ms",
                                 "prevalence_one_point_kernels_ms")}
        for rnd in range(a.rounds):
            pv = ens.prevalence(points=a.points, window=window, variants=variants, summary=dict(quantiles=(0.5,)), values=False)
            inc = ens.incidence(bins=a.points, window=window, summary=dict(quantiles=(0.5,)), counts=False)
            tb = ens.incidence(edges=behind).kernel_ms
            one = ens.prevalence(points=1, window=window, variants=variants, summary=dict(quantiles=(0.5,)), values=False).kernel_ms
            for k, v in zip(timed, (pv.kernel_ms, pv.clock_ms, inc.kernel_ms, inc.clock_ms, tb, one)):
                timed[k].append(v)
            print(name, "round", rnd, "prevalence kernels %.3f ms (clock %.1f ms; one point %.3f ms)  incidence kernels %.3f ms (clock %.1f ms)  pack alone %.3f ms"
                  % (pv.kernel_ms, pv.clock_ms, one, inc.kernel_ms, inc.clock_ms, tb), flush=True)
        pack = np.asarray(timed["pack_only_ms"])
        prev_ms = np.asarray(timed["prevalence_kernels_ms"]) - pack
        inc_ms = np.asarray(timed["incidence_kernels_ms"]) - pack
        prev_bytes, inc_bytes = 24 * total, 24 * int(total - inc.outside.sum())
        p_med, i_med = float(np.median(prev_ms)), float(np.median(inc_ms))
        V = int(pv.final.shape[2])
        out["variants"][name] = dict(
            V=V, cells=int(m.popNum * V), block_bytes=4 * R * (a.points + 1) * int(m.popNum) * V, passes=pv.passes, rounds_ms=timed,
            prevalence_count_and_scan_ms=stats(prev_ms),
            prevalence_one_point_count_and_scan_ms=stats(np.asarray(timed["prevalence_one_point_kernels_ms"]) - pack), incidence_count_ms=stats(inc_ms), prevalence_over_incidence=stats(prev_ms / inc_ms),
            prevalence_log_bytes=prev_bytes, incidence_log_bytes=inc_bytes,
            prevalence_TBs=prev_bytes / (p_med * 1e-3) / 1e12 if p_med > 0 else None,
            incidence_TBs=inc_bytes / (i_med * 1e-3) / 1e12 if i_med > 0 else None,
            prevalence_clock_ms=stats(timed["prevalence_clock_ms"]), incidence_clock_ms=stats(timed["incidence_clock_ms"]))
        print(name, json.dumps({k: v for k, v in out["variants"][name].items() if k != "rounds_ms"}), flush=True)
        if a.out:    # (written after every variant map: a later one that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    ens.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
