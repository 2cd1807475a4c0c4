"""Measurement of Ensemble.susceptibles (vgx_get_susceptibles) next to Ensemble.prevalence with as many classes on the same
ensemble and grid, in the protocol of tools/probe_prevalence.py.

Workload: --model (default c3_s5_p16: 16 populations, one susceptibility group, so P * G = 16 cells; p70: 70 populations, two
groups, 140 cells), R replicates x --events events each in one direct call with the event log, T = 100 grid points over
[0, the earliest final time among the first 64 replicates].  susceptibles() tracks every group as its own class; prevalence()
gets haplotype h % G, so both passes hold P * G cells.
In one process, ROUNDS times in alternation: susceptibles, prevalence, and an incidence call whose window lies behind every
event (it packs the clock inputs and counts nothing: the pack kernel alone, which every call runs first); with --alt KEY=VALUE
also susceptibles with that environment setting (a measurement build's switch between two forms of the counting kernel), set for
that call only.  Reported, median [min, max]: ms[0] (all kernels) and ms[1] (host clock) of every call; the counting + scan
kernels as ms[0] minus the pack kernel; the log bytes read (24 per event) over that time next to the HBM peak.
Before anything is timed, final is compared with replicate_state() and susceptibles + prevalence (every haplotype tracked) with
the population sizes for a few replicates.

    python tools/probe_susceptibles.py [--rounds 5] [--model p70 --replicates 1024 --events 20000] [--alt KEY=VALUE] [--out FILE.json]
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
    ap.add_argument("--model", default="c3_s5_p16")
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--alt", default=None, help="KEY=VALUE: an environment setting to time susceptibles() under as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    R = a.replicates
    with helpers.quiet():
        sim, phases = models.build(Simulator, a.model)
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    m = ens.model
    G = int(m.susNum)
    t_end = min(float(ens.replicate_state(r).currentTime) for r in range(min(R, 64)))
    window = (0.0, t_end)
    total = int(res.events.sum())
    behind = [t_end * 1e6, t_end * 2e6]
    variants = np.arange(m.hapNum) % G
    summary = dict(quantiles=(0.5,))
    alt = a.alt.split("=", 1) if a.alt else None

    def sus(env=None, values=False):
        if env:
            os.environ[env[0]] = env[1]
        try:
            return ens.susceptibles(points=a.points, window=window, summary=summary, values=values)
        finally:
            if env:
                del os.environ[env[0]]

    # before anything is timed: the final state, and nobody lost or made
    sv, pv = ens.susceptibles(points=a.points, window=window), ens.prevalence(points=a.points, window=window, replicates=[0, 1, R - 1])
    sizes = np.asarray(m.sizes, dtype=np.int64)
    for k, r in enumerate((0, 1, R - 1)):
        assert np.array_equal(sv.final[r], ens.replicate_state(r).susceptible), "final differs from the replicate's state"
        assert np.array_equal(sv.values[r].sum(axis=-1, dtype=np.int64) + pv.values[k].sum(axis=-1, dtype=np.int64),
                              np.broadcast_to(sizes, (a.points, m.popNum))), "susceptible + infectious is not the population size"
    if alt:
        other = sus(alt, values=True)
        assert np.array_equal(other.values, sv.values) and np.array_equal(other.final, sv.final), "the alternative form gives another block"
        del other
    del sv, pv
    ens.prevalence(points=a.points, window=window, variants=variants, summary=summary, values=False)   # warm-up
    ens.incidence(edges=behind)
    names = ["susceptibles", "prevalence", "pack_only"] + (["susceptibles_alt"] if alt else [])
    timed = {n + "_kernels_ms": [] for n in names}
    clock = {n: [] for n in ("susceptibles", "prevalence")}
    for rnd in range(a.rounds):
        s = sus()
        p = ens.prevalence(points=a.points, window=window, variants=variants, summary=summary, values=False)
        tb = ens.incidence(edges=behind).kernel_ms
        row = [s.kernel_ms, p.kernel_ms, tb] + ([sus(alt).kernel_ms] if alt else [])
        for n, v in zip(names, row):
            timed[n + "_kernels_ms"].append(v)
        clock["susceptibles"].append(s.clock_ms)
        clock["prevalence"].append(p.clock_ms)
        print("round", rnd, "  ".join("%s %.3f ms" % (n, v) for n, v in zip(names, row)), "(clocks %.1f / %.1f ms)" % (s.clock_ms, p.clock_ms), flush=True)
    pack = np.asarray(timed["pack_only_kernels_ms"])
    log_bytes = 24 * total
    out = {"workload": a.model, "replicates": R, "events_asked": a.events, "total_events": total, "points": a.points, "window": list(window),
           "rounds": a.rounds, "hbm_peak_TBs": HBM_PEAK_TBS, "kernel": ens.engine.last_kernel, "G": G, "cells": int(m.popNum * G), "passes": int(s.passes),
           "alt": a.alt, "log_bytes": log_bytes, "rounds_ms": timed,
           "susceptibles_clock_ms": stats(clock["susceptibles"]), "prevalence_clock_ms": stats(clock["prevalence"])}
    for n in names:
        if n == "pack_only":
            continue
        ms = np.asarray(timed[n + "_kernels_ms"]) - pack
        out[n + "_count_and_scan_ms"] = stats(ms)
        out[n + "_TBs"] = log_bytes / (float(np.median(ms)) * 1e-3) / 1e12 if np.median(ms) > 0 else None
    out["susceptibles_over_prevalence"] = stats((np.asarray(timed["susceptibles_kernels_ms"]) - pack) / (np.asarray(timed["prevalence_kernels_ms"]) - pack))
    if alt:
        out["alt_over_plain"] = stats((np.asarray(timed["susceptibles_alt_kernels_ms"]) - pack) / (np.asarray(timed["susceptibles_kernels_ms"]) - pack))
    ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
