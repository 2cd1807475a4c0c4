"""Measurement of Ensemble.tau_lineages (vgx_get_tau_lineages) next to Ensemble.tau_genealogies on the same ensembles.

Workloads: the probe ensembles of tools/probe_ensemble_tau_genealogies.py, 2048 replicates of tau_b (2000 direct events of warm-up,
then 200 tau steps) and 512 of tau_d (30000 direct events, then 40 steps), with the event log; T = 100 grid points from before the
model's first event to after every replicate's last step, four variant classes.  Per workload, in one process, ROUNDS times in
alternation: tau_genealogies(seed) and tau_lineages(seed) with the values copied to the host.  Reported per round and as median [min, max]: the
canonicalise, walk, binning and suffix-sum kernels of tau_lineages() apart (Lineages.stage_ms), its host cuts, its host part (whole
call minus kernels) and the whole call; and the device time of tau_genealogies() (GenealogyBatch.kernel_ms: its canonicalise and walk
kernels together, which is all that call reports), to be read against the canonicalise plus walk kernels of tau_lineages().  Before
anything is timed status and generator are compared with tau_genealogies() and a few rows with the host replay of the rule.

The tau walk header changed when tau_lineages() was added (an observer template parameter whose default does nothing), so the same
figure of tau_genealogies() is wanted from the library of the commit before, in the same session: --parent-library PATH runs this
tool again in a fresh process per workload on that library (--genealogies-only: it then calls nothing that library lacks).  The
findings reported are whether the difference of two medians exceeds the run-to-run spread (max - min) observed in either series.

    python tools/probe_tau_lineages.py [--rounds 5] [--parent-library OLD/libvgx.so] [--out profiles/tau_lineages.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
WORKLOADS = (("tau_b", 2048), ("tau_d", 512))
NEW_SYMBOLS = ("vgx_get_tau_lineages", "vgx_test_tau_lineages")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v), "rounds": [float(x) for x in v]}


def versus(a, b):
    """Two series of timings: the difference of the medians against the largest run-to-run spread of either."""
    diff = b["median"] - a["median"]
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return {"median_difference_ms": diff, "largest_run_to_run_spread_ms": spread, "difference_exceeds_spread": bool(abs(diff) > spread)}


def ensemble(case, R):
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, case)
        phases[0][0](sim)
        sim.simulate(**phases[0][1])
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(phases[1][1]["iterations"], sample_size=10 ** 12, record_events=True)
    return ens


def genealogies_only(case, R, rounds, seed):
    ens = ensemble(case, R)
    ens.tau_genealogies(seed=seed, replicates=np.arange(min(R, 64)))   # warm-up (code objects, allocator)
    ms = [ens.tau_genealogies(seed=seed).kernel_ms for _ in range(rounds)]
    ens.close()
    return stats(ms)


def workload(case, R, a):
    from vgsim_amd import _capi
    ens = ensemble(case, R)
    m = ens.model
    steps_end = ens.replicate_states_tau()[3]
    t0 = float(m.events.times[0]) if m.events.ptr else 0.0
    window = (t0 - 1e-3, float(steps_end.max()) * 1.001 + 1e-3)
    variants = (np.arange(m.hapNum) % 4).astype(np.int64)
    V = int(variants.max()) + 1
    ln = ens.tau_lineages(points=a.points, window=window, variants=variants, seed=a.seed)   # warm-up, and the check
    b = ens.tau_genealogies(seed=a.seed)
    assert np.array_equal(ln.status, b.status) and np.array_equal(ln.rng_raw, b.rng_raw), "the walk differs from that of tau_genealogies()"
    for r in (0, 1, R - 1):
        if ln.ok[r]:
            want = _capi.replay_tau_lineages(ens._tau_chain_model(r), a.seed, ln.times, ln.variant_of, V, rng_position=(0, 0))
            assert np.array_equal(ln.values[r], want["values"]) and np.array_equal(ln.root[r], want["root"]), "row %d differs from the host replay" % r
    keys = ("canonicalise_ms", "walk_ms", "binning_ms", "scan_ms", "kernels_ms", "host_cuts_ms", "host_part_ms", "call_ms")
    timed = {k: [] for k in keys}
    gen_ms = []
    for rnd in range(a.rounds):
        b = ens.tau_genealogies(seed=a.seed)
        ln = ens.tau_lineages(points=a.points, window=window, variants=variants, seed=a.seed)   # (no summary: some walks of these ensembles fail)
        gen_ms.append(b.kernel_ms)
        for k, v in zip(keys, tuple(ln.stage_ms) + (ln.kernel_ms, ln.clock_ms, ln.wall_ms - ln.kernel_ms, ln.wall_ms)):
            timed[k].append(v)
        print(case, "round", rnd, "tau_genealogies kernels %.3f ms;  tau_lineages canonicalise %.3f, walk %.3f, binning %.3f, scan %.3f ms (cuts %.2f ms, call %.2f ms)"
              % ((b.kernel_ms,) + tuple(ln.stage_ms) + (ln.clock_ms, ln.wall_ms)), flush=True)
    out = {"workload": case, "replicates": R, "prefix_events": int(m.events.ptr), "points": a.points, "window": list(window), "classes": V,
           "cells": int(m.popNum) * V, "passes": ln.passes, "healthy_walks": int(ln.ok.sum()), "lineage_records": int(ln.records.sum()),
           "tau_genealogies_kernels_ms": stats(gen_ms), "tau_lineages": {k: stats(v) for k, v in timed.items()}}
    both = [c + w for c, w in zip(timed["canonicalise_ms"], timed["walk_ms"])]
    out["tau_lineages"]["canonicalise_plus_walk_ms"] = stats(both)
    # expectation 2: the lineage walk is not slower than the genealogy walk (both sides: canonicalise + walk)
    out["lineages_vs_genealogies_canonicalise_plus_walk"] = versus(out["tau_genealogies_kernels_ms"], out["tau_lineages"]["canonicalise_plus_walk_ms"])
    ens.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--parent-library", default=None, help="libvgx.so of the commit before")
    ap.add_argument("--genealogies-only", default=None, metavar="CASE:R", help="(the child run on another library)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.genealogies_only:
        from vgsim_amd import _capi
        lib = ctypes.CDLL(_capi.LIB_PATH)
        for name in NEW_SYMBOLS:   # a library of the commit before lacks them: bind what it has
            if not hasattr(lib, name):
                _capi.SIGNATURES.pop(name, None)
        case, R = a.genealogies_only.split(":")
        print("RESULT " + json.dumps(genealogies_only(case, int(R), a.rounds, a.seed)), flush=True)
        return
    out = {"rounds": a.rounds, "workloads": []}
    for case, R in WORKLOADS:
        w = workload(case, R, a)
        if a.parent_library:   # expectation 1: tau_genealogies' kernels are the same on both libraries
            env = dict(os.environ, VGX_LIBRARY=os.path.abspath(a.parent_library))
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--genealogies-only", "%s:%d" % (case, R), "--rounds", str(a.rounds),
                                  "--seed", str(a.seed)], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            parent = json.loads([line for line in txt.splitlines() if line.startswith("RESULT ")][-1][7:])
            w["tau_genealogies_kernels_parent_library_ms"] = parent
            w["tau_genealogies_parent_vs_this_library"] = versus(parent, w["tau_genealogies_kernels_ms"])
        out["workloads"].append(w)
    out["not_measured"] = ["other grids", "class counts near the LDS limit", "steps near 8192 raw rows"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
