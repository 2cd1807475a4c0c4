"""Measurement of scenario ensembles (vgx_set_param_sets) on the one-replicate-per-wavefront kernel.

Workload: c3_s5_p16, R replicates x N events each (sample_size unbounded, no event log), seeds 1000 .. 1000 + R - 1.  Runs, each
warmed up once and then timed ROUNDS times in alternation (a, b1, b64, b4096, a, ...), so that drift of the shared machine hits
all of them alike:
  (a)  the plain ensemble with kernel='wave': one shared parameter copy in the kernel arguments;
  (b)  the scenario form with G = 1, 64 and R copies of the same model as scenarios (G = 1 is vgx_set_params again: the plain path
       reached through the new entry; 64 and R pay the indirection, R also one table set per replicate);
  (c)  what a user does without scenarios: G = 64 separate Ensembles of R / 64 replicates each, run one after the other, with
       kernel='auto' (the engine's own choice at that size) and with kernel='wave' (like for like).
Every run simulates the same trajectories (same model, same seeds): the per-replicate event counts are compared, not assumed.
Reported per run: the kernel time (HIP events around the launch) and the wall time of simulate() (which also uploads parameters
and state) of every round, their medians, and the ratios (b)/(a) and (c)/(b64) per round with their range.

    python tools/probe_param_sets.py [--replicates 4096] [--events 100000] [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    def model():
        with helpers.quiet():
            sim, phases = models.build(Simulator, "c3_s5_p16")
            phases[0][0](sim)
        return sim

    R, N, split = a.replicates, a.events, 64
    assert R % split == 0
    seeds = 1000 + np.arange(R, dtype=np.int64)
    sim = model()
    runs = {"a_plain_wave": Ensemble(sim, R, seeds=seeds)}
    for G in (1, split, R):
        runs["b_sets_%d" % G] = Ensemble(sim, R, seeds=seeds, scenarios=[sim] * G)
    parts = [Ensemble(sim, R // split, seeds=seeds[g * (R // split):(g + 1) * (R // split)]) for g in range(split)]

    def one(ens, kernel):
        t = time.perf_counter()
        res = ens.simulate(N, sample_size=10 ** 12, record_events=False, kernel=kernel)
        return res.kernel_ms, time.perf_counter() - t, res.events.copy(), ens.engine.last_kernel

    def in_turn(kernel):
        ms, wall, ev, names = 0.0, 0.0, [], set()
        for ens in parts:
            k, w, e, name = one(ens, kernel)
            ms, wall = ms + k, wall + w
            ev.append(e)
            names.add(name)
        return ms, wall, np.concatenate(ev), "/".join(sorted(names))

    timed = {name: {"kernel_ms": [], "wall_s": []} for name in list(runs) + ["c_64_ensembles_auto", "c_64_ensembles_wave"]}
    events = None
    for rnd in range(-1, a.rounds):    # round -1: the warm-up of every shape (code objects, allocations), not recorded
        for name, ens in runs.items():
            k, w, ev, kern = one(ens, 'wave')
            assert kern == "wave"
            if events is None:
                events = ev
            assert np.array_equal(ev, events), name + ": other trajectories than the plain ensemble"
            if rnd >= 0:
                timed[name]["kernel_ms"].append(k)
                timed[name]["wall_s"].append(w)
        if rnd < a.split_rounds:
            for kernel in ("auto", "wave"):
                k, w, ev, kern = in_turn(kernel)
                assert np.array_equal(ev, events), "64 ensembles (%s): other trajectories than the plain ensemble" % kernel
                timed["c_64_ensembles_" + kernel]["kernel"] = kern
                if rnd >= 0:
                    timed["c_64_ensembles_" + kernel]["kernel_ms"].append(k)
                    timed["c_64_ensembles_" + kernel]["wall_s"].append(w)
        print("round", rnd, {n: (t["kernel_ms"][-1:] or None) for n, t in timed.items()}, flush=True)

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    def ratio(num, den, key):
        n = min(len(timed[num][key]), len(timed[den][key]))
        return stats(np.asarray(timed[num][key][:n]) / np.asarray(timed[den][key][:n]))   # round by round

    out = {"workload": "c3_s5_p16", "replicates": R, "events_per_replicate_asked": N, "total_events": int(events.sum()),
           "rounds": a.rounds, "split": split,
           "device_bytes": {name: int(ens.engine.device_bytes) for name, ens in runs.items()},
           "runs": {name: dict(t, kernel_ms_stats=stats(t["kernel_ms"]), wall_s_stats=stats(t["wall_s"]),
                               events_per_s_kernel=float(events.sum() / (np.median(t["kernel_ms"]) * 1e-3)))
                    for name, t in timed.items()},
           "ratios_kernel_ms": {"a_over_a_spread (max / min of a)": float(np.max(timed["a_plain_wave"]["kernel_ms"]) / np.min(timed["a_plain_wave"]["kernel_ms"]))},
           "ratios_wall_s": {}}
    for key, dst in (("kernel_ms", out["ratios_kernel_ms"]), ("wall_s", out["ratios_wall_s"])):
        for G in (1, split, R):
            dst["b%d_over_a" % G] = ratio("b_sets_%d" % G, "a_plain_wave", key)
        for kernel in ("auto", "wave"):
            dst["c_%s_over_b%d" % (kernel, split)] = ratio("c_64_ensembles_" + kernel, "b_sets_%d" % split, key)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    for ens in list(runs.values()) + parts:
        ens.close()


if __name__ == "__main__":
    main()
