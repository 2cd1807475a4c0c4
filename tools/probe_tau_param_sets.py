"""Measurement of simulate_tau on a scenario ensemble (vgx_simulate_tau after vgx_set_param_sets) against what a user had without it.

Model: the small-model ensemble of bench.py's tau_small leg and of tools/probe_tau_incidence.py (16 haplotypes x 3 populations, 10^6
hosts per population, a 2000-event direct warm-up as the common start state), G = 4 parameter sets (the model itself, a faster
variant, another NPI setting, a higher mutation rate), 2048 replicates, --steps tau steps on the device step loop.
Two routes to the same 2048 final states, compared bit for bit (compartments, counters, times) in an untimed warm-up round:
  scenario   ONE ensemble of 2048 replicates, 512 per set: one simulate_tau(per_scenario=True) call, one launch;
  one-set    FOUR ensembles of 512 replicates, one per set: four simulate_tau calls (what the parent commit offers).
The ensembles exist before anything is timed.  Each route is timed ROUNDS times in alternation.  Reported, median [min, max]: wall
time of either route's calls, the time of their kernels, and the ratio round by round.

    python tools/probe_tau_param_sets.py [--rounds 5] [--out FILE.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def models():
    """The warmed base model and the four scenarios (copies of it: parameters and state)."""
    from oracle import oracle
    from vgsim_amd import Simulator
    oracle.build()
    s = Simulator(number_of_sites=2, populations_number=3, seed=7)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.05)
    s.set_total_migration_probability(0.002); s.set_population_size(10 ** 6)
    s.set_npi([0.3, 0.05, 0.01])
    assert oracle.run_direct(s.simulation, 2000, 10 ** 12, -1, 200) == 0     # (on the CPU oracle: the model then holds no engine and can be copied)
    a, b, c, d = (copy.deepcopy(s) for _ in range(4))
    b.set_transmission_rate(3.2, haplotype=5)
    c.set_npi([0.1, 0.01, 0.002])
    d.set_mutation_rate(0.2)
    return s, [a, b, c, d]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    from vgsim_amd.ensemble import Ensemble

    os.environ["VGX_TAU_STEP_KERNELS"] = "0"
    G, R = 4, a.replicates
    per = R // G
    assert per * G == R
    with helpers.quiet():
        base, scen = models()
    seeds = 1000 + np.arange(R, dtype=np.int64)
    scenario_of = np.repeat(np.arange(G), per)
    whole = Ensemble(base, R, seeds=seeds, scenarios=scen, scenario_of=scenario_of)
    parts = [Ensemble(scen[g], per, seeds=seeds[g * per:(g + 1) * per]) for g in range(G)]

    def scenario_route():
        t = time.perf_counter()
        res = whole.simulate_tau(a.steps, sample_size=10 ** 15, per_scenario=True)
        return time.perf_counter() - t, res.kernel_ms

    def one_set_route():
        t, k = time.perf_counter(), 0.0
        for e in parts:
            k += e.simulate_tau(a.steps, sample_size=10 ** 15).kernel_ms
        return time.perf_counter() - t, k

    # warm-up of both routes and the comparison of their results (untimed)
    scenario_route()
    one_set_route()
    got = whole.replicate_states_tau()
    steps_all = 0
    for g, e in enumerate(parts):
        want = e.replicate_states_tau()
        for x, y in zip(got, want):
            assert np.array_equal(x[g * per:(g + 1) * per], y), "scenario run and one-set run differ (set %d)" % g
        steps_all += int(want[2][:, 7].sum()) - per * int(base.simulation.events.ptr)

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    timed = {"scenario_wall_s": [], "one_set_wall_s": [], "scenario_kernel_ms": [], "one_set_kernels_ms": []}
    for rnd in range(a.rounds):
        ts, ks = scenario_route()
        to, ko = one_set_route()
        for k, v in (("scenario_wall_s", ts), ("one_set_wall_s", to), ("scenario_kernel_ms", ks), ("one_set_kernels_ms", ko)):
            timed[k].append(v)
        print("round", rnd, "scenario %.4f s (kernel %.2f ms)   four one-set calls %.4f s (kernels %.2f ms)" % (ts, ks, to, ko), flush=True)
    m = base.simulation
    out = dict(haplotypes=int(m.hapNum), populations=int(m.popNum), replicates=R, sets=G, replicates_per_set=per, tau_steps=a.steps,
               steps_of_all_replicates=steps_all, rounds=timed,
               scenario_wall_s=stats(timed["scenario_wall_s"]), one_set_wall_s=stats(timed["one_set_wall_s"]),
               scenario_kernel_ms=stats(timed["scenario_kernel_ms"]), one_set_kernels_ms=stats(timed["one_set_kernels_ms"]),
               one_set_over_scenario_wall=stats(np.asarray(timed["one_set_wall_s"]) / np.asarray(timed["scenario_wall_s"])),
               one_set_over_scenario_kernels=stats(np.asarray(timed["one_set_kernels_ms"]) / np.asarray(timed["scenario_kernel_ms"])),
               scenario_spread_max_over_min=float(np.max(timed["scenario_wall_s"]) / np.min(timed["scenario_wall_s"])),
               one_set_spread_max_over_min=float(np.max(timed["one_set_wall_s"]) / np.min(timed["one_set_wall_s"])))
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    whole.close()
    for e in parts:
        e.close()


if __name__ == "__main__":
    main()
