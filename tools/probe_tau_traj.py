"""Development aid: what summary trajectories cost the tau paths.  The same seeds with traj_points=0 and traj_points=1001 (a grid over
the span of the call), in interleaved runs; one JSON line per run, then the medians.

  small: the on-device step loop (vgx_taus.hip) on bench's tau_small shapes (16x3 at 2048 replicates, 256x5 at 512; 1000 steps per
         replicate after a 2000-event direct warm-up): steps/s of device time.
  c4:    the step kernels (vgx_tau.hip) on BASELINE config 4 (2^20 haplotypes x 256 populations, 3 hosts per compartment, one replicate,
         start state staged by vgx_stage_tau as bench's tau leg does): device ms per step.

    python tools/probe_tau_traj.py [--only small|c4] [--runs 3] [--points 0,1001] [--window T0,T1]

--window: config 4's grid without the first (untimed) call that finds the span of the steps (for a profiler run of the timed calls alone)."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def small_cases(runs, points):
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    out = {}
    for name, sites, pops, reps in (("16x3", 2, 3, 2048), ("256x5", 4, 5, 512)):
        with contextlib.redirect_stdout(io.StringIO()):
            s = Simulator(number_of_sites=sites, populations_number=pops, seed=7)
        s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.05)
        s.set_total_migration_probability(0.002); s.set_population_size(10 ** 6)
        with contextlib.redirect_stdout(io.StringIO()):
            s.simulate(2000, sample_size=10 ** 12)
        ens = Ensemble(s, reps)
        seeds = 7 + np.arange(reps, dtype=np.int64)
        ens.simulate_tau(1000, sample_size=10 ** 15, seeds=seeds)       # allocations; the span of the call for the grid
        t0 = float(s.simulation.currentTime)
        t1 = max(float(ens.replicate_state(r).currentTime) for r in range(0, reps, max(1, reps // 64)))
        rows = {T: [] for T in points}
        for i in range(runs):
            for T in points:
                res = ens.simulate_tau(1000, sample_size=10 ** 15, seeds=seeds, traj_points=T, traj_window=(t0, t1))
                rate = float(res.loop_iterations.sum()) / (res.kernel_ms * 1e-3)
                rows[T].append(rate)
                print(json.dumps({"case": name, "replicates": reps, "traj_points": T, "run": i, "steps": int(res.loop_iterations.sum()),
                                  "kernel_ms": res.kernel_ms, "steps_per_s": rate}), flush=True)
        ens.close()
        out[name] = {T: statistics.median(v) for T, v in rows.items()}
    return out


def c4_case(runs, points, window=None, steps=20):
    from vgsim_amd import Simulator, _capi
    with contextlib.redirect_stdout(io.StringIO()):
        s = Simulator(number_of_sites=10, populations_number=256, seed=2020)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.01)
    s.set_total_migration_probability(0.01); s.set_population_size(10 ** 7)
    m = s.simulation
    m.infectious[:] = 3
    m.susceptible[:, 0] -= 3 * m.hapNum
    eng = _capi.HipEngine(m.sites, m.hapNum, m.popNum, m.susNum, n_replicates=1)
    m.events.CreateEvents(steps)
    m.events.ptr = 1            # not the first call of the model: capacity = ptr + iterations (events.pxi:61-68)
    m.events.CreateEvents(steps)
    eng.set_params(m); eng.set_seeds(np.array([2020], dtype=np.int64))

    def call(T, window):
        eng.set_state(m)
        eng.stage_tau()
        o = _capi.VgxRunOpts(); o.record_events = 0
        o.traj_points = T
        o.traj_t0, o.traj_t1 = window
        eng._check(eng.lib.vgx_simulate_tau(eng.handle, steps, 10 ** 15, -1.0, 1, C.byref(o)))
        c = eng.counters(0)
        return c, eng.last_kernel_ms, eng.lib.vgx_last_kernel_launches(eng.handle)

    if window is None:
        c, _, _ = call(0, (0.0, 1.0))                           # allocations; the times of the steps for the grid
        n = int(c.ev_ptr - c.ev_first_new)
        times = np.zeros(n, dtype=np.float64)
        eng._check(eng.lib.vgx_get_events(eng.handle, 0, c.ev_first_new, n, times.ctypes.data_as(C.POINTER(C.c_double)),
                                          None, None, None, None, None))
        window = (0.0, float(times[-1]))
    print(json.dumps({"case": "config4", "window": list(window)}), flush=True)
    rows = {T: [] for T in points}
    for i in range(runs):
        for T in points:
            c, ms, launches = call(T, window)
            k = max(int(c.loop_iterations), 1)
            rows[T].append(ms / k)
            print(json.dumps({"case": "config4", "traj_points": T, "run": i, "steps": k, "kernel_ms": ms, "ms_per_step": ms / k,
                              "launches": int(launches)}), flush=True)
    eng.close()
    return {"config4": {T: statistics.median(v) for T, v in rows.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("small", "c4"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", default="0,1001")
    ap.add_argument("--window")
    a = ap.parse_args()
    points = [int(x) for x in a.points.split(",")]
    med = {}
    if a.only in (None, "small"):
        med.update(small_cases(a.runs, points))
    if a.only in (None, "c4"):
        med.update(c4_case(a.runs, points, tuple(float(x) for x in a.window.split(",")) if a.window else None))
    print(json.dumps({"medians": med}), flush=True)


if __name__ == "__main__":
    main()
