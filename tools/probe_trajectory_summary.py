"""Measurement of Ensemble.trajectory_summary (vgx_get_trajectory_summary) against the route a user had without it.

Workload: c3_s5_p16 (16 populations), traj_points=101, so a replicate's trajectories are N = 101 * 16 * 2 = 3232 columns.  Shapes:
  scenarios   R = 4096 replicates as 64 scenarios of 64 (the scenario probe's ensemble): 64 groups, the wavefront form;
  one_group   R = 16384 replicates of a plain ensemble: one group of 16384, the workgroup form at its documented maximum.
After one simulate(traj_points=101) call per shape, two routes to the same quantiles (0.025, 0.5, 0.975, method 'lower': exact on
both routes, compared bit for bit before anything is timed), with min, max and mean:
  device   ens.trajectory_summary(): the block stays on the device;
  host     ens.trajectories() to the host, then per group np.sort down the replicates and the same ranks, min, max, mean.
Each route is warmed up once and then timed ROUNDS times in alternation (device, host, device, ...).  Reported per shape: the wall
time of either route per round, median [min, max], their ratio round by round, the device time of the kernels alone
(TrajectorySummary.kernel_ms) and the bytes the kernels move (8 read + 4 written by the transpose, 4 read by the sort, per member
and column) over that time, next to the HBM peak.

    python tools/probe_trajectory_summary.py [--rounds 5] [--events 20000] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK_TBS = 8.0    # MI355X, specification
Q = (0.025, 0.5, 0.975)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--events", type=int, default=20000)
    ap.add_argument("--points", type=int, default=101)
    ap.add_argument("--shapes", default="scenarios:4096:64,one_group:16384:1", help="name:replicates:groups, comma-separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble, _summary_ranks

    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    out = {"workload": "c3_s5_p16", "traj_points": a.points, "events_per_replicate_asked": a.events, "rounds": a.rounds,
           "quantiles": list(Q), "method": "lower", "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    for spec in a.shapes.split(","):
        name, R, G = spec.split(":")
        R, G = int(R), int(G)
        seeds = 1000 + np.arange(R, dtype=np.int64)
        ens = Ensemble(sim, R, seeds=seeds, scenarios=[sim] * G if G > 1 else None)
        # the window: up to the earliest final time of a first, short look (so that every grid point cuts through every replicate)
        ens.simulate(a.events, sample_size=10 ** 12)
        t_end = min(float(ens.replicate_state(r).currentTime) for r in range(0, R, max(R // 16, 1)))
        res = ens.simulate(a.events, sample_size=10 ** 12, traj_points=a.points, traj_window=(0.0, t_end))
        group_of = ens.scenario_of.astype(np.int64) if G > 1 else np.zeros(R, dtype=np.int64)
        members = [np.nonzero(group_of == g)[0] for g in range(G)]
        ranks = [_summary_ranks(Q, len(m), 'lower') for m in members]

        def device():
            t = time.perf_counter()
            s = ens.trajectory_summary(quantiles=Q, method='lower')
            return time.perf_counter() - t, s

        def host():
            t = time.perf_counter()
            traj = ens.trajectories()
            quant, lo, hi, mean = [], [], [], []
            for m, rk in zip(members, ranks):
                srt = np.sort(traj[m], axis=0)
                quant.append(srt[rk])
                lo.append(srt[0])
                hi.append(srt[-1])
                mean.append(srt.sum(axis=0) / len(m))
            return time.perf_counter() - t, (np.stack(quant), np.stack(lo), np.stack(hi), np.stack(mean))

        timed = {"device_wall_s": [], "host_wall_s": [], "device_kernel_ms": [], "device_copy_ms": [], "device_library_ms": []}
        for rnd in range(-1, a.rounds):    # round -1: warm-up of both routes and the comparison of their results
            td, s = device()
            th, (quant, lo, hi, mean) = host()
            if rnd < 0:
                assert np.array_equal(s.quantiles, quant) and np.array_equal(s.min, lo) and np.array_equal(s.max, hi)
                assert np.array_equal(s.mean, mean)    # (sums of whole numbers below 2^53: exact in float64 in any order)
                continue
            timed["device_wall_s"].append(td)
            timed["host_wall_s"].append(th)
            timed["device_kernel_ms"].append(s.kernel_ms)
            timed["device_copy_ms"].append(s.copy_ms)
            timed["device_library_ms"].append(s.wall_ms)
            print(name, "round", rnd, "device %.4f s (kernels %.3f ms)  host %.4f s" % (td, s.kernel_ms, th), flush=True)
        N = a.points * ens.model.popNum * 2
        kernel_bytes = 16 * R * N
        k_med = float(np.median(timed["device_kernel_ms"]))
        out["shapes"][name] = dict(
            replicates=R, groups=G, columns=N, block_bytes=8 * R * N, simulate_kernel_ms=res.kernel_ms, passes=s.passes,
            rounds=timed, device_wall_s=stats(timed["device_wall_s"]), host_wall_s=stats(timed["host_wall_s"]),
            host_over_device=stats(np.asarray(timed["host_wall_s"]) / np.asarray(timed["device_wall_s"])),
            device_kernel_ms=stats(timed["device_kernel_ms"]), kernel_bytes=kernel_bytes,
            kernel_TBs=kernel_bytes / (k_med * 1e-3) / 1e12, kernel_share_of_hbm_peak=kernel_bytes / (k_med * 1e-3) / 1e12 / HBM_PEAK_TBS)
        ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
