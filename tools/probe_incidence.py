"""Measurement of Ensemble.incidence (vgx_get_incidence) against the route a user had without it.

Workload: c3_s5_p16 (16 populations), one direct call with the event log, T = 100 bins over [0, the earliest final time among the
replicates of the host route), so that every bin cuts through each of them (--window latest: up to the latest one, so that
nearly every event lies inside the window).
Shapes:
  ensemble   R = 4096 replicates x 10^5 events each (the shape of DESIGN.md §14);
  single     one replicate, as many events as --single-events asks for (10^7) or the run gives: a chain whose tiles are the only
             parallelism there is.
Two routes to the same [n, T, P, 7] block, compared bit for bit in an untimed warm-up round before anything is timed:
  device   ens.incidence(bins=T, window=...): the log stays on the device;
  host     ens.replicate_events(r) for every replicate (32 bytes per event to the host, one call each), then a numpy histogram
           (searchsorted + np.add.at per channel).
The host route over all 4096 replicates would take minutes, so it runs over the first --host-replicates of them (the device
route over the same subset is what the warm-up compares it with), and both routes are reported PER REPLICATE: the device route's
wall time over all R divided by R, the host route's over the subset divided by its size.  Each route is timed ROUNDS times in
alternation (device, host, device, ...).  Reported, median [min, max]: wall time of either route per replicate and their ratio round
by round; ms[0] (kernels) and ms[1] (host clock) of the device route; the counting kernel alone (ms[0] minus ms[0] of a call whose
window lies behind every event: that call packs the clock inputs and counts nothing) and the log bytes it reads (24 per event
INSIDE the window: tiles outside it are skipped) over that time next to the HBM peak.

    python tools/probe_incidence.py [--rounds 5] [--out FILE.json]
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


def host_block(ens, reps, edges, P):
    """The route without incidence(): every replicate's chain to the host, then numpy."""
    T = len(edges) - 1
    out = np.zeros((len(reps), T, P, 7), dtype=np.int32)
    for i, r in enumerate(reps):
        ev = ens.replicate_events(int(r))
        b = np.searchsorted(edges, ev[0], side='right') - 1
        typ, pop, npop = ev[1].astype(np.int64), ev[3].astype(np.int64), ev[5].astype(np.int64)
        ok = (b >= 0) & (b < T)
        plain = ok & (typ < 5)
        np.add.at(out[i], (b[plain], pop[plain], typ[plain]), 1)
        mig = ok & (typ == 5)
        np.add.at(out[i], (b[mig], npop[mig], 5), 1)
        np.add.at(out[i], (b[mig], pop[mig], 6), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--single-events", type=int, default=10 ** 7)
    ap.add_argument("--host-replicates", type=int, default=64)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--window", choices=("earliest", "latest"), default="earliest")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    out = {"workload": "c3_s5_p16", "bins": a.bins, "window_end": a.window, "rounds": a.rounds, "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    for name, R, events in (("ensemble", a.replicates, a.events), ("single", 1, a.single_events)):
        with helpers.quiet():
            sim, phases = models.build(Simulator, "c3_s5_p16")
            phases[0][0](sim)
        ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
        t = time.perf_counter()
        with helpers.quiet():
            res = ens.simulate(events, sample_size=10 ** 12, record_events=True)
        sim_s = time.perf_counter() - t
        P = ens.model.popNum
        sub = np.arange(min(R, a.host_replicates), dtype=np.int64)
        t_end = (min if a.window == 'earliest' else max)(float(ens.replicate_state(int(r)).currentTime) for r in sub)
        window = (0.0, t_end)
        total = int(res.events.sum())

        def device(reps=None):
            t = time.perf_counter()
            inc = ens.incidence(bins=a.bins, window=window, replicates=reps)
            return time.perf_counter() - t, inc

        def host():
            t = time.perf_counter()
            block = host_block(ens, sub, edges, P)
            return time.perf_counter() - t, block

        # warm-up of both routes and the comparison of their results (untimed)
        _, inc = device(sub)
        edges = inc.edges
        _, block = host()
        assert np.array_equal(inc.counts, block), "device and host route differ"
        device()
        behind = ens.incidence(edges=[t_end * 1e6, t_end * 2e6])    # nothing to count: the pack kernel alone
        assert not behind.counts.any()
        timed = {"device_wall_s": [], "host_wall_s": [], "kernels_ms": [], "clock_ms": [], "library_ms": [], "pack_only_ms": []}
        for rnd in range(a.rounds):
            td, inc = device()
            th, _ = host()
            tb = ens.incidence(edges=[t_end * 1e6, t_end * 2e6]).kernel_ms
            timed["device_wall_s"].append(td)
            timed["host_wall_s"].append(th)
            timed["kernels_ms"].append(inc.kernel_ms)
            timed["clock_ms"].append(inc.clock_ms)
            timed["library_ms"].append(inc.wall_ms)
            timed["pack_only_ms"].append(tb)
            print(name, "round", rnd, "device %.4f s over %d replicates (kernels %.3f ms, pack alone %.3f ms, clock %.1f ms)  host %.4f s over %d"
                  % (td, R, inc.kernel_ms, tb, inc.clock_ms, th, len(sub)), flush=True)
        dev_per = np.asarray(timed["device_wall_s"]) / R
        host_per = np.asarray(timed["host_wall_s"]) / len(sub)
        count_ms = np.asarray(timed["kernels_ms"]) - np.asarray(timed["pack_only_ms"])
        in_window = int(total - inc.outside.sum())
        log_bytes = 24 * in_window    # (the kernel reads the records inside the window only)
        c_med = float(np.median(count_ms))
        out["shapes"][name] = dict(
            replicates=R, events_asked=events, total_events=total, longest_chain=int(res.events.max()), kernel=ens.engine.last_kernel,
            simulate_wall_s=sim_s, window=list(window), host_route_replicates=len(sub), passes=inc.passes,
            block_bytes=int(inc.counts.nbytes), events_in_window=in_window, rounds=timed,
            device_wall_s=stats(timed["device_wall_s"]), device_wall_s_per_replicate=stats(dev_per),
            host_wall_s_per_replicate=stats(host_per), host_over_device_per_replicate=stats(host_per / dev_per),
            device_spread_max_over_min=float(np.max(timed["device_wall_s"]) / np.min(timed["device_wall_s"])),
            kernels_ms=stats(timed["kernels_ms"]), clock_ms=stats(timed["clock_ms"]), library_ms=stats(timed["library_ms"]),
            count_kernel_ms=stats(count_ms), log_bytes=log_bytes,
            count_kernel_TBs=log_bytes / (c_med * 1e-3) / 1e12 if c_med > 0 else None,
            count_kernel_share_of_hbm_peak=log_bytes / (c_med * 1e-3) / 1e12 / HBM_PEAK_TBS if c_med > 0 else None)
        print(name, json.dumps({k: v for k, v in out["shapes"][name].items() if k != "rounds"}), flush=True)
        ens.close()
        if a.out:    # (written after every shape: a later shape that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
