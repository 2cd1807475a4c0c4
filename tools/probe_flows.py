"""Measurement of Ensemble.flows (vgx_get_flows): its two forms against each other and against the route a user had without it.

Workload: c3_s5_p16 (16 populations), one direct call with the event log, R = 4096 replicates x 10^5 events each (the shape of
DESIGN.md §14 and §16), T = 100 bins over [0, the earliest final time among the replicates of the host route), so that every
bin cuts through each of them.  Measured at V = 1 (one class: a table of 256 cells) and at V = 8 classes (haplotype h in class
h % 8: 2048 cells), where both forms fit.
Three routes to the same [n, T, P, P, V] block, compared bit for bit in an untimed warm-up round before anything is timed:
  dense    ens.flows(...) under VGX_FLOWS_FORM=dense: all P * P * V cells of a bin in LDS;
  split    ens.flows(...) under VGX_FLOWS_FORM=split: the diagonal in LDS, a record off it straight to device memory;
  host     ens.replicate_events(r) for every replicate (32 bytes per event to the host, one call each), then a numpy histogram
           (searchsorted + np.add.at): the route there is without flows().
The host route over all 4096 replicates would take minutes, so it runs over the first --host-replicates of them (the device
routes over the same subset are what the warm-up compares it with), and the routes are reported PER REPLICATE: a device route's
wall time over all R divided by R, the host route's over the subset divided by its size.  The routes are timed ROUNDS times in
alternation (dense, split, host, dense, ...).  Reported, median [min, max]: wall time of every route per replicate; split over
dense round by round, on wall time, on ms[0] (kernels) and on the counting kernel alone (ms[0] minus ms[0] of a call of the same
form whose window lies behind every event: that call packs the clock inputs and counts nothing); host over either device route;
the max / min spread of dense's own rounds, which is what a difference between the forms has to exceed.

    python tools/probe_flows.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FORMS = ("dense", "split")


def host_block(ens, reps, edges, P, vo, V):
    """The route without flows(): every replicate's chain to the host, then numpy."""
    T = len(edges) - 1
    out = np.zeros((len(reps), T, P, P, V), dtype=np.int32)
    vo = vo.astype(np.int64)
    for i, r in enumerate(reps):
        ev = ens.replicate_events(int(r))
        b = np.searchsorted(edges, ev[0], side='right') - 1
        typ, hap, pop, npop = ev[1].astype(np.int64), ev[2].astype(np.int64), ev[3].astype(np.int64), ev[5].astype(np.int64)
        ok = (b >= 0) & (b < T) & ((typ == 0) | (typ == 5))
        cls = np.where(ok, vo[np.where(ok, hap, 0)], -1)
        ok &= cls >= 0
        dst = np.where(typ == 5, npop, pop)
        np.add.at(out[i], (b[ok], pop[ok], dst[ok], cls[ok]), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--host-replicates", type=int, default=64)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--classes", type=int, nargs="+", default=[1, 8])
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
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    t = time.perf_counter()
    with helpers.quiet():
        res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    sim_s = time.perf_counter() - t
    P, H = ens.model.popNum, ens.model.hapNum
    sub = np.arange(min(R, a.host_replicates), dtype=np.int64)
    t_end = min(float(ens.replicate_state(int(r)).currentTime) for r in sub)
    window = (0.0, t_end)
    behind = [t_end * 1e6, t_end * 2e6]
    total = int(res.events.sum())
    out = {"workload": "c3_s5_p16", "bins": a.bins, "rounds": a.rounds, "replicates": R, "events_asked": a.events, "total_events": total,
           "longest_chain": int(res.events.max()), "kernel": ens.engine.last_kernel, "simulate_wall_s": sim_s, "window": list(window),
           "host_route_replicates": len(sub), "classes": {}}

    for V in a.classes:
        vo = (np.arange(H, dtype=np.int64) % V).astype(np.int32)

        def device(form, reps=None, edges=None):
            os.environ["VGX_FLOWS_FORM"] = form
            t = time.perf_counter()
            fl = ens.flows(variants=vo, replicates=reps, **(dict(bins=a.bins, window=window) if edges is None else dict(edges=edges)))
            dt = time.perf_counter() - t
            assert fl.form == form
            return dt, fl

        def host(edges):
            t = time.perf_counter()
            block = host_block(ens, sub, edges, P, vo, V)
            return time.perf_counter() - t, block

        # warm-up of all routes and the comparison of their results (untimed)
        _, fd = device("dense", sub)
        _, fs = device("split", sub)
        edges = fd.edges
        _, block = host(edges)
        assert np.array_equal(fd.counts, block) and np.array_equal(fs.counts, block), "device and host route differ"
        assert block.sum() - np.einsum('rbppc->', block) > 0, "no transmission across populations in the window"
        _, fd = device("dense")
        _, fs = device("split")
        assert np.array_equal(fd.counts, fs.counts), "the forms differ"
        in_window, across = int(total - fd.outside.sum()), int(fd.counts.sum(dtype=np.int64) - np.einsum('rbppc->', fd.counts, dtype=np.int64))
        counted, block_bytes = int(fd.counts.sum(dtype=np.int64)), int(fd.counts.nbytes)
        del fd, fs
        for form in FORMS:
            assert not device(form, edges=behind)[1].counts.any()
        timed = {"%s_%s" % (f, k): [] for f in FORMS for k in ("wall_s", "kernels_ms", "clock_ms", "library_ms", "pack_only_ms")}
        timed["host_wall_s"] = []
        for rnd in range(a.rounds):
            line = []
            for form in FORMS:
                td, fl = device(form)
                tb = device(form, edges=behind)[1].kernel_ms
                for k, v in (("wall_s", td), ("kernels_ms", fl.kernel_ms), ("clock_ms", fl.clock_ms), ("library_ms", fl.wall_ms), ("pack_only_ms", tb)):
                    timed["%s_%s" % (form, k)].append(v)
                line.append("%s %.4f s (kernels %.3f ms, pack alone %.3f ms, clock %.1f ms)" % (form, td, fl.kernel_ms, tb, fl.clock_ms))
                del fl
            th, _ = host(edges)
            timed["host_wall_s"].append(th)
            print("V = %d round %d over %d replicates: %s; host %.4f s over %d" % (V, rnd, R, "; ".join(line), th, len(sub)), flush=True)
        arr = {k: np.asarray(v) for k, v in timed.items()}
        count = {f: arr[f + "_kernels_ms"] - arr[f + "_pack_only_ms"] for f in FORMS}
        host_per = arr["host_wall_s"] / len(sub)
        spread = float(arr["dense_wall_s"].max() / arr["dense_wall_s"].min())
        ratio_wall = arr["split_wall_s"] / arr["dense_wall_s"]
        out["classes"][str(V)] = dict(
            V=V, lds_bytes={"dense": 4 * P * P * V, "split": 4 * P * V}, block_bytes=block_bytes, events_in_window=in_window,
            new_infections_counted=counted, of_them_across=across, rounds=timed,
            dense_wall_s_per_replicate=stats(arr["dense_wall_s"] / R), split_wall_s_per_replicate=stats(arr["split_wall_s"] / R),
            host_wall_s_per_replicate=stats(host_per),
            host_over_dense_per_replicate=stats(host_per / (arr["dense_wall_s"] / R)), host_over_split_per_replicate=stats(host_per / (arr["split_wall_s"] / R)),
            split_over_dense_wall=stats(ratio_wall), split_over_dense_kernels=stats(arr["split_kernels_ms"] / arr["dense_kernels_ms"]),
            split_over_dense_count_kernel=stats(count["split"] / count["dense"]),
            dense_wall_spread_max_over_min=spread, dense_count_kernel_spread_max_over_min=float(count["dense"].max() / count["dense"].min()),
            split_faster_beyond_dense_spread=bool(np.median(ratio_wall) < 1.0 / spread),
            dense_kernels_ms=stats(arr["dense_kernels_ms"]), split_kernels_ms=stats(arr["split_kernels_ms"]),
            dense_count_kernel_ms=stats(count["dense"]), split_count_kernel_ms=stats(count["split"]),
            dense_clock_ms=stats(arr["dense_clock_ms"]), split_clock_ms=stats(arr["split_clock_ms"]),
            dense_library_ms=stats(arr["dense_library_ms"]), split_library_ms=stats(arr["split_library_ms"]))
        print("V = %d" % V, json.dumps({k: v for k, v in out["classes"][str(V)].items() if k != "rounds"}), flush=True)
        if a.out:    # (written after every V: a later one that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    os.environ.pop("VGX_FLOWS_FORM", None)
    ens.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
