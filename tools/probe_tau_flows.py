"""Measurement of Ensemble.tau_flows (vgx_get_tau_flows): its two forms against each other and against the route a user had
without it.

Workload: the ensemble shape of tools/probe_tau_incidence.py: 16 haplotypes x 3 populations, 2048 replicates, a
2000-event direct warm-up as the prefix, --steps tau steps per replicate (halved until every replicate's block of the multievent
log holds its rows) on the device step loop (VGX_TAU_STEP_KERNELS=0).  The window runs from half of the prefix's last time to 0.9
of the latest final time.  Two grids: T = --bins (100), and T = --long-bins (at least the number of steps, so that nearly every
step changes the bin: the flush scan of the dense form runs once per step there); the long grid runs over the first
--long-replicates replicates, which bounds its block.  Measured at V = 1 (one class) and V = 16 (every haplotype its own class),
where both forms fit.
Three routes to the same [n, T, P, P, V] int64 block, compared bit for bit in an untimed warm-up round before anything is timed:
  dense    ens.tau_flows(...) under VGX_FLOWS_FORM=dense: all P * P * V int64 cells of a bin in LDS;
  split    ens.tau_flows(...) under VGX_FLOWS_FORM=split: the diagonal in LDS, a row off it straight to device memory;
  host     per replicate ens.replicate_events(r) + ens.engine.multievents(r) (48 bytes per row to the host), then a weighted numpy
           histogram (searchsorted on the step times, np.add.at with num), in front of which the model's prefix is counted per
           replicate: the route there is without tau_flows().
The host route runs over the first --host-replicates replicates, and all routes are reported PER REPLICATE.  The routes are timed
ROUNDS times in alternation (dense, split, host, dense, ...).  Reported, median [min, max]: wall time of every route per replicate;
split over dense round by round on wall time and on ms[0] (kernels); host over either device route; the max / min spread of
dense's own rounds, which is what a difference between the forms has to exceed.

    python tools/probe_tau_flows.py [--rounds 5] [--out FILE.json]
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


def add_weighted(out, t, num, typ, hap, pop, npop, edges, vo, within=True):
    """Rows (time, num, type, haplotype, population, newPopulation) with non-decreasing times into out [T, P, P, V]."""
    T = len(edges) - 1
    b = np.searchsorted(edges, t, side='right') - 1
    ok = (b >= 0) & (b < T) & (num > 0) & ((typ == 5) | ((typ == 0) & bool(within)))
    cls = np.where(ok, vo[np.where(ok, hap, 0)], -1)
    ok &= cls >= 0
    dst = np.where(typ == 5, npop, pop)
    np.add.at(out, (b[ok], pop[ok], dst[ok], cls[ok]), num[ok])


def host_block(ens, reps, edges, P, vo, V):
    """The route without tau_flows(): every replicate's records and rows to the host, then numpy."""
    m = ens.model
    n_pre = int(m.events.ptr)
    pre = m.events
    assert not (pre.types[:n_pre] == 6).any(), "the probe's prefix is a direct warm-up"
    vo = vo.astype(np.int64)
    out = np.zeros((len(reps), len(edges) - 1, P, P, V), dtype=np.int64)
    for i, r in enumerate(reps):
        c = ens.engine.counters(int(r))
        own = ens.replicate_events(int(r))[:, int(c.ev_first_new):]
        rows = ens.engine.multievents(int(r))
        if c.restarts == 0:
            add_weighted(out[i], pre.times[:n_pre], np.ones(n_pre, dtype=np.int64), pre.types[:n_pre], pre.haplotypes[:n_pre],
                         pre.populations[:n_pre], pre.newPopulations[:n_pre], edges, vo)
        t = np.repeat(own[0], (own[3] - own[2]).astype(np.int64))      # a row carries the time of its step's MULTITYPE record
        add_weighted(out[i], t, rows["num"], rows["types"], rows["haplotypes"], rows["populations"], rows["newPopulations"], edges, vo)
    return out


def small_model():
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=2, populations_number=3, seed=7)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.05)
    s.set_total_migration_probability(0.002); s.set_population_size(10 ** 6)
    s.simulate(2000, sample_size=10 ** 12)
    return s


def off_diagonal(block):
    return int(block.sum(dtype=np.int64) - np.diagonal(block, axis1=-3, axis2=-2).sum(dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, default=32)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--long-bins", type=int, default=0, help="0: the number of tau steps that ran")
    ap.add_argument("--long-replicates", type=int, default=256)
    ap.add_argument("--classes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    os.environ["VGX_TAU_STEP_KERNELS"] = "0"
    with helpers.quiet():
        sim = small_model()
    R, steps = a.replicates, a.steps
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    while True:   # the recorded rows of all replicates share 2^28 rows of device memory: halve the steps until a replicate's block holds its rows
        t = time.perf_counter()
        try:
            res = ens.simulate_tau(steps, sample_size=10 ** 15, record_events=True)
        except _capi.VgxError as err:
            if "multievent buffer full" not in str(err) or steps < 20:
                raise
            steps //= 2
            print("multievent buffer full: trying", steps, "steps", flush=True)
            continue
        sim_s = time.perf_counter() - t
        break
    m = ens.model
    P, H, n_pre = m.popNum, m.hapNum, int(m.events.ptr)
    off = np.zeros(R + 1, dtype=np.int64)                              # (the sizing form: offsets only, no rows to the host)
    ens.engine._check(ens.engine.lib.vgx_get_multievents_all(ens.engine.handle, 0, _capi._p(off), None, None))
    own_rows = int(off[-1])
    t_pre = float(m.events.times[n_pre - 1])
    window = (0.5 * t_pre, 0.9 * float(ens.replicate_states_tau()[3].max()))
    sub = np.arange(min(R, a.host_replicates), dtype=np.int64)
    long_bins = a.long_bins if a.long_bins > 0 else steps
    out = {"workload": "16 haplotypes x 3 populations, direct warm-up of 2000 events, device step loop", "rounds": a.rounds, "replicates": R,
           "tau_steps": steps, "prefix_events": n_pre, "own_rows_all_replicates": own_rows, "replicates_with_prefix": int((res.restarts == 0).sum()),
           "simulate_tau_wall_s": sim_s, "window": list(window), "host_route_replicates": len(sub), "cases": {}}

    for T, n_dev in ((a.bins, R), (long_bins, min(R, a.long_replicates))):
        reps_dev = None if n_dev == R else np.arange(n_dev, dtype=np.int64)
        rows_dev = int(off[n_dev]) + n_pre                             # the prefix is read once per call
        for V in a.classes:
            vo = (np.arange(H, dtype=np.int64) % V).astype(np.int32)
            key = "T%d_V%d" % (T, V)

            def device(form, reps):
                os.environ["VGX_FLOWS_FORM"] = form
                t = time.perf_counter()
                fl = ens.tau_flows(bins=T, window=window, variants=vo, replicates=reps)
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
            assert np.array_equal(fd.outside, fs.outside)
            assert off_diagonal(block) > 0, "no transmission across populations in the window"
            _, fd = device("dense", reps_dev)
            _, fs = device("split", reps_dev)
            assert np.array_equal(fd.counts, fs.counts) and np.array_equal(fd.outside, fs.outside), "the forms differ"
            counted, across, block_bytes, passes = int(fd.counts.sum(dtype=np.int64)), off_diagonal(fd.counts), int(fd.counts.nbytes), fd.passes
            bins_hit = float((fd.counts.reshape(n_dev, T, -1).sum(axis=2) > 0).sum(axis=1).mean())
            del fd, fs
            timed = {"%s_%s" % (f, k): [] for f in FORMS for k in ("wall_s", "kernels_ms", "cuts_ms", "library_ms")}
            timed["host_wall_s"] = []
            for rnd in range(a.rounds):
                line = []
                for form in FORMS:
                    td, fl = device(form, reps_dev)
                    for k, v in (("wall_s", td), ("kernels_ms", fl.kernel_ms), ("cuts_ms", fl.clock_ms), ("library_ms", fl.wall_ms)):
                        timed["%s_%s" % (form, k)].append(v)
                    line.append("%s %.4f s (kernels %.3f ms, cuts %.2f ms, library %.2f ms)" % (form, td, fl.kernel_ms, fl.clock_ms, fl.wall_ms))
                    del fl
                th, _ = host(edges)
                timed["host_wall_s"].append(th)
                print("%s round %d over %d replicates: %s; host %.4f s over %d" % (key, rnd, n_dev, "; ".join(line), th, len(sub)), flush=True)
            arr = {k: np.asarray(v) for k, v in timed.items()}
            host_per = arr["host_wall_s"] / len(sub)
            spread = float(arr["dense_wall_s"].max() / arr["dense_wall_s"].min())
            kspread = float(arr["dense_kernels_ms"].max() / arr["dense_kernels_ms"].min())
            ratio_wall, ratio_k = arr["split_wall_s"] / arr["dense_wall_s"], arr["split_kernels_ms"] / arr["dense_kernels_ms"]
            out["cases"][key] = dict(
                T=T, V=V, replicates=n_dev, lds_bytes={"dense": 8 * P * P * V, "split": 8 * P * V}, block_bytes=block_bytes, passes=passes,
                rows_read=rows_dev, new_infections_counted=counted, of_them_across=across, bins_with_counts_per_replicate=bins_hit, rounds=timed,
                dense_wall_s_per_replicate=stats(arr["dense_wall_s"] / n_dev), split_wall_s_per_replicate=stats(arr["split_wall_s"] / n_dev),
                host_wall_s_per_replicate=stats(host_per),
                host_over_dense_per_replicate=stats(host_per / (arr["dense_wall_s"] / n_dev)),
                host_over_split_per_replicate=stats(host_per / (arr["split_wall_s"] / n_dev)),
                split_over_dense_wall=stats(ratio_wall), split_over_dense_kernels=stats(ratio_k),
                dense_wall_spread_max_over_min=spread, dense_kernels_spread_max_over_min=kspread,
                split_faster_beyond_dense_spread=bool(np.median(ratio_wall) < 1.0 / spread),
                split_kernels_faster_beyond_dense_spread=bool(np.median(ratio_k) < 1.0 / kspread),
                dense_kernels_ms=stats(arr["dense_kernels_ms"]), split_kernels_ms=stats(arr["split_kernels_ms"]),
                dense_cuts_ms=stats(arr["dense_cuts_ms"]), split_cuts_ms=stats(arr["split_cuts_ms"]),
                dense_library_ms=stats(arr["dense_library_ms"]), split_library_ms=stats(arr["split_library_ms"]))
            print(key, json.dumps({k: v for k, v in out["cases"][key].items() if k != "rounds"}), flush=True)
            if a.out:    # (written after every case: a later one that fails leaves the earlier result)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
    out["split_faster_beyond_dense_spread_in_every_case"] = all(c["split_faster_beyond_dense_spread"] for c in out["cases"].values())
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    os.environ.pop("VGX_FLOWS_FORM", None)
    ens.close()
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}, indent=1))


if __name__ == "__main__":
    main()
