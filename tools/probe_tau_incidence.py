"""Measurement of Ensemble.tau_incidence (vgx_get_tau_incidence) against the route a user had without it.

Shapes:
  ensemble   the small-model ensemble of bench.py's tau_small leg: 16 haplotypes x 3 populations, 2048 replicates, a 2000-event
             direct warm-up as the prefix, --steps tau steps per replicate (halved until every replicate's block of the multievent log holds its
             rows) on the device step loop (VGX_TAU_STEP_KERNELS=0);
  single     ONE replicate on the step-kernel path (VGX_TAU_STEP_KERNELS=1) of a model of 4^7 haplotypes x 4 populations = 2^16
             compartments, --single-steps steps after a direct warm-up: a chain whose tiles are the only parallelism there is.
T = 100 bins from half of the prefix's last time to 0.9 of the latest final time.
Two routes to the same [n, T, P, 7] int64 block, compared bit for bit in an untimed warm-up round before anything is timed:
  device   ens.tau_incidence(bins=T, window=...): the rows stay on the device, the prefix is counted once;
  host     per replicate ens.replicate_events(r) + ens.engine.multievents(r) (48 bytes per row to the host), then a weighted numpy
           histogram (searchsorted on the step times, np.add.at with num) in front of which the model's prefix is counted per replicate.
The host route runs over the first --host-replicates replicates, and both routes are reported PER REPLICATE.  Each route is timed
ROUNDS times in alternation.  Reported, median [min, max]: wall time of either route per replicate and their ratio round by round;
ms[0] (kernels), ms[1] (host cut search) and ms[2] of the device route; the rows read x 48 bytes over ms[0] next to the HBM peak (an
UPPER estimate: rows outside the window are loaded 16 bytes each, and ms[0] holds the init kernel too); and
the prefix's part: its rows among all rows read, and the wall time of a call over one replicate (prefix + one chain: an upper bound
of what the prefix costs a call) over the whole call's.

    python tools/probe_tau_incidence.py [--rounds 5] [--out FILE.json]
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


def add_weighted(out, t, num, typ, pop, npop, edges):
    """Rows (time, num, type, population, newPopulation) with non-decreasing times into out [T, P, 7]."""
    T = len(edges) - 1
    b = np.searchsorted(edges, t, side='right') - 1
    ok = (b >= 0) & (b < T) & (num > 0)
    plain = ok & (typ < 5)
    np.add.at(out, (b[plain], pop[plain], typ[plain]), num[plain])
    mig = ok & (typ == 5)
    np.add.at(out, (b[mig], npop[mig], 5), num[mig])
    np.add.at(out, (b[mig], pop[mig], 6), num[mig])


def host_block(ens, reps, edges, P):
    """The route without tau_incidence(): every replicate's records and rows to the host, then numpy."""
    m = ens.model
    n_pre = int(m.events.ptr)
    pre = m.events
    assert not (pre.types[:n_pre] == 6).any(), "the probe's prefix is a direct warm-up"
    out = np.zeros((len(reps), len(edges) - 1, P, 7), dtype=np.int64)
    for i, r in enumerate(reps):
        c = ens.engine.counters(int(r))
        own = ens.replicate_events(int(r))[:, int(c.ev_first_new):]
        rows = ens.engine.multievents(int(r))
        if c.restarts == 0:
            add_weighted(out[i], pre.times[:n_pre], np.ones(n_pre, dtype=np.int64), pre.types[:n_pre], pre.populations[:n_pre],
                         pre.newPopulations[:n_pre], edges)
        t = np.repeat(own[0], (own[3] - own[2]).astype(np.int64))      # a row carries the time of its step's MULTITYPE record
        add_weighted(out[i], t, rows["num"], rows["types"], rows["populations"], rows["newPopulations"], edges)
    return out


def small_model():
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=2, populations_number=3, seed=7)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.05)
    s.set_total_migration_probability(0.002); s.set_population_size(10 ** 6)
    s.simulate(2000, sample_size=10 ** 12)
    return s


def large_model(warm_events):
    from vgsim_amd import Simulator
    s = Simulator(number_of_sites=7, populations_number=4, seed=7)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.05)
    s.set_total_migration_probability(0.002); s.set_population_size(10 ** 8)
    s.simulate(warm_events, sample_size=10 ** 12)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--single-steps", type=int, default=300)
    ap.add_argument("--single-warm-events", type=int, default=200000)
    ap.add_argument("--host-replicates", type=int, default=32)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--shapes", default="ensemble,single")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    out = {"bins": a.bins, "rounds": a.rounds, "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    for name in a.shapes.split(","):
        os.environ["VGX_TAU_STEP_KERNELS"] = "0" if name == "ensemble" else "1"
        with helpers.quiet():
            sim = small_model() if name == "ensemble" else large_model(a.single_warm_events)
        R, steps = (a.replicates, a.steps) if name == "ensemble" else (1, a.single_steps)
        ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
        while True:   # the recorded rows of all replicates share 2^28 rows of device memory: halve the steps until a replicate's block holds its rows
            t = time.perf_counter()
            try:
                res = ens.simulate_tau(steps, sample_size=10 ** 15, record_events=True)
            except _capi.VgxError as err:
                if "multievent buffer full" not in str(err) or steps < 20:
                    raise
                steps //= 2
                print(name, "multievent buffer full: trying", steps, "steps", flush=True)
                continue
            sim_s = time.perf_counter() - t
            break
        m = ens.model
        P, n_pre = m.popNum, int(m.events.ptr)
        off = np.zeros(R + 1, dtype=np.int64)                          # (the sizing form: offsets only, no rows to the host)
        ens.engine._check(ens.engine.lib.vgx_get_multievents_all(ens.engine.handle, 0, _capi._p(off), None, None))
        own_rows = int(off[-1])
        with_prefix = int((res.restarts == 0).sum())
        rows_read = own_rows + n_pre                                   # the prefix is read once per call
        t_pre = float(m.events.times[n_pre - 1])
        window = (0.5 * t_pre, 0.9 * float(ens.replicate_states_tau()[3].max()))
        sub = np.arange(min(R, a.host_replicates), dtype=np.int64)

        def device(reps=None):
            t = time.perf_counter()
            inc = ens.tau_incidence(bins=a.bins, window=window, replicates=reps)
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
        timed = {"device_wall_s": [], "host_wall_s": [], "kernels_ms": [], "cuts_ms": [], "library_ms": [], "one_replicate_wall_s": []}
        for rnd in range(a.rounds):
            td, inc = device()
            th, _ = host()
            t1, _ = device(sub[:1])
            for k, v in (("device_wall_s", td), ("host_wall_s", th), ("kernels_ms", inc.kernel_ms), ("cuts_ms", inc.clock_ms),
                         ("library_ms", inc.wall_ms), ("one_replicate_wall_s", t1)):
                timed[k].append(v)
            print(name, "round", rnd, "device %.4f s over %d replicates (kernels %.3f ms, cuts %.2f ms, library %.2f ms)  host %.4f s over %d  one replicate %.4f s"
                  % (td, R, inc.kernel_ms, inc.clock_ms, inc.wall_ms, th, len(sub), t1), flush=True)
        dev_per = np.asarray(timed["device_wall_s"]) / R
        host_per = np.asarray(timed["host_wall_s"]) / len(sub)
        k_med = float(np.median(timed["kernels_ms"]))
        out["shapes"][name] = dict(
            haplotypes=int(m.hapNum), populations=P, replicates=R, tau_steps=steps, step_kernels=os.environ["VGX_TAU_STEP_KERNELS"],
            prefix_events=n_pre, own_rows_all_replicates=own_rows, replicates_with_prefix=with_prefix, rows_read=rows_read,
            prefix_share_of_rows_read=n_pre / rows_read, prefix_rows_if_read_per_replicate=n_pre * with_prefix,
            simulate_tau_wall_s=sim_s, window=list(window), host_route_replicates=len(sub), passes=inc.passes,
            block_bytes=int(inc.counts.nbytes), rounds=timed,
            device_wall_s=stats(timed["device_wall_s"]), device_wall_s_per_replicate=stats(dev_per),
            host_wall_s_per_replicate=stats(host_per), host_over_device_per_replicate=stats(host_per / dev_per),
            device_spread_max_over_min=float(np.max(timed["device_wall_s"]) / np.min(timed["device_wall_s"])),
            kernels_ms=stats(timed["kernels_ms"]), cuts_ms=stats(timed["cuts_ms"]), library_ms=stats(timed["library_ms"]),
            one_replicate_wall_s=stats(timed["one_replicate_wall_s"]),
            one_replicate_call_over_whole_call=stats(np.asarray(timed["one_replicate_wall_s"]) / np.asarray(timed["device_wall_s"])),
            bytes_note="row_bytes counts 48 bytes for every row read; rows outside the window are loaded 16 bytes each (num only), and ms[0] "
                       "holds the init kernel too: kernels_TBs and the share of the HBM peak are UPPER estimates of the counting kernel's rate",
            row_bytes=48 * rows_read, kernels_TBs=48 * rows_read / (k_med * 1e-3) / 1e12 if k_med > 0 else None,
            kernels_share_of_hbm_peak=48 * rows_read / (k_med * 1e-3) / 1e12 / HBM_PEAK_TBS if k_med > 0 else None)
        print(name, json.dumps({k: v for k, v in out["shapes"][name].items() if k != "rounds"}), flush=True)
        ens.close()
        if a.out:    # (written after every shape: a later shape that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
