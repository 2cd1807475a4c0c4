"""Measurement of Ensemble.tau_prevalence (vgx_get_tau_prevalence) next to Ensemble.tau_incidence on the same ensemble and grid in
one process, and against the route a user had without it.

Shapes (those of tools/probe_tau_incidence.py, whose models this probe imports):
  ensemble   16 haplotypes x 3 populations, 2048 replicates, a 2000-event direct warm-up as the prefix, --steps tau steps per
             replicate (halved until every replicate's block of the multievent log holds its rows) on the device step loop;
  single     ONE replicate on the step-kernel path of a model of 4^7 haplotypes x 4 populations, --single-steps steps after a
             direct warm-up: one long chain whose tiles are the only parallelism there is.
T = 100 grid points (prevalence) / 100 bins (incidence) over the same window, from half of the prefix's last time to 0.9 of the
latest final time; every haplotype its own class (the single shape: h % 64, since 4 x 16384 int64 cells exceed the LDS budget).
Timed ROUNDS times in alternation (prevalence, incidence, host route), after an untimed warm-up round in which the device block is
compared bit for bit with the host route's:
  ms[0] (kernels), ms[1] (host cut search) and ms[2] (whole library call) of both device calls, and the wall time around them;
  host     per replicate ens.replicate_events(r) + ens.engine.multievents(r) (48 bytes per row to the host), then a numpy replay
           (interval of every row by searchsorted on the step times, np.add.at with signed num, cumsum over the intervals), in
           front of which the model's prefix is replayed per replicate; over the first --host-replicates replicates, reported per
           replicate and scaled to R.
Reported, median [min, max] over the rounds; the shares of ms[2] that are kernels and cut search.

    python tools/probe_tau_prevalence.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def add_signed(net, t, num, typ, hap, pop, nhap, npop, grid, vo):
    """Rows with non-decreasing times into the net changes net [T + 1, P, V]: interval k holds the rows with grid[k - 1] < t <= grid[k]."""
    k = np.searchsorted(grid, t, side='left')
    ok = num > 0
    cls, ncls = vo[hap], vo[np.where(typ == 3, nhap, hap)]          # (newHaplotype means something for a MUTATION only)
    for kinds, where, c, sign in (((0,), pop, cls, 1), ((1, 2), pop, cls, -1), ((5,), npop, cls, 1), ((3,), pop, cls, -1), ((3,), pop, ncls, 1)):
        sel = ok & np.isin(typ, kinds) & (c >= 0) & ((typ != 3) | (cls != ncls))
        np.add.at(net, (k[sel], where[sel], c[sel]), sign * num[sel])


def host_block(ens, reps, grid, vo, V, initial):
    """The route without tau_prevalence(): every replicate's records and rows to the host, then numpy.  `initial` [P, H]: the
    model's initial state, where every chain of the probe starts.  (values, final)"""
    m = ens.model
    P, n_pre, pre = m.popNum, int(m.events.ptr), m.events
    assert not (pre.types[:n_pre] == 6).any(), "the probe's prefix is a direct warm-up"
    T = len(grid)
    values, final = np.zeros((len(reps), T, P, V), dtype=np.int64), np.zeros((len(reps), P, V), dtype=np.int64)
    for i, r in enumerate(reps):
        c = ens.engine.counters(int(r))
        own = ens.replicate_events(int(r))[:, int(c.ev_first_new):]
        rows = ens.engine.multievents(int(r))
        net = np.zeros((T + 1, P, V), dtype=np.int64)
        if c.restarts == 0:
            add_signed(net, pre.times[:n_pre], np.ones(n_pre, dtype=np.int64), pre.types[:n_pre], pre.haplotypes[:n_pre], pre.populations[:n_pre],
                       pre.newHaplotypes[:n_pre], pre.newPopulations[:n_pre], grid, vo)
        t = np.repeat(own[0], (own[3] - own[2]).astype(np.int64))      # a row carries the time of its step's MULTITYPE record
        add_signed(net, t, rows["num"], rows["types"], rows["haplotypes"], rows["populations"], rows["newHaplotypes"], rows["newPopulations"], grid, vo)
        start = np.zeros((P, V), dtype=np.int64)
        np.add.at(start.T, vo[vo >= 0], initial[:, vo >= 0].T)
        run = start + np.cumsum(net, axis=0)
        values[i], final[i] = run[:T], run[T]
    return values, final


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--single-steps", type=int, default=300)
    ap.add_argument("--single-warm-events", type=int, default=200000)
    ap.add_argument("--host-replicates", type=int, default=64)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--shapes", default="ensemble,single")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    from probe_tau_incidence import large_model, small_model
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    out = {"points": a.points, "rounds": a.rounds, "shapes": {}}
    for name in a.shapes.split(","):
        os.environ["VGX_TAU_STEP_KERNELS"] = "0" if name == "ensemble" else "1"
        with helpers.quiet():
            sim = small_model() if name == "ensemble" else large_model(a.single_warm_events)
        R, steps = (a.replicates, a.steps) if name == "ensemble" else (1, a.single_steps)
        ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
        while True:   # halve the steps until a replicate's block of the multievent log holds its rows
            try:
                res = ens.simulate_tau(steps, sample_size=10 ** 15, record_events=True)
            except _capi.VgxError as err:
                if "multievent buffer full" not in str(err) or steps < 20:
                    raise
                steps //= 2
                print(name, "multievent buffer full: trying", steps, "steps", flush=True)
                continue
            break
        m = ens.model
        P, H, n_pre = m.popNum, m.hapNum, int(m.events.ptr)
        off = np.zeros(R + 1, dtype=np.int64)                          # (the sizing form: offsets only, no rows to the host)
        ens.engine._check(ens.engine.lib.vgx_get_multievents_all(ens.engine.handle, 0, _capi._p(off), None, None))
        own_rows = int(off[-1])
        t_pre = float(m.events.times[n_pre - 1])
        window = (0.5 * t_pre, 0.9 * float(ens.replicate_states_tau()[3].max()))
        vo = np.arange(H) if 8 * P * H <= 65536 else np.arange(H) % 64
        V = int(vo.max()) + 1
        sub = np.arange(min(R, a.host_replicates), dtype=np.int64)
        initial = np.asarray(ens.replicate_state(0).initial_infectious, dtype=np.int64)

        def prevalence(reps=None):
            t = time.perf_counter()
            pv = ens.tau_prevalence(points=a.points, window=window, variants=vo, replicates=reps)
            return time.perf_counter() - t, pv

        def incidence():
            t = time.perf_counter()
            inc = ens.tau_incidence(bins=a.points, window=window)
            return time.perf_counter() - t, inc

        def host():
            t = time.perf_counter()
            block = host_block(ens, sub, grid, vo, V, initial)
            return time.perf_counter() - t, block

        # warm-up of all routes and the comparison of their results (untimed)
        _, pv = prevalence(sub)
        grid = pv.times
        _, (values, final) = host()
        assert np.array_equal(pv.values, values) and np.array_equal(pv.final, final), "device and host route differ"
        prevalence()
        incidence()
        keys = ("wall_s", "kernels_ms", "cuts_ms", "library_ms")
        timed = {"prevalence": {k: [] for k in keys}, "incidence": {k: [] for k in keys}, "host_wall_s": []}
        for rnd in range(a.rounds):
            tp, pv = prevalence()
            ti, inc = incidence()
            th, _ = host()
            for what, wall, r in (("prevalence", tp, pv), ("incidence", ti, inc)):
                for k, v in zip(keys, (wall, r.kernel_ms, r.clock_ms, r.wall_ms)):
                    timed[what][k].append(v)
            timed["host_wall_s"].append(th)
            print(name, "round", rnd, "prevalence: kernels %.3f ms, cuts %.3f ms, library %.3f ms   incidence: kernels %.3f ms, cuts %.3f ms, library %.3f ms   host %.4f s over %d"
                  % (pv.kernel_ms, pv.clock_ms, pv.wall_ms, inc.kernel_ms, inc.clock_ms, inc.wall_ms, th, len(sub)), flush=True)
        host_per = np.asarray(timed["host_wall_s"]) / len(sub)
        lib = np.asarray(timed["prevalence"]["library_ms"])
        out["shapes"][name] = dict(
            haplotypes=int(H), populations=P, classes=V, replicates=R, tau_steps=steps, step_kernels=os.environ["VGX_TAU_STEP_KERNELS"],
            prefix_events=n_pre, own_rows_all_replicates=own_rows, replicates_with_prefix=int((res.restarts == 0).sum()), window=list(window),
            prevalence_passes=pv.passes, incidence_passes=inc.passes, prevalence_block_bytes=int(pv.values.nbytes + pv.final.nbytes),
            incidence_block_bytes=int(inc.counts.nbytes), rounds=timed,
            prevalence={k: stats(timed["prevalence"][k]) for k in keys}, incidence={k: stats(timed["incidence"][k]) for k in keys},
            prevalence_kernels_share_of_library=stats(np.asarray(timed["prevalence"]["kernels_ms"]) / lib),
            prevalence_cuts_share_of_library=stats(np.asarray(timed["prevalence"]["cuts_ms"]) / lib),
            prevalence_over_incidence_kernels=stats(np.asarray(timed["prevalence"]["kernels_ms"]) / np.asarray(timed["incidence"]["kernels_ms"])),
            host_route_replicates=len(sub), host_ms_per_replicate=stats(1e3 * host_per), host_s_scaled_to_R=stats(host_per * R),
            host_over_device_wall=stats(host_per * R / np.asarray(timed["prevalence"]["wall_s"])))
        print(name, json.dumps({k: v for k, v in out["shapes"][name].items() if k != "rounds"}), flush=True)
        ens.close()
        if a.out:    # (written after every shape: a later shape that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
