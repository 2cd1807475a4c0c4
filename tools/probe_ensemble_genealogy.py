"""Measurement of Ensemble.genealogies() (the device backward pass) against the per-replicate loop over Ensemble.genealogy.

Workload: c3_s5_p16, R replicates x N events each (sample_size unbounded), one direct call with the event log.  Reports the
walk kernels' device time (HIP events around the launches; run under `rocprofv3 --kernel-trace --stats` for the profiler's
figure), the host clock + output conversion, the wall time of genealogies() for both layouts (one replicate per lane / per
wavefront), and the wall time of the host loop over LOOP replicates, scaled to R (labelled as scaled).  Every replicate of
the loop is also checked against the batch.

    python tools/probe_ensemble_genealogy.py [--replicates 4096] [--events 100000] [--loop 64] [--out FILE.json]
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
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    R = a.replicates
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    t = time.perf_counter()
    res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    sim_s = time.perf_counter() - t
    out = {"workload": "c3_s5_p16", "replicates": R, "events_per_replicate": a.events, "kernel": ens.engine.last_kernel,
           "total_events": res.total_events, "simulate_wall_s": sim_s}
    for layout in ("lane", "wave"):
        ens.genealogies(seed=None, replicates=np.arange(min(R, 64)), layout=layout)   # warm-up (code objects, allocator)
        t = time.perf_counter()
        b = ens.genealogies(seed=None, layout=layout)
        wall = time.perf_counter() - t
        out[layout] = {"genealogies_wall_s": wall, "walk_kernel_ms": b.kernel_ms, "clock_and_convert_ms": b.clock_ms,
                       "c_call_ms": b.wall_ms, "passes": b.passes, "ok": int((b.status == 0).sum()),
                       "failed": int((b.status != 0).sum()), "nodes": int(b.node_offsets[-1]),
                       "events_per_s": res.total_events / wall}
        print(layout, json.dumps(out[layout]), flush=True)
        if layout == "wave":   # the default layout
            batch = b
    L = min(a.loop, R)
    t = time.perf_counter()
    for r in range(L):
        try:
            want = ens.genealogy(r, None)
        except RuntimeError as e:
            assert batch.status[r] != 0 and batch.message(r) == str(e)
            continue
        got = batch.replicate(r)
        assert all(np.array_equal(got[k], want[k]) for k in ("tree", "times", "mut_node", "mut_time", "mig_node", "mig_time"))
        assert got["rng_raw"] == want["rng_raw"]
    loop = time.perf_counter() - t
    out["host_loop"] = {"replicates_timed": L, "wall_s": loop, "wall_s_scaled_to_R (scaled)": loop * R / L}
    out["speedup_vs_scaled_loop"] = {k: loop * R / L / out[k]["genealogies_wall_s"] for k in ("wave", "lane")}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ens.close()


if __name__ == "__main__":
    main()
