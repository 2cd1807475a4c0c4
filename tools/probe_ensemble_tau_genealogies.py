"""Measurement of Ensemble.tau_genealogies() (the device backward pass of tau chains) against the per-replicate host route.

Workload: a case of tests/models.py with a tau phase (default tau_b: 2000 direct events of warm-up, then 200 tau steps), R replicates
of the tau phase with the event log, one reseeded walk per replicate.  Reports
  (i)  ms[0..2] of the C call: the canonicalise and walk kernels (HIP events around the launches), the host's conversion of the
       outputs, whole call; the wall time of tau_genealogies() itself, for the first and for a repeated call; raw and canonical rows;
  (ii) the only route an ensemble offers without tau_genealogies(): per replicate engine.multievents(r), replicate_events(r),
       _capi.canonical_multievents and vgx_get_genealogy on prefix + own steps (this is Ensemble.tau_genealogy), over LOOP
       replicates, scaled to R (labelled as scaled, not run), and the ratio.  Every replicate of the loop is checked against the batch.
No torch work: one process.  Run every GPU step under a time limit of its own, e.g.

    timeout -k 10 600 python tools/probe_ensemble_tau_genealogies.py [--case tau_b] [--replicates 2048] [--loop 64] [--out FILE.json]
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
    ap.add_argument("--case", default="tau_b")
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, a.case)
        phases[0][0](sim)
        sim.simulate(**phases[0][1])
    nt = phases[1][1]["iterations"]
    m = sim.simulation
    R = a.replicates
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    t = time.perf_counter()
    res = ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    sim_s = time.perf_counter() - t
    off, _ = ens.replicate_multievents()
    out = {"workload": a.case, "replicates": R, "tau_steps_per_replicate": nt, "prefix_events": int(m.events.ptr),
           "prefix_multievent_rows": int(m.multievents.ptr), "raw_rows_all_replicates": int(off[-1]),
           "restarted_replicates": int((res.restarts > 0).sum()), "simulate_tau_wall_s": sim_s}
    for label in ("first_call", "repeated_call"):
        t = time.perf_counter()
        b = ens.tau_genealogies(seed=a.seed)
        wall = time.perf_counter() - t
        out[label] = {"tau_genealogies_wall_s": wall, "kernels_ms": b.kernel_ms, "host_conversion_ms": b.clock_ms, "c_call_ms": b.wall_ms,
                      "passes": b.passes}
        print(label, json.dumps(out[label]), flush=True)
    out["healthy_replicates"] = int((b.status == 0).sum())
    out["nodes_all_replicates"] = int(b.node_offsets[-1])
    out["statuses"] = {str(int(s)): int((b.status == s).sum()) for s in np.unique(b.status)}
    L = min(a.loop, R)
    t = time.perf_counter()
    for r in range(L):
        try:
            want = ens.tau_genealogy(r, a.seed)
        except RuntimeError as e:
            assert b.status[r] != 0 and b.message(r) == str(e), r
            continue
        got = b.replicate(r)
        for k, v in want.items():
            assert (np.array_equal(got[k], v) if isinstance(v, np.ndarray) else got[k] == v), (r, k)
    loop = time.perf_counter() - t
    out["host_route"] = {"replicates_timed": L, "loop_wall_s": loop, "loop_wall_s_scaled_to_R (scaled, not run)": loop * R / L}
    out["speedup_vs_scaled_host_route"] = (loop * R / L) / out["repeated_call"]["tau_genealogies_wall_s"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ens.close()


if __name__ == "__main__":
    main()
