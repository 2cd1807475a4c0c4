"""Measurement of Ensemble.timelines() (the device log replay) against the per-replicate host loop.

Workload: c3_s5_p16, R replicates x N events each (sample_size unbounded), one direct call with the event log; 16 infectious and
4 susceptible compartments (the ones occupied at the end of replicate 0 first), step_num = 100.  Reports
  (i)   ms[0..2] of the C call: pack + replay kernels (HIP events around the launches), host clock, whole call; and the wall time
        of timelines() itself;
  (ii)  the replay kernel's device time (the call's kernel time minus that of a call without queries, which runs the pack kernel
        alone) next to its floor: the log bytes it must read (24 B x events) over the read-only stream rate bench.py's
        stream_rates() measures on the same GPU;
  (iii) the host loop an ensemble offers without timelines(): replicate_state + replicate_events + one numpy replay per query, over
        LOOP replicates, scaled to R (labelled as scaled), and the ratio.  Every replicate of the loop is checked against the batch.

    python tools/probe_ensemble_timelines.py [--replicates 4096] [--events 100000] [--loop 64] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
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
    ap.add_argument("--step-num", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    # the plain-stream rates of this GPU, measured as bench.py --full measures them, in a process of their own before the engine exists
    code = "import sys, json; sys.path.insert(0, %r); import bench; print('STREAMS ' + json.dumps(bench.stream_rates(0)))" % ROOT
    child = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if child.returncode != 0:
        raise RuntimeError("bench.stream_rates failed: " + child.stderr.decode()[-2000:])
    streams = json.loads([l for l in child.stdout.decode().splitlines() if l.startswith("STREAMS ")][-1][8:])
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd._model import Events
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, "c3_s5_p16")
        phases[0][0](sim)
    R, step = a.replicates, a.step_num
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    t = time.perf_counter()
    res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
    sim_s = time.perf_counter() - t
    m0 = ens.replicate_state(0)
    occ = [tuple(int(x) for x in ph) for ph in np.argwhere(m0.infectious > 0)]
    rng = np.random.default_rng(0)
    rng.shuffle(occ)
    inf = occ[:16]
    while len(inf) < 16:
        q = (int(rng.integers(0, m0.popNum)), int(rng.integers(0, m0.hapNum)))
        if q not in inf:
            inf.append(q)
    sus = [(p, 0) for p in range(4)]
    out = {"workload": "c3_s5_p16", "replicates": R, "events_per_replicate": a.events, "kernel": ens.engine.last_kernel,
           "total_events": res.total_events, "simulate_wall_s": sim_s, "step_num": step, "infectious_queries": len(inf),
           "susceptible_queries": len(sus)}
    ens.timelines(infectious=inf, susceptible=sus, step_num=step, replicates=np.arange(min(R, 64)))   # warm-up (code objects, allocator)
    for semantics in ("first_call", "reference", "compartment"):   # first_call: 'reference' including the allocation of the pinned staging
        t = time.perf_counter()
        b = ens.timelines(infectious=inf, susceptible=sus, step_num=step, semantics="reference" if semantics == "first_call" else semantics)
        wall = time.perf_counter() - t
        out[semantics] = {"timelines_wall_s": wall, "kernels_ms": b.kernel_ms, "host_clock_ms": b.clock_ms, "c_call_ms": b.wall_ms,
                          "replay_launches": b.passes, "events_per_s": res.total_events / wall}
        print(semantics, json.dumps(out[semantics]), flush=True)
        if semantics == "reference":
            batch = b
    t = time.perf_counter()
    none = ens.timelines(step_num=step)
    out["no_queries"] = {"timelines_wall_s": time.perf_counter() - t, "pack_kernel_ms": none.kernel_ms, "host_clock_ms": none.clock_ms,
                         "c_call_ms": none.wall_ms}
    log_bytes = 24 * res.total_events
    replay_ms = batch.kernel_ms - none.kernel_ms
    floor_ms = log_bytes / (streams["read_only_sum_GBs"] * 1e9) * 1e3
    out["replay_kernel"] = {"device_ms (kernels_ms - pack_kernel_ms)": replay_ms, "log_bytes": log_bytes, "this_gpu_streams": streams,
                            "floor_ms (log bytes / read-only stream rate)": floor_ms, "times_the_floor": replay_ms / floor_ms,
                            "staged_bytes_to_host (12 B/event)": 12 * res.total_events}
    L = min(a.loop, R)
    t = time.perf_counter()
    for r in range(L):
        m = ens.replicate_state(r)
        chain = ens.replicate_events(r)
        ev = Events()
        ev.CreateEvents(max(chain.shape[1], 1))
        ev.times[:chain.shape[1]] = chain[0]
        for k, name in enumerate(ev.COLUMNS):
            getattr(ev, name)[:chain.shape[1]] = chain[k + 1].astype(np.int64)
        ev.ptr = chain.shape[1]
        m.events = ev
        for k, (p, h) in enumerate(inf):
            data, sample, tp, _ = m.get_data_infectious(p, h, step)
            assert np.array_equal(batch.infectious[r, k], data) and np.array_equal(batch.samples[r, k], sample)
            assert batch.time_points[r].tolist() == tp
        for k, (p, s) in enumerate(sus):
            assert np.array_equal(batch.susceptible[r, k], m.get_data_susceptible(p, s, step)[0])
    loop = time.perf_counter() - t
    out["host_loop"] = {"replicates_timed": L, "wall_s": loop, "wall_s_scaled_to_R (scaled, not run)": loop * R / L}
    out["speedup_vs_scaled_loop"] = loop * R / L / out["reference"]["timelines_wall_s"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ens.close()


if __name__ == "__main__":
    main()
