"""Measurement of Ensemble.tau_timelines() (the device replay of tau chains) against the per-replicate host path.

Workload: a case of tests/models.py with a tau phase (default tau_d: 30 000 direct events of warm-up, then 40 tau steps), R replicates
of the tau phase with the event log; 16 infectious and 4 susceptible compartments (the ones occupied at the end of replicate 0
first), step_num = 100.  Reports
  (i)  ms[0..2] of the C call: replay kernel (HIP events around the launches), the host's cut search, whole call; and the wall time of
       tau_timelines() itself, for the first and for repeated calls;
  (ii) the path an ensemble offers without tau_timelines(): replicate_multievents() once, then per replicate replicate_events and
       the host replay (_model.py) of prefix + own steps, over LOOP replicates, scaled to R (labelled as scaled, not run), and the
       ratio.  Every replicate of the loop is checked against the batch.
No torch work: one process.  Run every GPU step under a time limit of its own, e.g.

    timeout -k 10 600 python tools/probe_ensemble_tau_timelines.py [--case tau_d] [--replicates 4096] [--loop 64] [--out FILE.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="tau_d")
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--step-num", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd._model import Events, MultiEvents
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, a.case)
        phases[0][0](sim)
        sim.simulate(**phases[0][1])
    nt = phases[1][1]["iterations"]
    m = sim.simulation
    R, step = a.replicates, a.step_num
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    t = time.perf_counter()
    res = ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    sim_s = time.perf_counter() - t
    states = ens.replicate_states_tau()
    occ = [tuple(int(x) for x in ph) for ph in np.argwhere(states[0][0] > 0)]
    rng = np.random.default_rng(0)
    rng.shuffle(occ)
    inf = occ[:16]
    while len(inf) < min(16, m.popNum * m.hapNum):
        q = (int(rng.integers(0, m.popNum)), int(rng.integers(0, m.hapNum)))
        if q not in inf:
            inf.append(q)
    sus = [(p, s) for p in range(m.popNum) for s in range(m.susNum)][:4]
    t = time.perf_counter()
    off, rows = ens.replicate_multievents()
    readout_s = time.perf_counter() - t
    own_rows = int(off[-1])
    out = {"workload": a.case, "replicates": R, "tau_steps_per_replicate": nt, "prefix_events": int(m.events.ptr),
           "own_rows_all_replicates": own_rows, "row_bytes_read_by_the_kernel": 48 * (own_rows + R * int(m.events.ptr)),
           "restarted_replicates": int((res.restarts > 0).sum()), "simulate_tau_wall_s": sim_s, "step_num": step,
           "infectious_queries": len(inf), "susceptible_queries": len(sus)}
    for label, semantics in (("first_call", "reference"), ("reference", "reference"), ("compartment", "compartment")):
        t = time.perf_counter()
        b = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=step, semantics=semantics)
        wall = time.perf_counter() - t
        out[label] = {"tau_timelines_wall_s": wall, "kernel_ms": b.kernel_ms, "host_cuts_ms": b.clock_ms, "c_call_ms": b.wall_ms,
                      "replay_launches": b.passes}
        print(label, json.dumps(out[label]), flush=True)
        if label == "reference":
            batch = b
    t = time.perf_counter()
    none = ens.tau_timelines(step_num=step)
    out["no_queries"] = {"tau_timelines_wall_s": time.perf_counter() - t, "host_cuts_ms": none.clock_ms, "c_call_ms": none.wall_ms}
    # the path that exists without tau_timelines(): the rows of all replicates to the host, then a host replay per replicate
    L = min(a.loop, R)
    n_pre, k_pre = int(m.events.ptr), int(m.multievents.ptr)
    t = time.perf_counter()
    for r in range(L):
        c = ens.engine.counters(r)
        pre_e, pre_k = (0, 0) if c.restarts > 0 else (n_pre, k_pre)
        own = ens.replicate_events(r)[:, int(c.ev_first_new):]
        hm = copy.copy(m)
        hm.currentTime = float(states[3][r])
        ev = Events()
        ev.CreateEvents(max(pre_e + own.shape[1], 1))
        ev.times[:pre_e] = m.events.times[:pre_e]
        ev.times[pre_e:pre_e + own.shape[1]] = own[0]
        for k, name in enumerate(ev.COLUMNS):
            col = own[k + 1].astype(np.int64)
            if name in ("haplotypes", "populations"):
                col = col + pre_k
            getattr(ev, name)[:pre_e] = getattr(m.events, name)[:pre_e]
            getattr(ev, name)[pre_e:pre_e + own.shape[1]] = col
        ev.ptr = pre_e + own.shape[1]
        mv = MultiEvents()
        sl = slice(int(off[r]), int(off[r + 1]))
        steps_of = rows["steps"][sl]
        mv.extend(np.concatenate((m.multievents.times[:pre_k], own[0][steps_of])),
                  **{name: np.concatenate((getattr(m.multievents, name)[:pre_k], rows[name][sl])) for name in mv.COLUMNS})
        hm.events, hm.multievents = ev, mv
        for k, (p, h) in enumerate(inf):
            data, sample, tp, _ = hm.get_data_infectious(p, h, step)
            assert np.array_equal(batch.infectious[r, k], data) and np.array_equal(batch.samples[r, k], sample), (r, p, h)
            assert batch.time_points[r].tolist() == tp
        for k, (p, s) in enumerate(sus):
            assert np.array_equal(batch.susceptible[r, k], hm.get_data_susceptible(p, s, step)[0]), (r, p, s)
    loop = time.perf_counter() - t
    out["host_path"] = {"replicate_multievents_wall_s (all replicates, run)": readout_s, "replicates_timed": L, "loop_wall_s": loop,
                        "loop_wall_s_scaled_to_R (scaled, not run)": loop * R / L,
                        "total_s (read-out + scaled loop)": readout_s + loop * R / L}
    out["speedup_vs_scaled_host_path"] = out["host_path"]["total_s (read-out + scaled loop)"] / out["reference"]["tau_timelines_wall_s"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ens.close()


if __name__ == "__main__":
    main()
