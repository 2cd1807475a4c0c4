"""Measurement of Ensemble.introductions / tau_introductions (vgx_get_introductions, vgx_get_tau_introductions) next to what a user
did before them: genealogies() / tau_genealogies() and the host sweep over every healthy replicate's tree and node labels.

Workloads: that of tools/probe_mutation_spectrum.py: c3_s5_p16 (16 populations: the LDS form of the kernel), 4096 replicates x 10^5
events each in one direct call with the event log; p70 (70 populations: the global form, rows of 61 KB), 1024 replicates x 2 * 10^4
events; and tau_b x 2048 of tools/probe_tau_lineages.py.  Per workload, in one process, ROUNDS times in alternation: the new call,
and the old route (the genealogies call followed by _capi.introductions over every healthy replicate).  Reported per round and as
median [min, max]: the walk kernel and the lineage kernel apart (and the canonicalise kernel of a tau call), the whole C call and
the call as Python sees it; the old route as its C call, the Python call and the host loop.  The expectation recorded with the
issue is that the call costs about its walk kernel plus a few ms.  Before anything is timed status and generator are compared
with the genealogies call and every healthy row with the host sweep, for equality.

    python tools/probe_introductions.py [--rounds 5] [--out profiles/introductions.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from probe_tau_lineages import ensemble, stats, versus   # noqa: E402  (the same tau ensembles)

BLOCKS = ("tips_by_pop", "imports", "into", "spectrum", "stats")


def old_route(batch_call, P):
    """(batch, rows of the healthy replicates, ms of the C call, of the Python call, of the host loop)."""
    from vgsim_amd import _capi
    t0 = time.perf_counter()
    b = batch_call()
    t1 = time.perf_counter()
    rows = {}
    for i in np.nonzero(b.status == 0)[0]:
        n0, n1 = b.node_offsets[i], b.node_offsets[i + 1]
        rows[int(i)] = _capi.introductions(b.tree[n0:n1], b.tree_pop[n0:n1], P)
    t2 = time.perf_counter()
    return b, rows, b.wall_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def check(it, b, rows):
    assert np.array_equal(it.status, b.status) and np.array_equal(it.rng_raw, b.rng_raw), "the walk differs from that of the genealogies call"
    for i, want in rows.items():
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(it, k)[i], w), "row %d: %s differs from the host sweep" % (i, k)


def measure(case, ens, new_call, batch_call, a, stages):
    P = int(ens.model.popNum)
    it = new_call()   # warm-up (code objects, allocator), and the check
    b, rows, _, _, _ = old_route(batch_call, P)
    check(it, b, rows)
    keys = stages + ("call_ms", "python_call_ms")
    old_keys = ("c_call_ms", "python_call_ms", "host_loop_ms", "route_ms", "kernels_ms")
    timed, old = {k: [] for k in keys}, {k: [] for k in old_keys}
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        it = new_call()
        py_ms = (time.perf_counter() - t0) * 1e3
        st = tuple(it.stage_ms) if hasattr(it, "stage_ms") else tuple(it.kernel_ms)
        for k, v in zip(keys, st + (it.wall_ms, py_ms)):
            timed[k].append(v)
        b, rows, c_ms, call_ms, loop_ms = old_route(batch_call, P)
        for k, v in zip(old_keys, (c_ms, call_ms, loop_ms, call_ms + loop_ms, b.kernel_ms)):
            old[k].append(v)
        print("%s round %d: %s; call %.2f ms (in Python %.2f);  old route: C call %.2f, Python call %.2f, host loop %.2f ms" % (
            case, rnd, ", ".join("%s %.3f" % (k[:-3], v) for k, v in zip(stages, st)), it.wall_ms, py_ms, c_ms, call_ms, loop_ms), flush=True)
    ok = it.ok
    out = {"workload": case, "replicates": int(len(it.replicates)), "populations": P, "form": "lds" if P <= 32 else "global",
           "passes": it.passes, "healthy_walks": int(ok.sum()), "nodes": int((2 * it.tips[ok] - 1).sum()),
           "introductions": int(it.introductions[ok].sum()), "empty": int(it.empty[ok].sum()), "tips_median": float(np.median(it.tips[ok])),
           "introductions_median": float(np.median(it.introductions[ok])), "max_local_median": float(np.median(it.max_local[ok])),
           "new_call": {k: stats(v) for k, v in timed.items()}, "old_route": {k: stats(v) for k, v in old.items()}}
    out["route_over_call"] = out["old_route"]["route_ms"]["median"] / out["new_call"]["python_call_ms"]["median"]
    out["call_vs_old_c_call"] = versus(out["new_call"]["call_ms"], out["old_route"]["c_call_ms"])
    out["call_less_walk_ms"] = out["new_call"]["call_ms"]["median"] - out["new_call"]["walk_ms"]["median"]
    return out


def direct(case, R, events):
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, case)
        phases[0][0](sim)
    ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
    with helpers.quiet():
        res = ens.simulate(events, sample_size=10 ** 12, record_events=True)
    return ens, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--p70-replicates", type=int, default=1024)
    ap.add_argument("--p70-events", type=int, default=20000)
    ap.add_argument("--tau-replicates", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--skip", default="", help="comma-separated workloads to leave out: c3_s5_p16, p70, tau_b")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    out = {"rounds": a.rounds, "workloads": []}

    def keep():
        print(json.dumps(out["workloads"][-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for case, R, events in (("c3_s5_p16", a.replicates, a.events), ("p70", a.p70_replicates, a.p70_events)):
        if case in skip:
            continue
        ens, res = direct(case, R, events)
        w = measure(case, ens, lambda: ens.introductions(seed=None), lambda: ens.genealogies(seed=None), a, ("walk_ms", "lineages_ms"))
        w["events_asked"], w["total_events"], w["kernel"] = events, int(res.events.sum()), ens.engine.last_kernel
        out["workloads"].append(w)
        keep()
        ens.close()
    if "tau_b" not in skip:
        ens = ensemble("tau_b", a.tau_replicates)
        w = measure("tau_b", ens, lambda: ens.tau_introductions(seed=a.seed), lambda: ens.tau_genealogies(seed=a.seed), a,
                    ("canonicalise_ms", "walk_ms", "lineages_ms"))
        w["prefix_events"] = int(ens.model.events.ptr)
        out["workloads"].append(w)
        keep()
        ens.close()


if __name__ == "__main__":
    main()
