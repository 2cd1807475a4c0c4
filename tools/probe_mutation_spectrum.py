"""Measurement of Ensemble.mutation_spectrum / tau_mutation_spectrum (vgx_get_mutation_spectrum, vgx_get_tau_mutation_spectrum) next
to what a user did before them: genealogies() / tau_genealogies() and the host sweep over every healthy replicate's tree and
mutation records.

Workloads: that of tools/probe_tree_shapes.py: c3_s5_p16 (16 populations, 1024 haplotypes), 4096 replicates x 10^5 events each in
one direct call with the event log; and those of tools/probe_tau_lineages.py: 2048 replicates of tau_b and 512 of tau_d.  Per
workload, in one process, ROUNDS times in alternation: the new call, and the old route (the genealogies call followed by
_capi.mutation_spectrum over every healthy replicate).  Reported per round and as median [min, max]: the walk kernel and the
spectrum kernel apart (and the canonicalise kernel of a tau call), the whole C call and the call as Python sees it; the old route as
its C call, the Python call and the host loop.  On the direct workload tree_shapes() runs in the same alternation: the expectation
recorded with the issue is that mutation_spectrum() costs about its walk kernel plus copy-out, that is tree_shapes() less its host
clock.  Before anything is timed status and generator are compared with the genealogies call and every healthy row with the host
sweep, for equality.

    python tools/probe_mutation_spectrum.py [--rounds 5] [--out profiles/mutation_spectrum.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from probe_tau_lineages import WORKLOADS, ensemble, stats, versus   # noqa: E402  (the same tau ensembles)

BLOCKS = ("spectrum", "substitutions", "sums", "stats")


def old_route(batch_call, S):
    """(batch, rows of the healthy replicates, ms of the C call, of the Python call, of the host loop)."""
    from vgsim_amd import _capi
    t0 = time.perf_counter()
    b = batch_call()
    t1 = time.perf_counter()
    rows = {}
    for i in np.nonzero(b.status == 0)[0]:
        n0, n1, m0, m1 = b.node_offsets[i], b.node_offsets[i + 1], b.mut_offsets[i], b.mut_offsets[i + 1]
        rows[int(i)] = _capi.mutation_spectrum(b.tree[n0:n1], b.mut_node[m0:m1], b.mut_AS[m0:m1], b.mut_DS[m0:m1], b.mut_site[m0:m1], S)
    t2 = time.perf_counter()
    return b, rows, b.wall_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def check(ms, b, rows):
    assert np.array_equal(ms.status, b.status) and np.array_equal(ms.rng_raw, b.rng_raw), "the walk differs from that of the genealogies call"
    for i, want in rows.items():
        for k, w in zip(BLOCKS, want):
            assert np.array_equal(getattr(ms, k)[i], w), "row %d: %s differs from the host sweep" % (i, k)


def measure(case, ens, new_call, batch_call, a, stages, beside=None):
    S = int(ens.model.sites)
    ms = new_call()   # warm-up (code objects, allocator), and the check
    b, rows, _, _, _ = old_route(batch_call, S)
    check(ms, b, rows)
    keys = stages + ("call_ms", "python_call_ms")
    old_keys = ("c_call_ms", "python_call_ms", "host_loop_ms", "route_ms", "kernels_ms")
    timed, old, other = {k: [] for k in keys}, {k: [] for k in old_keys}, {}
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        ms = new_call()
        py_ms = (time.perf_counter() - t0) * 1e3
        st = tuple(ms.stage_ms) if hasattr(ms, "stage_ms") else tuple(ms.kernel_ms)
        for k, v in zip(keys, st + (ms.wall_ms, py_ms)):
            timed[k].append(v)
        b, rows, c_ms, call_ms, loop_ms = old_route(batch_call, S)
        for k, v in zip(old_keys, (c_ms, call_ms, loop_ms, call_ms + loop_ms, b.kernel_ms)):
            old[k].append(v)
        line = "%s round %d: %s; call %.2f ms (in Python %.2f);  old route: C call %.2f, Python call %.2f, host loop %.2f ms" % (
            case, rnd, ", ".join("%s %.3f" % (k[:-3], v) for k, v in zip(stages, st)), ms.wall_ms, py_ms, c_ms, call_ms, loop_ms)
        if beside is not None:
            t0 = time.perf_counter()
            ts = beside()
            for k, v in zip(("walk_ms", "shape_ms", "clock_ms", "call_ms", "python_call_ms"),
                            tuple(ts.kernel_ms) + (ts.clock_ms, ts.wall_ms, (time.perf_counter() - t0) * 1e3)):
                other.setdefault(k, []).append(v)
            line += ";  tree_shapes call %.2f ms (clock %.2f)" % (ts.wall_ms, ts.clock_ms)
        print(line, flush=True)
    ok = ms.ok
    out = {"workload": case, "replicates": int(len(ms.replicates)), "sites": S, "passes": ms.passes, "healthy_walks": int(ok.sum()),
           "nodes": int((2 * ms.tips[ok] - 1).sum()), "records": int(ms.mutations[ok].sum()), "tips_median": float(np.median(ms.tips[ok])),
           "singleton_share_median": float(np.nanmedian(ms.singleton_share())), "tajimas_d_median": float(np.nanmedian(ms.tajimas_d())),
           "new_call": {k: stats(v) for k, v in timed.items()}, "old_route": {k: stats(v) for k, v in old.items()}}
    out["route_over_call"] = out["old_route"]["route_ms"]["median"] / out["new_call"]["python_call_ms"]["median"]
    out["call_vs_old_c_call"] = versus(out["new_call"]["call_ms"], out["old_route"]["c_call_ms"])
    if other:
        out["tree_shapes"] = {k: stats(v) for k, v in other.items()}
        out["call_vs_tree_shapes"] = versus(out["new_call"]["call_ms"], out["tree_shapes"]["call_ms"])
        out["tree_shapes_less_clock_ms"] = out["tree_shapes"]["call_ms"]["median"] - out["tree_shapes"]["clock_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4096)
    ap.add_argument("--events", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--skip-direct", action="store_true")
    ap.add_argument("--skip-tau", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    import models
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble

    out = {"rounds": a.rounds, "workloads": []}
    if not a.skip_direct:
        R = a.replicates
        with helpers.quiet():
            sim, phases = models.build(Simulator, "c3_s5_p16")
            phases[0][0](sim)
        ens = Ensemble(sim, R, seeds=1000 + np.arange(R, dtype=np.int64))
        with helpers.quiet():
            res = ens.simulate(a.events, sample_size=10 ** 12, record_events=True)
        w = measure("c3_s5_p16", ens, lambda: ens.mutation_spectrum(seed=None), lambda: ens.genealogies(seed=None), a,
                    ("walk_ms", "spectrum_ms"), beside=lambda: ens.tree_shapes(seed=None))
        w["events_asked"], w["total_events"], w["kernel"] = a.events, int(res.events.sum()), ens.engine.last_kernel
        out["workloads"].append(w)
        ens.close()
    if not a.skip_tau:
        for case, R in WORKLOADS:
            ens = ensemble(case, R)
            w = measure(case, ens, lambda: ens.tau_mutation_spectrum(seed=a.seed), lambda: ens.tau_genealogies(seed=a.seed), a,
                        ("canonicalise_ms", "walk_ms", "spectrum_ms"))
            w["prefix_events"] = int(ens.model.events.ptr)
            out["workloads"].append(w)
            ens.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
