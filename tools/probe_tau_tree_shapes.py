"""Measurement of Ensemble.tau_tree_shapes (vgx_get_tau_tree_shapes) next to the route to the same rows without it.

Workloads: those of tools/probe_tau_lineages.py, 2048 replicates of tau_b (2000 direct events of warm-up, then 200 tau steps) and
512 of tau_d (30000 direct events, then 40 steps), with the event log.  Per workload, in one process, ROUNDS times in alternation:
tau_tree_shapes(seed), and the old route: tau_genealogies(seed) followed by _capi.tree_shape over every healthy replicate's tree.
Reported per round and as median [min, max]: the canonicalise, walk, node-time and shape kernels of tau_tree_shapes() apart
(TreeShapes.stage_ms), its host part (descriptors and step-time tables), everything else of the call (whole call minus kernels) and
the whole call; the old route as its C call (GenealogyBatch.wall_ms), the Python around it (sizing call, output arrays) and the host
loop over the trees.  Before anything is timed status and generator are compared with tau_genealogies() and every healthy row with
the host sweep.

vgx_tau_genealogies.hip gained a launcher for its walk kernel, so the device time of tau_genealogies() is wanted from the library of
the commit before, in the same session: --parent-library PATH runs this tool again in a fresh process per workload on that library
(--genealogies-only: it then calls nothing that library lacks).  The finding reported is whether the difference of two medians
exceeds the run-to-run spread (max - min) observed in either series.

    python tools/probe_tau_tree_shapes.py [--rounds 5] [--parent-library OLD/libvgx.so] [--out profiles/tau_tree_shapes.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from probe_tau_lineages import WORKLOADS, ensemble, genealogies_only, stats, versus   # noqa: E402  (the same ensembles)

NEW_SYMBOLS = ("vgx_get_tau_tree_shapes", "vgx_test_tau_node_times", "vgx_test_tau_node_times_device")


def old_route(ens, seed):
    """What a user does without the call: (batch, rows of the healthy replicates, ms of the C call, of the whole Python call, of the loop)."""
    from vgsim_amd import _capi
    t0 = time.perf_counter()
    b = ens.tau_genealogies(seed=seed)
    t1 = time.perf_counter()
    rows = {}
    for i, r in enumerate(b.replicates):
        if b.status[i] == 0:
            g = b.replicate(int(r))
            rows[i] = _capi.tree_shape(g["tree"], np.zeros(len(g["tree"]), dtype=np.int64), g["times"])
    t2 = time.perf_counter()
    return b, rows, b.wall_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def workload(case, R, a):
    ens = ensemble(case, R)
    ts = ens.tau_tree_shapes(seed=a.seed)   # warm-up, and the check
    b, rows, _, _, _ = old_route(ens, a.seed)
    assert np.array_equal(ts.status, b.status) and np.array_equal(ts.rng_raw, b.rng_raw), "the walk differs from that of tau_genealogies()"
    for i, (st, ln) in rows.items():
        N = 2 * int(st[0]) - 1
        assert np.array_equal(ts.stats[i, :10], st[:10]) and all(ts.lengths[i, k] == ln[k] for k in (0, 1, 6)), "row %d differs from the host sweep" % i
        assert all(abs(ts.lengths[i, k] - ln[k]) <= 4 * (N + 2) * 2.0 ** -53 * ln[k] for k in (2, 3, 4, 5)), "row %d: a length sum" % i
    keys = ("canonicalise_ms", "walk_ms", "node_times_ms", "shape_ms", "kernels_ms", "host_part_ms", "outside_kernels_ms", "call_ms", "python_call_ms")
    old_keys = ("c_call_ms", "python_call_ms", "host_loop_ms", "route_ms", "kernels_ms")
    timed, old = {k: [] for k in keys}, {k: [] for k in old_keys}
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        ts = ens.tau_tree_shapes(seed=a.seed)
        py_ms = (time.perf_counter() - t0) * 1e3
        kern = sum(ts.stage_ms)
        for k, v in zip(keys, tuple(ts.stage_ms) + (kern, ts.clock_ms, ts.wall_ms - kern, ts.wall_ms, py_ms)):
            timed[k].append(v)
        b, rows, c_ms, call_ms, loop_ms = old_route(ens, a.seed)
        for k, v in zip(old_keys, (c_ms, call_ms, loop_ms, call_ms + loop_ms, b.kernel_ms)):
            old[k].append(v)
        print(case, "round", rnd, "tau_tree_shapes canonicalise %.3f, walk %.3f, node times %.3f, shape %.3f ms (host part %.2f, call %.2f, in Python %.2f ms);"
              "  old route: C call %.2f, Python call %.2f, host loop %.2f ms"
              % (tuple(ts.stage_ms) + (ts.clock_ms, ts.wall_ms, py_ms, c_ms, call_ms, loop_ms)), flush=True)
    m = ens.model
    out = {"workload": case, "replicates": R, "prefix_events": int(m.events.ptr), "passes": ts.passes, "healthy_walks": int(ts.ok.sum()),
           "nodes": int((2 * ts.tips[ts.ok] - 1).sum()), "tau_tree_shapes": {k: stats(v) for k, v in timed.items()},
           "old_route": {k: stats(v) for k, v in old.items()}}
    new, was = out["tau_tree_shapes"], out["old_route"]
    out["old_route_over_call"] = was["route_ms"]["median"] / new["python_call_ms"]["median"]
    out["node_times_plus_shape_over_walk"] = (new["node_times_ms"]["median"] + new["shape_ms"]["median"]) / new["walk_ms"]["median"]
    both = [c + w for c, w in zip(timed["canonicalise_ms"], timed["walk_ms"])]
    new["canonicalise_plus_walk_ms"] = stats(both)
    out["shapes_vs_genealogies_canonicalise_plus_walk"] = versus(was["kernels_ms"], new["canonicalise_plus_walk_ms"])
    ens.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--parent-library", default=None, help="libvgx.so of the commit before")
    ap.add_argument("--genealogies-only", default=None, metavar="CASE:R", help="(the child run on another library)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.genealogies_only:
        from vgsim_amd import _capi
        lib = ctypes.CDLL(_capi.LIB_PATH)
        for name in list(_capi.SIGNATURES):   # a library of the commit before lacks the new symbols: bind what it has
            if name in NEW_SYMBOLS and not hasattr(lib, name):
                _capi.SIGNATURES.pop(name)
        case, R = a.genealogies_only.split(":")
        print("RESULT " + json.dumps(genealogies_only(case, int(R), a.rounds, a.seed)), flush=True)
        return
    out = {"rounds": a.rounds, "workloads": []}
    for case, R in WORKLOADS:
        w = workload(case, R, a)
        if a.parent_library:   # tau_genealogies' kernels are the same on both libraries
            env = dict(os.environ, VGX_LIBRARY=os.path.abspath(a.parent_library))
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--genealogies-only", "%s:%d" % (case, R), "--rounds", str(a.rounds),
                                  "--seed", str(a.seed)], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            parent = json.loads([line for line in txt.splitlines() if line.startswith("RESULT ")][-1][7:])
            w["tau_genealogies_kernels_parent_library_ms"] = parent
            w["tau_genealogies_parent_vs_this_library"] = versus(parent, w["old_route"]["kernels_ms"])
        out["workloads"].append(w)
    out["not_measured"] = ["several passes", "steps near 8192 raw rows", "tau_a and tau_c at scale", "other replicate counts"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
