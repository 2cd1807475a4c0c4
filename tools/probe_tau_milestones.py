"""Measurement of Ensemble.tau_milestones (vgx_get_tau_milestones) in both workgroup shapes next to Ensemble.tau_prevalence on the
same ensemble, in one process.

Shapes (those of tools/probe_tau_prevalence.py, whose models this probe imports):
  ensemble   16 haplotypes x 3 populations, 2048 replicates, a 2000-event direct warm-up as the prefix, --steps tau steps per
             replicate (halved until every replicate's block of the multievent log holds its rows) on the device step loop: steps
             of tens of rows;
  single     ONE replicate on the step-kernel path of a model of 4^7 haplotypes x 4 populations, --single-steps steps after a
             direct warm-up: steps of many thousands of rows, one long chain whose tiles are the only parallelism there is.
Every haplotype its own class (the single shape: h % 64, as the prevalence probe has it), thresholds (10, 100, 1000).
tau_prevalence(points=53) runs over the window from half of the prefix's last time to 0.9 of the latest final time.
ROUNDS times in alternation: tau_milestones with workgroups of one wavefront, of four wavefronts (VGX_TAU_MILESTONES_WAVES), and
tau_prevalence.  Reported, median [min, max]: kernel ms (pass A, walk and reduction; the prevalence's count and scan), the host's
table ms and the whole call, the walk's cost per row, and the ratios four waves / one and milestones / prevalence.
Before anything is timed the two shapes are compared with each other, `final` with tau_prevalence's and with the engine's state,
and peak with the largest value the grid sees.

    python tools/probe_tau_milestones.py [--rounds 5] [--out profiles/tau_milestones.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

THRESHOLDS = (10, 100, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--single-steps", type=int, default=300)
    ap.add_argument("--single-warm-events", type=int, default=200000)
    ap.add_argument("--points", type=int, default=53)
    ap.add_argument("--shapes", default="ensemble,single")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    from probe_tau_incidence import large_model, small_model
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}

    out = {"points": a.points, "rounds": a.rounds, "thresholds": list(THRESHOLDS), "shapes": {}}
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
        own_rows, own_steps = int(off[-1]), int(res.events.sum()) - n_pre * int((res.restarts == 0).sum())
        t_pre = float(m.events.times[n_pre - 1])
        window = (0.5 * t_pre, 0.9 * float(ens.replicate_states_tau()[3].max()))
        vo = np.arange(H) if 8 * P * H <= 65536 else np.arange(H) % 64
        V = int(vo.max()) + 1

        def milestones(waves):
            os.environ["VGX_TAU_MILESTONES_WAVES"] = str(waves)
            try:
                return ens.tau_milestones(variants=vo, thresholds=THRESHOLDS)
            finally:
                os.environ.pop("VGX_TAU_MILESTONES_WAVES", None)

        def prevalence():
            return ens.tau_prevalence(points=a.points, window=window, variants=vo)

        ms, ms4, pv = milestones(1), milestones(4), prevalence()       # warm-up and checks
        for k in ("final", "peak", "peak_event", "last_positive_event", "first_event"):
            assert np.array_equal(getattr(ms, k), getattr(ms4, k)), "the two workgroup shapes differ in " + k
        assert np.array_equal(ms.final[:, :P], pv.final) and (ms.peak[:, :P] >= pv.values.max(axis=1)).all()
        if V == H:
            assert np.array_equal(ms.final[:, :P], ens.replicate_states_tau()[0]), "final differs from the engine's state"
        keys = ("milestones_one_wave", "milestones_four_waves", "prevalence")
        timed = {k + "_" + f: [] for k in keys for f in ("kernels_ms", "host_ms", "library_ms")}
        for rnd in range(a.rounds):
            got = (milestones(1), milestones(4), prevalence())
            for k, g in zip(keys, got):
                timed[k + "_kernels_ms"].append(g.kernel_ms)
                timed[k + "_host_ms"].append(g.clock_ms)
                timed[k + "_library_ms"].append(g.wall_ms)
            print(name, "round", rnd, " ".join("%s %.3f" % (k, v[-1]) for k, v in timed.items()), flush=True)
        one, four, prev = (np.asarray(timed[k + "_kernels_ms"]) for k in keys)
        rows_all = own_rows + (int(m.events.ptr) if n_pre else 0)      # (the prefix's rows are read once per call)
        out["shapes"][name] = dict(
            haplotypes=int(H), populations=P, classes=V, replicates=R, tau_steps=steps, step_kernels=os.environ["VGX_TAU_STEP_KERNELS"],
            prefix_events=n_pre, own_rows_all_replicates=own_rows, own_steps_all_replicates=own_steps,
            rows_per_step=own_rows / max(own_steps, 1), lds_record_bytes=(P + 1) * V * (40 + 4 * len(THRESHOLDS)) + 16,
            milestones_passes=ms.passes, prevalence_passes=pv.passes, rounds_ms=timed,
            **{k + "_" + f: stats(timed[k + "_" + f]) for k in keys for f in ("kernels_ms", "host_ms", "library_ms")},
            one_wave_ns_per_row=float(np.median(one)) * 1e6 / rows_all, four_waves_ns_per_row=float(np.median(four)) * 1e6 / rows_all,
            prevalence_ns_per_row=float(np.median(prev)) * 1e6 / rows_all,
            four_waves_over_one=stats(four / one), one_wave_over_prevalence=stats(one / prev), four_waves_over_prevalence=stats(four / prev))
        print(name, json.dumps({k: v for k, v in out["shapes"][name].items() if k != "rounds_ms"}), flush=True)
        ens.close()
        if a.out:    # (written after every shape: a later shape that fails leaves the earlier result)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
