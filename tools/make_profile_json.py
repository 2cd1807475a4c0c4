"""Turns gpurun_out/prof_<TAG>/ (tools/collect_profiles.sh; TAG from the environment, default r04) into the committed artefacts under profiles/: kernel-stats CSVs,
the raw PMC rows, the SQ summary, and the JSON files bench.py reads for its `traffic` fields."""
import collections, csv, glob, json, os, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = os.environ.get("TAG", "r04")
SRC = os.path.join(ROOT, "gpurun_out", "prof_" + TAG)
DST = os.path.join(ROOT, "profiles")
LEGS = ("headline", "spread_occupancy", "spread_occupancy_fast", "tau_leap", "fast_mode", "table3", "tau_small", "single_trajectory",
        "config3_general", "propensity_scan", "config5")


def one(pattern):
    f = sorted(glob.glob(os.path.join(SRC, pattern)), key=os.path.getmtime)
    assert f, pattern
    return f[-1]      # (a leg collected twice: the later pass)


def pmc(leg, counter, big=False):
    """counter KiB and dispatch count per kernel name; big=True: only the launches within a factor 2 of the kernel's largest
    (a leg may also run the kernel on a single trajectory)"""
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(one("%s_%s/*/*counter_collection.csv" % (leg, "fetch" if counter == "FETCH_SIZE" else "write")))):
        if r["Counter_Name"] == counter:
            per[r["Kernel_Name"]][r["Dispatch_Id"]] += float(r["Counter_Value"])
    agg = collections.defaultdict(lambda: [0.0, 0])
    for k, d in per.items():
        top = max(d.values())
        vals = [v for v in d.values() if not big or v >= 0.5 * top]
        agg[k] = [sum(vals), len(vals)]
    return agg


def sq(leg):
    """SQ counters per kernel, per launch (tools/sq_summary.py's reduction)"""
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    launches = collections.Counter()
    seen = set()
    for f in glob.glob(os.path.join(SRC, "%s_sq/*/*counter_collection.csv" % leg)):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if "vgx_" not in k:
                continue
            agg[k][r["Counter_Name"]] += float(r["Counter_Value"])
            if (k, r["Dispatch_Id"]) not in seen:
                seen.add((k, r["Dispatch_Id"])); launches[k] += 1
    out = {}
    for k, c in agg.items():
        w = max(c.get("SQ_WAVES", 1.0), 1.0)
        wc = c.get("SQ_WAVE_CYCLES", 0.0)
        d = {"launches": launches[k], "waves_per_launch": c.get("SQ_WAVES", 0) / launches[k], "valu_per_wave": c.get("SQ_INSTS_VALU", 0) / w,
             "salu_per_wave": c.get("SQ_INSTS_SALU", 0) / w, "lds_per_wave": c.get("SQ_INSTS_LDS", 0) / w}
        if wc:
            d.update({"wait_any_frac": c.get("SQ_WAIT_ANY", 0) / wc, "wait_inst_any_frac": c.get("SQ_WAIT_INST_ANY", 0) / wc,
                      "active_inst_any_frac": c.get("SQ_ACTIVE_INST_ANY", 0) / wc,
                      "wave_cycles_per_wave": 4.0 * wc / w})      # SQ_*_CYCLES count quad-cycles (MI355X_MICROARCH.md)
        out[k] = d
    return out


CORR = ("gfx950: FETCH_SIZE counts 64 B per 128-B read request (MI355X_MICROARCH.md, HBM section) -> doubled; WRITE_SIZE taken as is; "
        "both in KiB; separate rocprofv3 --pmc passes with --kernel-trace only")
have = [leg for leg in LEGS if glob.glob(os.path.join(SRC, "%s_stats/*/*kernel_stats.csv" % leg))]
sq_all = {}
for leg in have:
    shutil.copy(one("%s_stats/*/*kernel_stats.csv" % leg), os.path.join(DST, "%s_%s_kernel_stats.csv" % (TAG, leg)))
    for c in ("fetch", "write", "sq"):
        f = glob.glob(os.path.join(SRC, "%s_%s/*/*counter_collection.csv" % (leg, c)))
        if f:
            shutil.copy(f[0], os.path.join(DST, "%s_%s_pmc_%s.csv" % (TAG, leg, c.upper())))
    log = open(os.path.join(SRC, "%s_stats.log" % leg)).read().splitlines()
    js = [ln for ln in log if ln.startswith("{")]
    if js:
        open(os.path.join(DST, "%s_%s_under_rocprof.json" % (TAG, leg)), "w").write(js[-1] + "\n")
    s = sq(leg)
    if s:
        sq_all[leg] = s
json.dump({"source": "rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU "
                     "SQ_INSTS_SALU SQ_INSTS_LDS, one pass per bench leg (tools/collect_profiles.sh), %s; raw rows in profiles/%s_*_pmc_SQ.csv" % (TAG, TAG),
           "legs": sq_all}, open(os.path.join(DST, "%s_sq_counters.json" % TAG), "w"), indent=1)

# legs not collected again this round keep their entry (their kernels did not change)
try:
    direct = json.load(open(os.path.join(DST, "pmc_direct_c3.json")))
except Exception:
    direct = {}
direct["source"] = ("rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE; raw rows in profiles/<round>_*_pmc_*.csv (each leg's entry names its round); "
                    "earlier rounds' values in git history")
direct["correction"] = CORR
HEAD = "python3 bench.py --full --no-cpu-baseline --no-tau --no-extra --steps 3 --warmup 1"
for leg, kernel, cmd, cfg in (
        ("headline", "vgx_quad_kernel", HEAD, {"replicates_per_gpu": 16384, "events_per_replicate": 100000, "trajectory_points": 1001}),
        ("spread_occupancy", "vgx_quad_long_kernel", "python3 bench.py --only spread_occupancy",
         {"replicates_per_gpu": 8192, "events_per_replicate": 10000, "occupied": 4096, "mode": "exact"}),
        ("spread_occupancy_fast", "vgx_quadf_kernel", "python3 bench.py --only spread_occupancy_fast",
         {"replicates_per_gpu": 12288, "events_per_replicate": 10000, "occupied": 4096, "mode": "fast"}),
        ("fast_mode", "vgx_quadf_kernel", "python3 bench.py --only fast_mode", {"replicates_per_gpu": 24576, "events_per_replicate": 100000, "mode": "fast"}),
        ("config3_general", "vgx_quadg_kernel_p64", "python3 bench.py --only config3_general", {"replicates_per_gpu": 16384, "events_per_replicate": 50000}),
        ("table3", "vgx_solo_kernel_c2" if TAG >= "r04" else "vgx_quadg_kernel_p16", "python3 bench.py --only table3 --no-cpu-baseline --table3-cells 2:0.001,10:0.001",
         {"replicates_per_gpu": 16384, "events_per_replicate": 50000, "K": 10, "M": 0.001})):
    if leg not in have:
        continue
    fa, wa = pmc(leg, "FETCH_SIZE", True), pmc(leg, "WRITE_SIZE", True)
    # the largest launches of the kernel (a leg may also run it on a small ensemble: fast_mode, table3)
    f, w = fa[kernel], wa[kernel]
    assert f[1] == w[1] and f[1] > 0, (leg, kernel, sorted(fa))
    direct[leg] = {"round": TAG, "command": cmd, "config": cfg, "kernel": kernel, "launches": f[1], "FETCH_SIZE_KiB_per_launch": f[0] / f[1],
                   "WRITE_SIZE_KiB_per_launch": w[0] / w[1], "hbm_bytes_per_launch": (2.0 * f[0] / f[1] + w[0] / w[1]) * 1024}
json.dump(direct, open(os.path.join(DST, "pmc_direct_c3.json"), "w"), indent=1)

if "tau_leap" in have:
    fk, wk = pmc("tau_leap", "FETCH_SIZE"), pmc("tau_leap", "WRITE_SIZE")
    # steps actually run by the leg: every step launches the drift pass once
    steps = max(v[1] for k, v in fk.items() if "drift8" in k)
    kern = {}
    tot = 0.0
    for k in sorted(set(fk) | set(wk)):
        if "vgx_tau" not in k:   # (template instances are listed as "void vgx_tau_...<...>(VgxTauArgs)")
            continue
        rb, wb = 2.0 * fk[k][0] * 1024 / steps, wk[k][0] * 1024 / steps
        kern[k] = {"launches": fk[k][1], "read_bytes_per_step": rb, "write_bytes_per_step": wb}
        tot += rb + wb
    old = json.load(open(os.path.join(DST, "pmc_tau_c4.json")))
    hist = dict(old.get("history", {}))
    prev = old.get("hbm_bytes_per_step")
    if prev and abs(prev - tot) > 1e6 and prev not in hist.values():
        hist["before %s" % TAG] = prev
    json.dump({"source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes, csv), command: python3 bench.py --only tau_leap "
                         "(config 4: the timed 20 steps and the call of 200 steps), %s; raw rows in profiles/%s_tau_leap_pmc_*.csv" % (TAG, TAG),
               "correction": CORR, "config": {"steps": 20, "per_cell": 3}, "steps_profiled": steps,
               "note": "per-step averages over every step the leg runs (its timed call of 20 steps and its call of 200 steps)", "kernels": kern,
               "hbm_bytes_per_step": tot, "history": hist}, open(os.path.join(DST, "pmc_tau_c4.json"), "w"), indent=1)
    print("tau %.3g B/step over %d steps" % (tot, steps))
    for k, v in sorted(kern.items(), key=lambda kv: -(kv[1]["read_bytes_per_step"] + kv[1]["write_bytes_per_step"]))[:8]:
        print("  %-60s %6.2f GB/step" % (k[:60], (v["read_bytes_per_step"] + v["write_bytes_per_step"]) / 1e9))
if "propensity_scan" in have:
    fk, wk = pmc("propensity_scan", "FETCH_SIZE"), pmc("propensity_scan", "WRITE_SIZE")
    ks = [k for k in fk if "vgx_rowscan" in k]
    passes = max(fk[k][1] for k in ks)
    old = json.load(open(os.path.join(DST, "pmc_rowscan.json")))
    fb = sum(2.0 * fk[k][0] * 1024 for k in ks) / passes
    wb = sum(wk[k][0] * 1024 for k in ks) / passes
    old.update({"source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE (and, separately, WRITE_SIZE) --output-format csv -- python3 bench.py --only propensity_scan, %s; "
                          "sums over vgx_rowscan_update_kernel + vgx_rowscan_choose_kernel, %d passes each; FETCH_SIZE doubled (gfx950 correction)" % (TAG, passes),
                "fetch_bytes_per_pass": fb, "write_bytes_per_pass": wb, "hbm_bytes_per_pass": fb + wb})
    json.dump(old, open(os.path.join(DST, "pmc_rowscan.json"), "w"), indent=1)
    print("rowscan %.4g B/pass (algorithmic %.4g)" % (fb + wb, old.get("algorithmic_bytes_per_pass", 0)))
for leg in direct:
    if isinstance(direct[leg], dict):
        print("%-24s %.3g B/launch" % (leg, direct[leg]["hbm_bytes_per_launch"]))
for leg, s in sq_all.items():
    for k, d in s.items():
        if d["waves_per_launch"] > 256:
            print("%-22s %-40s valu/wave %.3g active %.2f wait %.2f" % (leg, k[:40], d["valu_per_wave"], d.get("active_inst_any_frac", 0), d.get("wait_any_frac", 0)))
