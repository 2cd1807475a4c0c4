"""Two calls of c3_s5_p16, R = 4096, 10^5 events on the wavefront kernel, to be run under a profiler (profiles/param_sets_sq.json):

    python tools/run_param_sets_one.py plain|sets

'plain' is the plain ensemble, 'sets' the scenario form with 64 copies of the same set (tools/probe_param_sets.py times both)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import helpers
import models
from vgsim_amd import Simulator
from vgsim_amd.ensemble import Ensemble

with helpers.quiet():
    sim, phases = models.build(Simulator, "c3_s5_p16")
    phases[0][0](sim)
R = 4096
seeds = 1000 + np.arange(R, dtype=np.int64)
kw = {"scenarios": [sim] * 64} if sys.argv[1] == "sets" else {}
ens = Ensemble(sim, R, seeds=seeds, **kw)
for _ in range(2):
    res = ens.simulate(100000, sample_size=10 ** 12, record_events=False, kernel='wave')
    print(sys.argv[1], ens.engine.last_kernel, res.kernel_ms, int(res.events.sum()), flush=True)
ens.close()
