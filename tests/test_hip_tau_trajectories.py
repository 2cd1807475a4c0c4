"""Summary trajectories of tau-leaping ensembles (Ensemble.simulate_tau(traj_points=T, traj_window=(t0, t1))), on both tau paths:
the on-device step loop of small models (vgx_taus.hip, VGX_TAU_STEP_KERNELS=0) and the step kernels (vgx_tau.hip, =1).

Grid point j is g_j = t0 + j dt, dt = (t1 - t0) / (T - 1) (0 when T = 1), as for direct calls.  A step that takes the time from t to t'
(the time of its MULTITYPE record) writes every grid point not yet written with g_j < t' with the totals before the step; the call's end
writes the remaining ones with the final totals; a Restart starts the grid again on the restored state.  So the bins of a replicate are
a replay of its own log from the call's start state, and the tests below compare them with that replay with no tolerance."""
import ctypes as C

import numpy as np
import pytest

import helpers
import models

pytestmark = pytest.mark.gpu

BIRTH, DEATH, SAMPLING, MUTATION, SUSCCHANGE, MIGRATION = range(6)
PATHS = {"loop": "0", "steps": "1"}


def _grid(window, T):
    t0, t1 = float(window[0]), float(window[1])
    dt = (t1 - t0) / (T - 1) if T > 1 else 0.0
    return t0 + np.arange(T) * dt


def _totals(m):
    return np.asarray(m.infectious, dtype=np.int64).sum(axis=1), np.asarray(m.susceptible, dtype=np.int64).sum(axis=1)


def call_chain(ens, r):
    """The MULTITYPE records of replicate r written by the last call: (6, steps)."""
    return ens.replicate_events(r)[:, int(ens.engine.counters(r).ev_first_new):]


def replay(ens, r, start, window, T):
    """The bins of replicate r as its MULTITYPE records and their multievent rows give them, from the totals `start` (I[P], S[P])."""
    chain = call_chain(ens, r)
    rows = ens.engine.multievents(r)
    inf, sus = start[0].copy(), start[1].copy()
    grid = _grid(window, T)
    P = len(inf)
    out = np.empty((T, P, 2), dtype=np.float64)
    j = 0
    for k in range(chain.shape[1]):
        assert chain[1, k] == 6   # MULTITYPE
        t_new, m0, m1 = chain[0, k], int(chain[2, k]), int(chain[3, k])
        while j < T and grid[j] < t_new:
            out[j, :, 0], out[j, :, 1] = inf, sus
            j += 1
        ty, n = rows["types"][m0:m1], rows["num"][m0:m1]
        pop, npop = rows["populations"][m0:m1], rows["newPopulations"][m0:m1]
        for kinds, where, sign in (((BIRTH,), pop, 1), ((DEATH, SAMPLING), pop, -1), ((MIGRATION,), npop, 1)):
            sel = np.isin(ty, kinds)
            d = np.zeros(P, dtype=np.int64)
            np.add.at(d, where[sel], n[sel])
            inf += sign * d
            sus -= sign * d
    out[j:, :, 0], out[j:, :, 1] = inf, sus
    return out, (inf, sus), chain


def check_replay(ens, traj, start, window, T):
    """Every replicate's bins equal the replay of its log; the replay's end state is the replicate's state (the rules are right).
    (A replicate that restarted replays its final attempt from the initial state: the callers' start state where they restart.)"""
    assert traj.shape == (ens.R, T, ens.model.popNum, 2)
    for r in range(ens.R):
        want, end, _ = replay(ens, r, start, window, T)
        fin = _totals(ens.replicate_state(r))
        assert np.array_equal(end[0], fin[0]) and np.array_equal(end[1], fin[1]), "replicate %d: the replay does not end in its state" % r
        assert np.array_equal(traj[r], want), "replicate %d: bins differ from the replay of its log" % r


def warm(name):
    """A case of tests/models.py after its direct warm-up (phase 0)."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim, phases = models.build(Simulator, name)
        setup, kw = phases[0]
        setup(sim)
        sim.simulate(**kw)
    return sim, phases[1][1]["iterations"]


def window_of(ens, times_of, T):
    """A window that starts before the call's start time and ends after every replicate's last step."""
    t_start = float(ens.model.currentTime)
    t_last = max(times_of)
    span = max(t_last - t_start, 1e-3)
    return (t_start - 0.2 * span, t_last + 0.2 * span)


def last_times(ens):
    out = []
    for r in range(ens.R):
        ch = call_chain(ens, r)
        out.append(float(ch[0, -1]) if ch.shape[1] else float(ens.model.currentTime))
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_bins_equal_the_replay_of_the_log(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: every replicate's bins are the replay of its own log (T = 33 over a window around
    the call, and T = 1); without the event log the same seeds give the same bins and the same final states."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=np.array([3, 17, 101, 4242, 9, 77], dtype=np.int64))
    start = _totals(ens.model)
    res0 = ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    assert ens.traj_shape is None and all(call_chain(ens, r).shape[1] > 1 for r in range(ens.R))
    win = window_of(ens, last_times(ens), 33)
    assert win[0] < ens.model.currentTime
    for T in (33, 1):
        res = ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True, traj_points=T, traj_window=win)
        assert np.array_equal(res.events, res0.events)
        traj = ens.trajectories()
        check_replay(ens, traj, start, win, T)
        if T == 33:
            # the grid really cuts through the steps: bins change inside the window
            assert any(not np.array_equal(traj[r, 1], traj[r, -2]) for r in range(ens.R))
            states = [_totals(ens.replicate_state(r)) + (ens.replicate_state(r).currentTime,) for r in range(ens.R)]
            # without the event log: the same states first (the bins are compared with the logged run's), then the same bins
            ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False, traj_points=T, traj_window=win)
            for r in range(ens.R):
                st = ens.replicate_state(r)
                fin = _totals(st)
                assert np.array_equal(fin[0], states[r][0]) and np.array_equal(fin[1], states[r][1]) and st.currentTime == states[r][2], r
            assert np.array_equal(ens.trajectories(), traj)
    ens.close()


def _c4_scaled(seed, sparse=False):
    """The recipe of bench.py's config-4 leg at 7 sites x 4 populations (as tests/test_hip_tau.py builds it).  sparse: one compartment
    in 64 occupied (the step kernels then draw over the lists of occupied compartments)."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        s = Simulator(number_of_sites=7, populations_number=4, seed=seed)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.01)
    s.set_total_migration_probability(0.01); s.set_population_size(10 ** 7)
    m = s.simulation
    if sparse:
        m.infectious[:] = 0
        m.infectious[:, ::64] = 40
    else:
        m.infectious[:] = 3
    m.susceptible[:, 0] -= m.infectious.sum(axis=1)
    m.totalInfectious[:] = m.infectious.sum(axis=1)
    m.totalSusceptible[:] = m.susceptible.sum(axis=1)
    m.globalInfectious = int(m.totalInfectious.sum())
    m.first_simulation = True
    m.initial_infectious[:] = m.infectious
    m.initial_susceptible[:] = m.susceptible
    return s


def engine_call(ens, nt, T, window, record=True, dense=0, stage=False):
    """Ensemble.simulate_tau through the C ABI with the step kernels' validation modes: vgx_run_opts.reserved[1] = 1 / 2 (dense tries:
    the bounds check as a pass of its own / fused), stage: the start state put on the device by vgx_stage_tau first."""
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import EnsembleResult
    m, eng = ens.model, ens.engine
    ptr, size = m.events.ptr, m.events.size
    for _ in range(2):
        size = size + nt if ptr == 0 else max(size, ptr + nt)
    eng.set_params(m)
    saved = (m.events.ptr, m.events.size)
    m.events.size = size
    try:
        eng.set_state(m)
    finally:
        m.events.ptr, m.events.size = saved
    eng.set_seeds(ens.seeds)
    if stage:
        eng.stage_tau()
    o = _capi.VgxRunOpts()
    o.record_events = 1 if record else 0
    o.traj_points = T
    o.traj_t0, o.traj_t1 = float(window[0]), float(window[1])
    o.reserved[1] = dense
    eng._check(eng.lib.vgx_simulate_tau(eng.handle, nt, 10 ** 12, -1.0, 200, C.byref(o)))
    res = EnsembleResult(ens.R)
    call = eng.counters_all()
    res.events[:], res.loop_iterations[:], res.restarts[:] = call[:, 0], call[:, 1], call[:, 2]
    traj = np.empty((ens.R, T, m.popNum, 2), dtype=np.float64)
    eng._check(eng.lib.vgx_get_trajectories(eng.handle, traj.ctypes.data_as(C.c_void_p), 0))
    return res, traj


@pytest.mark.parametrize("mode", ["R1", "R4", "R1:sparse", "R4:sparse", "R1:dense1", "R2:dense2", "R1:staged"])
def test_step_kernels_at_scale(mode, monkeypatch):
    """The step kernels on the scaled config-4 state: one replicate (the front pass alone and the speculative rounds of a step), four
    (one synchronisation per try for all of them), a sparse state (tries over the lists of occupied compartments), the dense tries of
    vgx_run_opts.reserved[1] and a start state staged by vgx_stage_tau: the bins are the replay of every replicate's log."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", "1")
    R = int(mode.split(":")[0][1:])
    kind = mode.split(":")[1] if ":" in mode else ""
    base = _c4_scaled(11, sparse=kind == "sparse")
    ens = Ensemble(base, R, seeds=70000 + np.arange(R, dtype=np.int64))
    start = _totals(ens.model)
    nt = 3     # tau as the first call of a model: capacity 2 x iterations (pyx:2298, 2306) -> 6 leaps
    dense = {"dense1": 1, "dense2": 2}.get(kind, 0)
    res0, _ = engine_call(ens, nt, 1, (-1.0, -1.0), dense=dense, stage=kind == "staged")
    assert (res0.events == 2 * nt).all()
    win = window_of(ens, last_times(ens), 33)
    res, traj = engine_call(ens, nt, 33, win, dense=dense, stage=kind == "staged")
    assert np.array_equal(res.events, res0.events)
    check_replay(ens, traj, start, win, 33)
    assert not np.array_equal(traj[0, 1], traj[0, -2])
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_restarts_rebin_the_final_attempt(path, monkeypatch):
    """Attempts that die out within 100 records restart the replicate (pyx:714-738) on the initial state at time 0: its bins start again
    there and describe the final attempt, as its log does."""
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    with helpers.quiet():
        sim = Simulator(number_of_sites=1, populations_number=1, seed=5)
    sim.set_transmission_rate(1.1); sim.set_recovery_rate(0.9); sim.set_sampling_rate(0.1)
    m = sim.simulation
    assert int(m.globalInfectious) == 0 and not m.first_simulation
    ens = Ensemble(sim, 8, seeds=500 + np.arange(8, dtype=np.int64))
    start = _totals(ens.model)
    start[0][0] += 1       # the first call's index case (PrepareParameters): the initial state every Restart restores
    start[1][0] -= 1
    win = (-0.5, 6.0)
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True, traj_points=33, traj_window=win)
    assert res.restarts.max() > 0
    check_replay(ens, ens.trajectories(), start, win, 33)
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_time_limit_and_no_attempts(path, monkeypatch):
    """A time limit inside the window: the grid points after the last step hold the final state.  attempts=0: the call never starts and
    every grid point holds the start state."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 4, seeds=np.array([1, 2, 3, 4], dtype=np.int64))
    start = _totals(ens.model)
    t0 = float(ens.model.currentTime)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    t_end = min(last_times(ens))
    steps_full = [call_chain(ens, r).shape[1] for r in range(ens.R)]
    limit = float(np.float32(t0 + 0.5 * (t_end - t0)))
    win = (t0 - 0.1, t_end)
    ens.simulate_tau(nt, sample_size=10 ** 12, epidemic_time=limit, record_events=True, traj_points=33, traj_window=win)
    traj = ens.trajectories()
    check_replay(ens, traj, start, win, 33)
    grid = _grid(win, 33)
    lasts = last_times(ens)
    for r in range(ens.R):
        last = lasts[r]
        assert last >= limit and call_chain(ens, r).shape[1] < steps_full[r]   # (stopped by the limit)
        fin = _totals(ens.replicate_state(r))
        after = grid >= last
        assert after.sum() > 1
        assert (traj[r, after, :, 0] == fin[0]).all() and (traj[r, after, :, 1] == fin[1]).all()
    ens.simulate_tau(nt, sample_size=10 ** 12, attempts=0, record_events=True, traj_points=33, traj_window=win)
    traj = ens.trajectories()
    assert (traj[..., 0] == start[0]).all() and (traj[..., 1] == start[1]).all()
    ens.close()


def test_read_out_and_gather(tmp_path):
    """trajectories(out=<cuda tensor>), the single-rank gather (float64 and the int32 wire format, on the host and on the device) and
    Simulator.simulate_ensemble(method='tau') all give the bins trajectories() reads.  (A process of its own, in which torch takes the
    GPU first, as the RCCL test of tests/test_hip_ensemble.py does.)"""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "readout.py"
    script.write_text(textwrap.dedent("""
        import os, sys
        import numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        torch.cuda.set_device(0)
        from test_hip_tau_trajectories import warm
        sim, nt = warm("tau_c")
        P = sim.simulation.popNum
        ens = sim.ensemble(5, seeds=np.arange(5, dtype=np.int64) + 40)
        t0 = float(sim.simulation.currentTime)
        win = (t0 - 0.1, t0 + 2.0)
        ens.simulate_tau(nt, sample_size=10 ** 12, traj_points=17, traj_window=win)
        ref = ens.trajectories()
        assert ref.shape == (5, 17, P, 2)
        dev = torch.empty(ref.shape, dtype=torch.float64, device="cuda")
        assert ens.trajectories(out=dev) is dev
        assert np.array_equal(dev.cpu().numpy(), ref)
        for device in (None, "cuda"):
            g = ens.gather_trajectories(dst=0, device=device)
            assert g.shape == (1,) + ref.shape and g.dtype == torch.float64 and g.is_cuda == (device is not None)
            assert np.array_equal(g[0].cpu().numpy(), ref)
            g32 = ens.gather_trajectories(dst=0, wire_dtype=torch.int32, device=device)
            assert g32.dtype == torch.int32 and np.array_equal(g32[0].cpu().numpy(), ref.astype(np.int32))
        ens.close()
        ens2, res = sim.simulate_ensemble(3, nt, sample_size=10 ** 12, method='tau', traj_points=9, traj_window=win)
        assert ens2.trajectories().shape == (3, 9, P, 2)
        ens2.close()
        print("READOUT_OK")
    """) % (root, root))
    p = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b"READOUT_OK" in p.stdout, p.stdout.decode()[-3000:]


def _big_sparse_model():
    """More occupied compartments than the direct kernels' preparation of a tau call takes (2^18): the tau call makes no direct call."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        s = Simulator(number_of_sites=8, populations_number=5, seed=13)
    s.set_transmission_rate(2.5); s.set_recovery_rate(0.9); s.set_sampling_rate(0.1); s.set_mutation_rate(0.01)
    s.set_population_size(10 ** 7)
    m = s.simulation
    m.infectious[:] = 1
    m.susceptible[:, 0] -= m.infectious.sum(axis=1)
    m.totalInfectious[:] = m.infectious.sum(axis=1)
    m.totalSusceptible[:] = m.susceptible.sum(axis=1)
    m.globalInfectious = int(m.totalInfectious.sum())
    m.first_simulation = True
    m.initial_infectious[:] = m.infectious
    m.initial_susceptible[:] = m.susceptible
    return s


@pytest.mark.parametrize("case", ["tau_b", "big"])
def test_no_stale_bins_after_a_tau_call(case):
    """A direct call with trajectories, then a tau call without: nothing to read, from Python or from the C ABI."""
    from vgsim_amd.ensemble import Ensemble
    sim = _big_sparse_model() if case == "big" else warm(case)[0]
    ens = Ensemble(sim, 1 if case == "big" else 3)
    ens.simulate(5 if case == "big" else 200, traj_points=8, traj_window=(0.0, 10.0))
    assert ens.trajectories().shape[1] == 8
    ens.simulate_tau(2, sample_size=10 ** 12)
    with pytest.raises(RuntimeError):
        ens.trajectories()
    out = np.zeros((ens.R, 8, sim.simulation.popNum, 2))
    assert ens.engine.lib.vgx_get_trajectories(ens.engine.handle, out.ctypes.data_as(C.c_void_p), 0) != 0
    assert (out == 0).all()
    ens.close()
