"""Scenario ensembles without a device: the kernel choice with several parameter sets installed (``vgx_direct_shape.param_sets``,
through ``vgx_test_direct_plan``) and the checks ``Ensemble`` makes on its scenarios before it creates an engine."""
import copy

import numpy as np
import pytest

import helpers
from test_direct_plan import BIG, CASES, MID, ONE, SMALL, TINY, WIDE
from vgsim_amd import _capi

WAVE = 1


def refused(shape, mode, kernel):
    with pytest.raises(_capi.VgxError) as err:
        _capi.direct_plan(shape, mode=mode, kernel=kernel)
    assert err.value.code == 1
    assert "several parameter sets" in str(err.value)
    return str(err.value)


@pytest.mark.parametrize("shape", [SMALL, MID, WIDE, ONE, TINY, BIG], ids=["small", "mid", "wide", "one", "tiny", "big"])
def test_several_sets_run_on_the_wave_kernel_only(shape):
    s = dict(shape, R=4096, param_sets=3)
    for kernel in (0, 1):
        plan = _capi.direct_plan(s, mode=0, kernel=kernel)
        assert plan == dict(dict.fromkeys(plan, 0), kernel=WAVE)
    for kernel in (2, 3, 4, 5, 6):
        assert "kernel 0 or 1" in refused(s, 0, kernel)
    for mode in (1, 2):
        for kernel in (0, 1):
            assert "mode 0" in refused(s, mode, kernel)


@pytest.mark.parametrize("name,model,change,mode,kernel,want", [c for c in CASES if isinstance(c[5], dict)], ids=lambda v: v if isinstance(v, str) else "")
def test_one_set_is_the_plan_without_the_field(name, model, change, mode, kernel, want):
    """param_sets 0 and 1 change no row of the existing table (every kernel is chosen by some row of it)."""
    shape = dict(model, **change)
    for n in (0, 1):
        assert _capi.direct_plan(dict(shape, param_sets=n), mode=mode, kernel=kernel) == want


def test_the_table_reaches_every_kernel():
    assert {c[5]["kernel"] for c in CASES if isinstance(c[5], dict)} == {1, 2, 3, 4, 5, 6, 7}


# ---- Ensemble's checks, made before the engine exists ----

def make(**ctor):
    from vgsim_amd import Simulator
    kw = dict(number_of_sites=2, populations_number=3, number_of_susceptible_groups=2, seed=1)
    kw.update(ctor)
    with helpers.quiet():
        sim = Simulator(**kw)
    sim.set_population_size(400)
    return sim


def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was created before the scenarios were checked")
    monkeypatch.setattr(_capi, "HipEngine", boom)


def test_scenarios_are_checked_before_the_engine_exists(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    no_engine(monkeypatch)
    base = make()
    good = copy.deepcopy(base)
    good.set_transmission_rate(2.6, haplotype=0)
    bad = {
        "dimensions (sites": make(number_of_sites=1),
        "dimensions (sites, populations": make(populations_number=2),
        "dimensions": make(number_of_susceptible_groups=3),
        "population sizes": copy.deepcopy(base),
        "recombination probability": make(recombination_probability=0.1),
        "genome length": make(genome_length=1000),
        "site positions": copy.deepcopy(base),
        "memory_optimization": make(memory_optimization=True),
    }
    bad["population sizes"].set_population_size(500, population=1)
    bad["site positions"].set_mutation_position(0, 12345)
    for what, sim in bad.items():
        with pytest.raises(ValueError, match=what.split(" (")[0]):
            Ensemble(base, 8, scenarios=[good, sim])
    with pytest.raises(ValueError, match="memory_optimization"):
        Ensemble(make(memory_optimization=True), 8, scenarios=[good])
    with pytest.raises(ValueError, match="one scenario index per replicate"):
        Ensemble(base, 8, scenarios=[base, good], scenario_of=[0, 1, 0])
    for of in ([0, 1, 2, 0, 0, 0, 0, 0], [0, -1, 0, 0, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match=r"integers in \[0, 2\)"):
            Ensemble(base, 8, scenarios=[base, good], scenario_of=of)
    with pytest.raises(ValueError, match="at least one"):
        Ensemble(base, 8, scenarios=[])
    with pytest.raises(ValueError, match="needs scenarios"):
        Ensemble(base, 8, scenario_of=[0] * 8)
    # a valid scenario list passes every check and only then reaches the engine
    with pytest.raises(AssertionError, match="engine was created"):
        Ensemble(base, 8, scenarios=[base, good])


def test_default_map_and_facade_pass_through(monkeypatch):
    from vgsim_amd.ensemble import Ensemble

    class FakeEngine:
        def __init__(self, *a, **k):
            pass
    monkeypatch.setattr(_capi, "HipEngine", FakeEngine)
    base = make()
    a, b, c = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    ens = Ensemble(base, 7, scenarios=[a, b, c])
    assert np.array_equal(ens.scenario_of, np.arange(7) % 3)
    assert [m is s.simulation for m, s in zip(ens.scenarios, (a, b, c))] == [True] * 3
    ens = base.ensemble(4, scenarios=[a, b], scenario_of=[1, 1, 0, 0])
    assert np.array_equal(ens.scenario_of, [1, 1, 0, 0])
    assert Ensemble(base, 4).scenarios is None and Ensemble(base, 4).scenario_of is None
    for call in (lambda: ens.simulate(10, mode='fast'), lambda: ens.simulate(10, kernel='quad'), lambda: ens.simulate_tau(10)):
        with pytest.raises(ValueError, match="scenario ensemble"):
            call()
