"""Scenario ensembles on the tau path without a device: what ``Ensemble.simulate_tau`` checks and hands to the engine before the library
runs (the contact-density check it shares with ``simulate``, ``scenario_of``, the parameter sets), on a stand-in engine that records
the calls it gets."""
import copy

import numpy as np
import pytest

import helpers
from vgsim_amd import _capi


def make():
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=2, populations_number=3, number_of_susceptible_groups=2, seed=1)
    sim.set_population_size(400)
    sim.set_npi([0.2, 0.02, 0.004])
    return sim


class Reached(Exception):
    """The stand-in engine was asked to run: every Python-side check has passed."""


class FakeEngine:
    def __init__(self, *a, **k):
        self.calls = []

    def set_params(self, m):
        self.calls.append(("set_params", m))

    def set_param_sets(self, models, set_of):
        self.calls.append(("set_param_sets", list(models), np.array(set_of)))

    def set_state(self, m):
        self.calls.append(("set_state", m))

    def set_seeds(self, seeds):
        self.calls.append(("set_seeds", np.array(seeds)))

    @property
    def lib(self):
        raise Reached()


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(_capi, "HipEngine", FakeEngine)


def run(ens, call):
    return ens.simulate(50) if call == "simulate" else ens.simulate_tau(50, per_scenario=True)


def scenario_ensemble(R=6, scenario_of=None):
    from vgsim_amd.ensemble import Ensemble
    base = make()
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    b.set_transmission_rate(2.6, haplotype=0)
    b.set_npi([0.5, 0.05, 0.01], population=1)
    return base, a, b, Ensemble(base, R, scenarios=[a, b], scenario_of=scenario_of)


@pytest.mark.parametrize("call", ["simulate", "simulate_tau"])
def test_both_simulate_calls_install_the_parameter_sets(fake, call):
    base, a, b, ens = scenario_ensemble(scenario_of=[1, 1, 0, 0, 1, 0])
    with pytest.raises(Reached):
        run(ens, call)
    names = [c[0] for c in ens.engine.calls]
    assert names == ["set_param_sets", "set_state", "set_seeds"]
    _, models, set_of = ens.engine.calls[0]
    assert models[0] is a.simulation and models[1] is b.simulation
    assert np.array_equal(set_of, [1, 1, 0, 0, 1, 0])
    assert ens.engine.calls[1][1] is base.simulation       # the start state is the base simulator's


def test_simulate_tau_runs_scenarios_when_asked(fake):
    """The message of the parent commit is gone: a call that asks for the scenarios reaches the engine, one that does not is told
    how to ask (before the engine is touched), and a plain ensemble cannot ask."""
    from vgsim_amd.ensemble import Ensemble
    _, _, _, ens = scenario_ensemble()
    with pytest.raises(Reached):
        ens.simulate_tau(50, per_scenario=True)
    ens.engine.calls.clear()
    with pytest.raises(ValueError, match="scenario ensemble.*per_scenario=True") as err:
        ens.simulate_tau(50)
    assert "runs one parameter set only" not in str(err.value) and "has no simulate_tau" not in str(err.value)
    assert ens.engine.calls == []
    with pytest.raises(ValueError, match="needs a scenario ensemble"):
        Ensemble(make(), 4).simulate_tau(50, per_scenario=True)


@pytest.mark.parametrize("call", ["simulate", "simulate_tau"])
def test_contact_density_mismatch_is_refused_by_both_calls(fake, call):
    base, a, b, ens = scenario_ensemble()
    b.simulation.contactDensity[1] = 0.7       # neither its before- nor its after-lockdown value
    with pytest.raises(ValueError) as err:
        run(ens, call)
    assert str(err.value) == ("scenario 1: the contact density of population 1 is 0.7, its own settings give 1.0 for the lockdown "
                              "state of the start state")
    assert ens.engine.calls == []              # refused before the engine is touched
    # the lockdown state is the START state's: with population 1 locked down there, the scenario's after-lockdown value is the one
    b.simulation.contactDensity[1] = 0.5
    with pytest.raises(ValueError, match=r"scenario 1: the contact density of population 1 is 0.5, its own settings give 1.0"):
        run(ens, call)
    base.simulation.lockdownON[1] = 1
    a.simulation.contactDensity[1] = 0.2
    with pytest.raises(Reached):
        run(ens, call)


def test_the_check_is_one_helper(fake, monkeypatch):
    """``simulate`` and ``simulate_tau`` call the same check: a scenario that one refuses the other refuses, through one method."""
    from vgsim_amd.ensemble import Ensemble
    seen = []
    monkeypatch.setattr(Ensemble, "_check_scenario_contact_densities", lambda self: seen.append(self))
    _, _, _, ens = scenario_ensemble()
    for call in ("simulate", "simulate_tau"):
        with pytest.raises(Reached):
            run(ens, call)
    assert seen == [ens, ens]
    plain = Ensemble(make(), 4)
    for call in ("simulate", "simulate_tau"):
        with pytest.raises(Reached):
            getattr(plain, call)(50)
    assert seen == [ens, ens] and [c[0] for c in plain.engine.calls[:1]] == ["set_params"]


def test_scenario_of_is_validated_before_the_engine_exists(monkeypatch):
    from vgsim_amd.ensemble import Ensemble

    def boom(*a, **k):
        raise AssertionError("the engine was created before the scenarios were checked")
    monkeypatch.setattr(_capi, "HipEngine", boom)
    base = make()
    other = copy.deepcopy(base)
    with pytest.raises(ValueError, match="one scenario index per replicate"):
        Ensemble(base, 6, scenarios=[base, other], scenario_of=[0, 1])
    for of in ([0, 1, 2, 0, 0, 0], [0, -1, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match=r"integers in \[0, 2\)"):
            Ensemble(base, 6, scenarios=[base, other], scenario_of=of)


def test_tau_analytics_take_the_scenario_groups(fake):
    """What the tau analytics hand to the summaries: the scenario map and count of a scenario ensemble, (None, 1) of a plain one."""
    from vgsim_amd.ensemble import Ensemble, _summary_groups
    _, _, _, ens = scenario_ensemble(scenario_of=[1, 1, 0, 0, 1, 0])
    of, n = ens._scenario_groups()
    assert n == 2 and np.array_equal(of, [1, 1, 0, 0, 1, 0])
    group_of, G = _summary_groups('auto', None, ens.R, of, n)
    assert G == 2 and np.array_equal(group_of, [1, 1, 0, 0, 1, 0])
    assert Ensemble(make(), 4)._scenario_groups() == (None, 1)
