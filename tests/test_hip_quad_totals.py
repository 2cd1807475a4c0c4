"""Per-population totals of the exact row kernel (vgx_quad.hip keeps totalSusceptible, totalInfectious and globalInfectious as
doubles: whole numbers below 2^53, exact) on models whose host counts do not fit 32 bits: runs with the kernel forced to `quad`,
bit for bit against the CPU oracle, each with accepted migrations and a Restart (two attempts die out within 100 events)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

BEYOND_2_31 = [3000000017, 5000000011, 2 ** 32 + 12345]                              # every population above 2^31 hosts
BELOW_2_31 = [2 ** 31 - 1, 2 ** 31 - 19, 2 ** 31 - 61, 2 ** 31 - 69, 2 ** 31 - 85]   # the largest the one-class form takes: 2^33.3 in all
EVENTS = 6000


def _model(sizes, seed=3):
    from vgsim_amd import Simulator
    with helpers.quiet():
        s = Simulator(number_of_sites=2, populations_number=len(sizes), number_of_susceptible_groups=1, seed=seed)
    s.set_transmission_rate(1.6)
    s.set_recovery_rate(0.9)
    s.set_sampling_rate(0.1)
    s.set_mutation_rate(0.05)
    s.set_total_migration_probability(0.3)
    for i, n in enumerate(sizes):
        s.set_population_size(n, population=i)
    return s


def _pair(oracle_mod, sizes):
    hip = _model(sizes)
    with helpers.quiet():
        hip.simulate(iterations=EVENTS, sample_size=10 ** 9, kernel="quad")
    ref = _model(sizes)
    assert oracle_mod.run_direct(ref.simulation, EVENTS, 10 ** 9, -1, 200) == 0
    return hip.simulation, ref.simulation


def _check(hip, ref, what):
    assert ref.events.ptr == EVENTS and ref.good_attempt > 1, "the case must contain a Restart"
    assert ref.migPlus > 100, "the case must contain accepted migrations"
    helpers.assert_models_equal(hip, ref, what)
    assert int(hip.susceptible.sum()) + int(hip.infectious.sum()) > 2 ** 32


def test_population_sizes_beyond_2_31_vs_oracle(oracle_mod):
    """Every population above 2^31 hosts, kernel forced to `quad`.  (The one-class form streams 4-byte haplotype counts, so the host
    hands populations of 2^31 hosts and more to the general form of the row kernel, which shares the prefix chains.)"""
    hip, ref = _pair(oracle_mod, BEYOND_2_31)
    assert hip._engine.last_kernel in ("quad", "quadg")
    _check(hip, ref, "beyond 2^31")


def test_one_class_form_totals_beyond_32_bits_vs_oracle(oracle_mod):
    """The largest populations the one-class form takes (just below 2^31 each, more than 2^33 hosts in all): vgx_quad_kernel itself,
    totals around 2^31 and their sum in the doubles."""
    hip, ref = _pair(oracle_mod, BELOW_2_31)
    assert hip._engine.last_kernel == "quad"
    _check(hip, ref, "below 2^31")


def test_plain_division_switch_gives_the_same_run(oracle_mod, monkeypatch):
    """VGX_SOLO_PLAIN_DIV=1 selects the instantiation that divides BirthRate's terms by actualSizes with the division instead of the
    reciprocal sequence: the same run, bit for bit."""
    monkeypatch.setenv("VGX_SOLO_PLAIN_DIV", "1")
    hip, ref = _pair(oracle_mod, BELOW_2_31)
    assert hip._engine.last_kernel == "quad"
    _check(hip, ref, "plain division")
