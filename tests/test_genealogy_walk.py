"""The backward walk of the device pass (vgsim_amd/csrc/vgx_gwalk.h), compiled for the host and reached through
vgx_test_genealogy_walk: bit for bit the host pass (vgx_get_genealogy) on direct chains — the reference's goldens, random
models, a recombinant chain whose lineages never coalesce — and the same messages for the same failures.  No GPU."""
import copy
import glob
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import assert_genealogy_equal, dense, load
from test_hip_fuzz import build as fuzz_build

GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "genealogy_*.npz"))
              if not os.path.basename(p).startswith("genealogy_tau_"))
KEYS = ("tree", "tree_pop", "times", "mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time",
        "mig_node", "mig_time", "mig_old", "mig_new", "nodes_used", "rng_raw")


def _walk(m, seed, rng_raw=None):
    from vgsim_amd import _capi
    return _capi.genealogy_walk(m, seed, rng_raw=rng_raw)


def _host(m, seed, rng_raw=None):
    from vgsim_amd import _capi
    return _capi.get_genealogy(m, seed, rng_raw=rng_raw)


def assert_same(a, b, what):
    assert set(a) == set(b), what
    for k in KEYS:
        if k in ("nodes_used", "rng_raw"):
            assert a[k] == b[k], "%s %s" % (what, k)
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s %s" % (what, k)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_walk_matches_reference_golden(oracle_mod, path):
    meta, z = load(path)
    sim = helpers.run_case_oracle(oracle_mod, meta["case"])
    m = sim.simulation
    st = oracle_mod.get_state(m)
    raw = tuple(st.rng_final) + (0, 0) if meta["genealogy_seed"] is None else None
    twin = copy.deepcopy(m)
    out = _walk(m, meta["genealogy_seed"], raw)
    assert_genealogy_equal(out, z, meta["case"])
    assert np.array_equal(m.infectious, dense(z["infectious_after_nz"], m.infectious.shape)), "walked-back infectious"
    want = _host(twin, meta["genealogy_seed"], raw)
    assert_same(out, want, meta["case"])
    assert np.array_equal(m.infectious, twin.infectious)


@pytest.mark.parametrize("seed", range(48))
def test_walk_equals_host_pass_on_random_models(oracle_mod, seed):
    sim, n = fuzz_build(seed)
    if oracle_mod.run_direct(sim.simulation, n, 10 ** 9, -1, 200) != 0:
        pytest.skip("zero-weight abort of the reference: no chain")   # (same models every run)
    m = sim.simulation
    st = oracle_mod.get_state(m)
    for gseed, raw in ((None, tuple(st.rng_final) + (0, 0)), (1000 + seed, None)):
        a, b = copy.deepcopy(m), copy.deepcopy(m)
        try:
            want = _host(b, gseed, raw)
        except RuntimeError as e:
            with pytest.raises(RuntimeError) as got:
                _walk(a, gseed, raw)
            assert str(got.value) == str(e)
            continue
        assert_same(_walk(a, gseed, raw), want, "fuzz %d seed %r" % (seed, gseed))
        assert np.array_equal(a.infectious, b.infectious)


def test_walk_reports_lineages_that_never_coalesce(oracle_mod):
    m = helpers.run_case_oracle(oracle_mod, "recomb_a").simulation
    twin = copy.deepcopy(m)
    with pytest.raises(RuntimeError, match="never coalesced") as got:
        _walk(m, 21)
    with pytest.raises(RuntimeError) as want:
        _host(twin, 21)
    assert str(got.value) == str(want.value)


def test_walk_refuses_fewer_than_two_samples(oracle_mod):
    m = helpers.run_case_oracle(oracle_mod, "g9_short").simulation
    m.sCounter = 1
    with pytest.raises(RuntimeError, match="Less than two cases were sampled"):
        _walk(m, 3)


def test_status_messages_are_the_host_passs():
    from vgsim_amd import _capi
    assert _capi.genealogy_message(0, 0) == ""
    assert _capi.genealogy_message(1, 0) == "Less than two cases were sampled..."
    assert _capi.genealogy_message(4, 17) == "vgx_get_genealogy: lineage 17 never coalesced (several roots)"
    assert _capi.genealogy_message(5, 9) == "vgx_get_genealogy: unknown event type 9"
