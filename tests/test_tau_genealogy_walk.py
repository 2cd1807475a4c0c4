"""The backward walk of the device pass for TAU chains (vgsim_amd/csrc/vgx_gwalk_tau.h), compiled for the host and reached through
vgx_test_tau_genealogy_walk and vgx_test_hypergeometric: the three trees recorded from the reference, continued chains and random
models against the host pass vgx_get_genealogy on every key (all six rng_raw words, the walked-back infectious), with the rows of
the trailing steps as they are and de-canonicalised (split and shuffled: what the tau kernels leave), the sampler against numpy,
and the failures.  No GPU."""
import copy
import glob
import os

import numpy as np
import pytest

import helpers
from test_genealogy_golden import assert_genealogy_equal, dense, load
from test_genealogy_walk import assert_same
from test_hip_fuzz import build as fuzz_build

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "genealogy_tau_*.npz")))
B, D, SA, MU, SC, MI, MULTI = range(7)


def _walk(m, seed, rng_raw=None):
    from vgsim_amd import _capi
    return _capi.tau_genealogy_walk(m, seed, rng_raw=rng_raw)


def _host(m, seed, rng_raw=None):
    from vgsim_amd import _capi
    return _capi.get_genealogy(m, seed, rng_raw=rng_raw)


def trailing_steps(m):
    """Index of the first of the chain's trailing MULTITYPE events."""
    ev = m.events
    k = ev.ptr
    while k > 0 and ev.types[k - 1] == MULTI:
        k -= 1
    return k


def decanonicalised(m, seed):
    """A copy of m whose trailing steps hold what the tau kernels leave: every row with num > 1 split into seeded random pieces, each
    step's rows shuffled (the rows of the steps before them stay as they are)."""
    rng = np.random.default_rng(seed)
    out = copy.deepcopy(m)
    ev, mv = out.events, out.multievents
    first = trailing_steps(out)
    k0 = int(ev.haplotypes[first]) if first < ev.ptr else mv.ptr
    cols = {c: list(getattr(mv, c)[:k0]) for c in mv.COLUMNS}
    times = list(mv.times[:k0])
    for e in range(first, ev.ptr):
        j0, j1 = int(ev.haplotypes[e]), int(ev.populations[e])
        rows = []
        for j in range(j0, j1):
            left = int(mv.num[j])
            while True:
                piece = left if left <= 1 or rng.random() < 0.2 else int(rng.integers(1, left))
                rows.append((j, piece))
                left -= piece
                if left == 0:
                    break
        rng.shuffle(rows)
        ev.haplotypes[e] = len(times)
        for j, piece in rows:
            for c in mv.COLUMNS:
                cols[c].append(piece if c == "num" else int(getattr(mv, c)[j]))
            times.append(float(mv.times[j]))
        ev.populations[e] = len(times)
    mv.ptr = 0
    mv.extend(times, **cols)
    return out


def check_against_host(m, seed, raw, what, scramble_seed=5):
    """The hook on m and on its de-canonicalised twin == vgx_get_genealogy on m: every key, or the same exception.  Returns the dict."""
    ref = copy.deepcopy(m)
    try:
        want = _host(ref, seed, raw)
    except RuntimeError as e:
        for twin in (copy.deepcopy(m), decanonicalised(m, scramble_seed)):
            with pytest.raises(RuntimeError) as got:
                _walk(twin, seed, raw)
            assert str(got.value) == str(e), what
        return None
    raw_rows = decanonicalised(m, scramble_seed)
    if trailing_steps(m) < m.events.ptr and (m.multievents.num[:m.multievents.ptr] > 1).any():
        assert raw_rows.multievents.ptr > m.multievents.ptr
    for twin, how in ((copy.deepcopy(m), "canonical rows"), (raw_rows, "split and shuffled rows")):
        got = _walk(twin, seed, raw)
        assert_same(got, want, "%s, %s" % (what, how))
        assert np.array_equal(twin.infectious, ref.infectious), "%s, %s: walked-back infectious" % (what, how)
    return want


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[10:-4] for p in GOLD])
def test_walk_matches_reference_golden(oracle_mod, path):
    meta, z = load(path)
    m = helpers.run_case_oracle(oracle_mod, meta["case"], record_multievents=True).simulation
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    raw = tuple(st.rng_final) + (0, 0) if meta["genealogy_seed"] is None else None
    mv = m.multievents
    # HRUA with Stirling arguments is walked: transmission rows of 10 draws or more, at lineage and infectious counts beyond 126
    assert ((mv.types[:mv.ptr] == B) & (mv.num[:mv.ptr] >= 10)).any() and m.sCounter >= 200 and m.infectious.max() >= 126
    assert trailing_steps(m) < m.events.ptr
    before = m.infectious.copy()
    want = check_against_host(m, meta["genealogy_seed"], raw, meta["case"])
    assert_genealogy_equal(want, z, meta["case"])
    assert np.array_equal(m.infectious, before)
    for twin in (copy.deepcopy(m), decanonicalised(m, 11)):
        assert_genealogy_equal(_walk(twin, meta["genealogy_seed"], raw), z, meta["case"])
        assert np.array_equal(twin.infectious, dense(z["infectious_after_nz"], m.infectious.shape)), "walked-back infectious"


def test_continued_chains(oracle_mod):
    """tau_d (a long direct warm-up with a lockdown, then steps), and a chain whose prefix holds direct events, the rows of an earlier
    tau call and direct events again, then new steps."""
    m = helpers.run_case_oracle(oracle_mod, "tau_d", record_multievents=True).simulation
    helpers.sparse_multievents(m, oracle_mod.get_state(m))
    assert 0 < trailing_steps(m) < m.events.ptr
    assert check_against_host(m, 31, None, "tau_d") is not None
    m = helpers.run_case_oracle(oracle_mod, "tau_then_direct", record_multievents=True).simulation
    assert m.events.types[m.events.ptr - 1] != MULTI
    assert oracle_mod.run_tau(m, 25, 10 ** 12, -1, 200, record_multievents=True) == 0
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    first = trailing_steps(m)
    t = m.events.types[:first]
    assert first < m.events.ptr and (t == MULTI).any() and t[0] != MULTI and t[-1] != MULTI
    assert int(m.events.haplotypes[first]) > 0                       # rows of the earlier call lie in front of the new steps'
    for seed, raw in ((32, None), (None, tuple(st.rng_final) + (0, 0)), (None, tuple(st.rng_final) + (1, 0x9E3779B9))):
        assert check_against_host(m, seed, raw, "tau_then_direct + tau") is not None


# fuzz models whose warm-up the reference completes (no zero-weight abort); all but one (11: a single case) sample enough to walk
FUZZ = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)


@pytest.mark.parametrize("seed", FUZZ)
def test_walk_equals_host_pass_on_random_models(oracle_mod, seed):
    sim, n = fuzz_build(seed)
    m = sim.simulation
    assert oracle_mod.run_direct(m, n, 10 ** 9, -1, 200) == 0
    assert oracle_mod.run_tau(m, 20, 10 ** 12, -1, 200, record_multievents=True) == 0
    st = oracle_mod.get_state(m)
    helpers.sparse_multievents(m, st)
    assert trailing_steps(m) < m.events.ptr
    for gseed, raw in ((None, tuple(st.rng_final) + (0, 0)), (1000 + seed, None)):
        check_against_host(m, gseed, raw, "fuzz %d seed %r" % (seed, gseed), scramble_seed=seed)


def _hand_made(rows_per_step, sCounter=4):
    """One population, one haplotype: two direct samplings, then steps of `rows_per_step` sampling rows of one case each."""
    from vgsim_amd import Simulator
    from vgsim_amd._model import Events, MultiEvents
    with helpers.quiet():
        sim = Simulator(number_of_sites=0, populations_number=1, seed=1)
    m = sim.simulation
    n_rows = sum(rows_per_step)
    ev = Events()
    ev.CreateEvents(2 + len(rows_per_step))
    ev.times[:2], ev.types[:2] = [0.1, 0.2], [SA, SA]
    at = 0
    for k, n in enumerate(rows_per_step):
        ev.times[2 + k], ev.types[2 + k], ev.haplotypes[2 + k], ev.populations[2 + k] = 0.3 + 0.1 * k, MULTI, at, at + n
        at += n
    ev.ptr = 2 + len(rows_per_step)
    mv = MultiEvents()
    step = np.repeat(np.arange(len(rows_per_step)), rows_per_step)
    mv.extend(0.3 + 0.1 * step, num=np.ones(n_rows), types=np.full(n_rows, SA), haplotypes=np.zeros(n_rows), populations=np.zeros(n_rows),
              newHaplotypes=np.zeros(n_rows), newPopulations=np.zeros(n_rows))
    m.events, m.multievents, m.sCounter = ev, mv, sCounter
    m.infectious[:] = 10
    return m


def test_failures_carry_the_python_layers_messages():
    from vgsim_amd import _capi
    few = _hand_made([1, 1], sCounter=1)
    with pytest.raises(RuntimeError) as got:
        _walk(few, 3)
    assert str(got.value) == "Less than two cases were sampled..." == _capi.genealogy_message(1, 0)
    with pytest.raises(RuntimeError) as want:
        _host(copy.deepcopy(few), 3)
    assert str(got.value) == str(want.value)
    # a step over the row bound: status 10 with the step as its argument, the text Ensemble.tau_genealogy raises
    assert _capi.TAU_STEP_ROWS_MAX == 8192 and _capi.GW_STEP_ROWS == 10
    over = _hand_made([3, _capi.TAU_STEP_ROWS_MAX + 1, 2], sCounter=2 + 6 + _capi.TAU_STEP_ROWS_MAX)
    with pytest.raises(RuntimeError) as got:
        _walk(over, 3)
    assert str(got.value) == _capi.genealogy_message(_capi.GW_STEP_ROWS, 1)
    assert "step 1" in str(got.value) and "8192" in str(got.value)
    # the bound itself is walked: 8192 rows of one channel merge into one row
    at = _hand_made([3, _capi.TAU_STEP_ROWS_MAX, 2], sCounter=2 + 5 + _capi.TAU_STEP_ROWS_MAX)
    merged = copy.deepcopy(at)
    mv = merged.multievents
    mv.ptr = 0
    mv.extend([0.3, 0.4, 0.5], num=[3, _capi.TAU_STEP_ROWS_MAX, 2], types=[SA] * 3, haplotypes=[0] * 3, populations=[0] * 3,
              newHaplotypes=[0] * 3, newPopulations=[0] * 3)
    merged.events.haplotypes[2:5], merged.events.populations[2:5] = [0, 1, 2], [1, 2, 3]
    # (no birth in this chain: the sampled lineages never coalesce; both report the same lineage)
    with pytest.raises(RuntimeError, match="never coalesced") as want:
        _host(merged, 3)
    with pytest.raises(RuntimeError) as got:
        _walk(at, 3)
    assert str(got.value) == str(want.value)
    assert _capi.genealogy_message(11, 9) == "vgx_get_genealogy: unknown multievent type 9"


# (good, bad, sample): both sides of the HRUA threshold on `sample` and on `total - sample`, good > bad and good < bad,
# sample > total / 2, Stirling arguments (>= 126), no good item
HYPER_SETS = [(40, 60, 9), (40, 60, 10), (60, 40, 91), (60, 40, 90), (7, 300, 150), (300, 7, 150), (30, 50, 70),
              (500, 900, 300), (20000, 3000, 9000), (126, 126, 126), (0, 50, 20), (0, 5, 3), (999999999, 999999999, 7),
              (999999999, 500000000, 700000000)]
# totals above 2^32: numpy's Generator refuses arguments of 10^9 or more, so these sets (the 64-bit path of random_interval below
# 10 draws, HRUA above) are compared with the oracle's restatement of the same sampler (oracle/vgx_oracle_genealogy.c, itself
# pinned on numpy by test_genealogy_golden.py::test_hypergeometric_matches_numpy)
HYPER_SETS_WIDE = [(2 ** 33, 2 ** 32, 8), (3, 2 ** 33, 9), (2 ** 32 + 5, 4, 2 ** 32 + 3), (3, 2 ** 33, 2 ** 32 + 5),
                   (2 ** 34, 2 ** 33, 5000), (5000, 2 ** 34, 2 ** 33)]
HYPER_DRAWS = 10 ** 4


def numpy_state(seed, has32=False, spare=0):
    bg = np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(0,)))
    s = bg.state
    s["has_uint32"], s["uinteger"] = int(has32), int(spare)
    bg.state = s
    return bg


def state_words(bg):
    s = bg.state
    st, inc = s["state"]["state"], s["state"]["inc"]
    m = 2 ** 64 - 1
    return (st >> 64, st & m, inc >> 64, inc & m, int(s["has_uint32"]), int(s["uinteger"]))


def hyper_starts(good):
    """Two start states per parameter set: without and with a buffered 32-bit half."""
    return [state_words(numpy_state(seed + good % 1000, has32, 0xDEADBEEF)) for seed, has32 in ((7, False), (8, True))]


@pytest.mark.parametrize("good,bad,sample", HYPER_SETS)
def test_hypergeometric_matches_numpy(good, bad, sample):
    """Values and final generator state (the buffered 32-bit half included) of 10^4 draws per parameter set.  numpy calls libm's log,
    the sampler the engine's own: a draw could differ only where a comparison is decided within the last ulp of a logarithm; none
    of these sets has such a draw."""
    from vgsim_amd import _capi
    for seed, has32 in ((7, False), (8, True)):
        bg = numpy_state(seed + good % 1000, has32, 0xDEADBEEF)
        start = state_words(bg)
        want = np.random.Generator(bg).hypergeometric(good, bad, sample, size=HYPER_DRAWS)
        got, end = _capi.hypergeometric(good, bad, sample, HYPER_DRAWS, start)
        assert np.array_equal(got, want), (good, bad, sample, int(np.argmax(got != want)))
        assert end == state_words(bg), (good, bad, sample)


@pytest.mark.parametrize("good,bad,sample", HYPER_SETS_WIDE)
def test_hypergeometric_above_32_bits_matches_the_oracle(oracle_mod, good, bad, sample):
    import ctypes as C
    from vgsim_amd import _capi
    lib = oracle_mod.lib()
    lib.vgo_hypergeometric.restype = C.c_int64
    for start in hyper_starts(good):
        r = oracle_mod.VgoGenRng()
        r.g.state_hi, r.g.state_lo, r.g.inc_hi, r.g.inc_lo, r.has_uint32, r.uinteger = start
        want = [int(lib.vgo_hypergeometric(C.byref(r), C.c_int64(good), C.c_int64(bad), C.c_int64(sample))) for _ in range(HYPER_DRAWS)]
        got, end = _capi.hypergeometric(good, bad, sample, HYPER_DRAWS, start)
        assert got.tolist() == want, (good, bad, sample)
        assert end == (r.g.state_hi, r.g.state_lo, r.g.inc_hi, r.g.inc_lo, r.has_uint32, r.uinteger), (good, bad, sample)
        assert 0 <= got.min() and got.max() <= min(good, sample)


def _more_migrants_than_sources():
    """Two populations, one haplotype.  Step 0: the one case of population 0 infects three hosts of population 1 (a MIGRATION row with
    num = 3); step 1: it is sampled, and so are two cases of population 1.  Walking back, two of the migration's three targets are
    sampled lineages (say), to be thinned against a source compartment that holds ONE case: numpy's hypergeometric raises on
    sample > good + bad, and vgx_get_genealogy, which does not check, goes on to pop from an empty list."""
    from vgsim_amd import Simulator
    from vgsim_amd._model import Events, MultiEvents
    with helpers.quiet():
        sim = Simulator(number_of_sites=0, populations_number=2, seed=1)
    m = sim.simulation
    ev = Events()
    ev.CreateEvents(2)
    ev.times[:2], ev.types[:2], ev.haplotypes[:2], ev.populations[:2] = [0.1, 0.2], [MULTI, MULTI], [0, 1], [1, 3]
    ev.ptr = 2
    mv = MultiEvents()
    mv.extend([0.1, 0.2, 0.2], num=[3, 1, 3], types=[MI, SA, SA], haplotypes=[0, 0, 0], populations=[0, 0, 1], newHaplotypes=[0, 0, 0],
              newPopulations=[1, 0, 0])
    m.events, m.multievents, m.sCounter = ev, mv, 4
    m.infectious[:] = [[0], [0]]
    return m


def test_a_row_numpy_would_refuse_is_a_status_not_a_walk_off_the_lists():
    """All three targets are sampled lineages here (population 1 ends empty), so the first draw takes all three for certain; the source
    compartment holds one case and one lineage: hypergeometric(1, 0, 3)."""
    from vgsim_amd import _capi
    m = _more_migrants_than_sources()
    before = m.infectious.copy()
    with pytest.raises(RuntimeError) as got:
        _walk(m, 3)
    assert str(got.value) == _capi.genealogy_message(12, 0)
    assert str(got.value).startswith("vgx_get_tau_genealogies:") and "event 0" in str(got.value)
    assert m.infectious.shape == before.shape
