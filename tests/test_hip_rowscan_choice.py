"""K3's two kernels (vgx_rowscan.hip behind ``vgx_propensity_scan``) at the places their structure can go wrong, driven through
``_capi.propensity_scan`` only.  One workgroup of 256 threads walks a row in tiles of 1024 entries, four consecutive entries per
thread, 64 threads per wavefront, so an entry's running sum comes from its thread's registers, from the thread before (a lane
shuffle), from the wavefront before (LDS) or from the tiles before (the carry).  The weights are fed bit for bit (bRate = 0,
rates123[..., 0] = w, infectious = 1 give hapPopRate == w; every test asserts that first) and the choice is compared with host
arithmetic on those known weights, never with the kernel's own intermediate values:

  1. exact arithmetic (integer weights, a power-of-two total, r a half-integer): the index and rnOut of a literal fastChoose
     (fast_choose.pxi:18-31) bit for bit, with r just inside every target entry, exactly at its end (a tie: the strict `<` of
     fast_choose.pxi:26 keeps the entry) and just past it, for every lane, wavefront and tile border and every pattern of zeros;
  2. rounded arithmetic (doubles of 1e-8 .. 1e8 in one row): r swept ulp by ulp across boundaries; the chosen entry has a
     positive weight, rnOut is finite, and entry and rnOut are right within the rounding of the kernel's own sums (D below);
  3. the update kernel: counts up to 2^63, both of its code paths elementwise bit for bit, subnormal and 1e300 magnitudes, the
     row total against math.fsum within its rounding (D_u below), a row of total 0 between two others;
  4. the entry points: the measuring call returns the first row's outputs, bad dimensions are refused and named.

u = 0 is the one input on which the reference has no answer when w[0] == 0 (it returns index 0 and aborts with "0-weight
sampled"); include/vgx.h gives it the first positive entry, and test_u_zero_picks_the_first_positive_entry holds it to that."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER, LANES, TB = 4, 64, 256                 # vgx_rowscan.hip: RS_PER entries per thread, 64 lanes, RS_TB threads
WAVE, TILE = LANES * PER, TB * PER          # entries per wavefront (256) and per tile (1024)
CALL_ENTRIES = 3 << 18                      # rows * H of one call: the wrapper holds about 64 bytes per entry, so under 64 MB


def _tiles(H):
    return (H + TILE - 1) // TILE


def _D(H):
    """Additions on the longest path from an entry to a value vgx_rowscan_choose_kernel compares with r or divides by, counted
    from its code: 3 in the thread (`part`), 6 levels of fscan, 4 for `tot` over the wavefront sums (longer than the 3 of `before`
    plus `pre + before`), one `carry += tot` per earlier tile, 1 for `block_scan(...) + carry`, then in the hit thread up to 3
    `run += w[j]` and `s_pre = run + w[j]`, the two subtractions of `r - (pre - wi)` and the rounding of the division (an error of
    2^-53 |rnOut|, at most one unit of 2^-53 total / w).  A sum of non-negative terms carries at most 2^-53 of itself per addition
    on the path, so every such value is within D 2^-53 total of the exact one; the additions to a zero (`tot`, `carry`, `before`
    start at 0.0) are exact and cover the second-order terms."""
    return 3 + 6 + 4 + (_tiles(H) - 1) + 1 + 4 + 2 + 1


def _D_u(H):
    """The same count for rowTotal in vgx_rowscan_update_kernel: 4 `part += hp[j]`, 6 levels of fscan, 4 for `tot`, one
    `acc += tot` per tile.  The first addition of each of the three accumulators is to 0.0 and exact: they cover the half ulp of
    math.fsum and the second-order terms."""
    return 4 + 6 + 4 + _tiles(H)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _scan(w, u):
    """the weights w[rows, H] through both kernels, split over calls; hapPopRate must come back as w, bit for bit"""
    from vgsim_amd import _capi
    w = np.ascontiguousarray(w, dtype=np.float64)
    rows, H = w.shape
    step = max(1, CALL_ENTRIES // H)
    out = dict(rowTotal=np.empty(rows), chosen=np.empty(rows, dtype=np.int64), rnOut=np.empty(rows))
    for a in range(0, rows, step):
        b = min(rows, a + step)
        r123 = np.zeros((b - a, H, 3))
        r123[:, :, 0] = w[a:b]
        o = _capi.propensity_scan(np.ones((b - a, H), dtype=np.int64), r123, np.arange(H), np.zeros(H), np.ones((H, 1)),
                                  np.ones((b - a, 1)), np.ones(b - a), u[a:b])
        assert _same_bits(o["hapPopRate"], w[a:b]), "the weights did not arrive bit for bit"
        for k in out:
            out[k][a:b] = o[k]
    return out


def _targets(H):
    """every index up to H = 260; beyond, the structural set: the first two threads, both sides of every wavefront border (every
    fourth of them a tile border) and the row's end"""
    if H <= 260:
        return list(range(H))
    t = set(range(8)) | set(range(H - 5, H))
    for b in range(WAVE, H, WAVE):
        t |= {b - 1, b, b + 1}
    return sorted(i for i in t if 0 <= i < H)


# ---- 1. exact arithmetic ---------------------------------------------------------------------------------------------------
def _literal_fast_choose(w, r):
    """fast_choose.pxi:18-31 on Python integers and Fractions"""
    i, total = 0, int(w[0])
    while total < r and i < len(w) - 1:
        i += 1
        total += int(w[i])
    return i, Fraction(r - (total - int(w[i]))) / int(w[i])


def _exact_vectors(H, rng):
    """integer weight rows (one per target, zero pattern and ballast end) whose totals are powers of two, and their targets"""
    base = rng.integers(1, 8, size=H)
    big = rng.random(H) < 0.05
    base[big] <<= rng.integers(1, 9, size=int(big.sum()))              # at most 7 * 256; the row's sum stays below 2^20
    keep = rng.random(H) < 0.1
    patterns = ["dense", "sparse", "lone", "thread"] + (["wave_gap"] if H > WAVE else []) + (["tile_gap"] if H > TILE else [])
    vec, tgt = [], []
    for i in _targets(H):
        for pattern in patterns:
            w = base.copy()
            if pattern == "sparse":
                w[~keep] = 0
            elif pattern == "lone":
                w[:] = 0
            elif pattern == "thread":                                   # zeros fill the rest of the target's thread
                w[i // PER * PER:i // PER * PER + PER] = 0
            elif pattern == "wave_gap":                                 # a whole wavefront of zeros behind the target
                w[i + 1:(i // WAVE + 2) * WAVE] = 0
            elif pattern == "tile_gap":                                 # a whole tile of zeros behind the target
                w[i + 1:(i // TILE + 2) * TILE] = 0
            w[i] = base[i]
            for b in (0, H - 1):                                        # the ballast makes the total a power of two
                v = w.copy()
                v[b] = 0
                s = int(v.sum())
                v[b] = (1 << s.bit_length()) - s
                vec.append(v)
                tgt.append(i)
    return np.array(vec, dtype=np.int64), np.array(tgt)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099])
def test_exact_rows_choose_the_literal_index_and_rn_bit_for_bit(H):
    rng = np.random.default_rng(H)
    vec, tgt = _exact_vectors(H, rng)
    cum = np.cumsum(vec, axis=1)
    total = cum[:, -1]
    assert np.all(total & (total - 1) == 0) and total.max() <= 1 << 20 and vec.min() >= 0 and vec.max() <= 1 << 20
    at = np.arange(len(vec))
    wt, ct = vec[at, tgt], cum[at, tgt]
    assert np.all(wt > 0)
    # r = m / 2: just inside the target, exactly at its end, just past it (where the row goes on)
    m = np.concatenate([2 * (ct - wt) + 1, 2 * ct, (2 * ct + 1)[ct < total]])
    v = np.concatenate([at, at, at[ct < total]])
    place = np.concatenate([np.zeros_like(at), np.ones_like(at), 2 * np.ones_like(at)[ct < total]])
    u = m / (2.0 * total[v])                                            # exact: the total is a power of two
    assert np.all(total[v] * u * 2 == m)
    # the literal fastChoose, vectorised: the first i with cumsum[i] >= r is the number of entries with cumsum < r
    want = np.empty(len(m), dtype=np.int64)
    for a in range(0, len(m), 512):
        want[a:a + 512] = (2 * cum[v[a:a + 512]] < m[a:a + 512, None]).sum(axis=1)
    ww, wc = vec[v, want], cum[v, want]
    assert np.all(want[place < 2] == tgt[v][place < 2]) and np.all(want[place == 2] > tgt[v][place == 2]) and np.all(ww > 0)
    want_rn = (m / 2.0 - (wc - ww)) / ww                                # both operands exact: the correctly rounded quotient
    for k in rng.choice(len(m), size=min(len(m), 64), replace=False):   # ... and literally, on a sample
        i, rn = _literal_fast_choose(vec[v[k]], Fraction(int(m[k]), 2))
        assert (i, float(rn)) == (want[k], want_rn[k])
    out = _scan(vec[v].astype(np.float64), u)
    assert _same_bits(out["rowTotal"], total[v].astype(np.float64))
    bad = np.nonzero((out["chosen"] != want) | (_bits(out["rnOut"]) != _bits(want_rn)))[0]
    assert len(bad) == 0, "%d of %d rows; first: %s" % (len(bad), len(m), [
        dict(H=H, target=int(tgt[v[k]]), place=int(place[k]), r=m[k] / 2, chosen=int(out["chosen"][k]), want=int(want[k]),
             rn=out["rnOut"][k], want_rn=want_rn[k], row=vec[v[k]][max(0, tgt[v[k]] - 8):tgt[v[k]] + 9].tolist()) for k in bad[:3]])


@pytest.mark.parametrize("H", [1, 3, 5, 1025, 2049])
def test_u_zero_picks_the_first_positive_entry(H):
    """r = 0: where w[0] > 0 this is the reference's answer (index 0, rn 0); behind leading zeros the reference aborts and the
    kernel's contract is the first positive entry, wherever it lies, with rn 0."""
    first = [p for p in (0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 2047, 2048) if p < H]
    w = np.zeros((len(first), H))
    for k, p in enumerate(first):
        w[k, p] = 3.0
        w[k, H - 1] += 5.0
    out = _scan(w, np.zeros(len(first)))
    assert _same_bits(out["rowTotal"], w.sum(axis=1))
    assert out["chosen"].tolist() == first
    assert np.all(out["rnOut"] == 0.0)


# ---- 2. rounded arithmetic -------------------------------------------------------------------------------------------------
def _rounded_rows(H, rng):
    """weight rows of mixed magnitudes with the zero patterns of part 1; every row ends in a positive entry (at the row's end the
    kernel clamps like fast_choose.pxi:26, whatever the last weight is)"""
    def mag():
        return 10.0 ** rng.uniform(-8, 8, size=H)
    rows = {"dense": mag(), "sparse": mag() * (rng.random(H) < 0.1)}
    for j in range(PER):                                                 # entry j the only positive one of every thread
        rows["thread_j%d" % j] = mag() * (np.arange(H) % PER == j)
    z = mag()                                                            # all-zero threads and trailing zeros inside threads
    thr = np.arange(H) // PER
    z[np.isin(thr, np.nonzero(rng.random(thr[-1] + 1) < 0.3)[0])] = 0.0
    tail = rng.integers(1, PER + 1, size=thr[-1] + 1)                    # entries of the thread that stay
    z[np.arange(H) % PER >= tail[thr]] = 0.0
    rows["zero_threads"] = z
    g = mag()
    g[WAVE:2 * WAVE] = 0.0                                               # a whole wavefront of zeros
    g[TILE - WAVE:TILE + WAVE] = 0.0                                     # ... and two across the tile border
    rows["wave_gap"] = g
    if H > 2 * TILE:
        g = mag()
        g[TILE:2 * TILE] = 0.0                                           # a whole tile of zeros
        rows["tile_gap"] = g
    for w in rows.values():
        w[H - 1] = 10.0 ** rng.uniform(-8, 8)
    return rows


def _boundaries(w, rng):
    """8 indices of the structural set (a tile border and a wavefront border among them) and up to 8 ends of the last positive entry
    in front of an all-zero thread"""
    H = len(w)
    t = _targets(H)
    pick = {TILE - 1, TILE, WAVE - 1, WAVE, H - 1} | set(rng.choice(t, size=3, replace=False).tolist())
    pos = np.nonzero(w > 0)[0]
    zero_thread = np.add.reduceat(w, np.arange(0, H, PER)) == 0.0
    ends = [int(p) for p in pos if p // PER + 1 < len(zero_thread) and zero_thread[p // PER + 1] and not np.any(w[p + 1:(p // PER + 1) * PER])]
    if len(ends) > 8:
        ends = [ends[k] for k in np.linspace(0, len(ends) - 1, 8).astype(int)]
    return sorted(pick | set(ends))


def _rounded_failures(w, tot, u, labels):
    """one weight row, its rowTotal and many u through the choice: what a correct kernel may return, checked against the exact
    prefix sums of the row (fractions, computed once); returns the (label, finding) of every row that is outside it"""
    H = len(w)
    exact = [Fraction(0)]
    for x in w:
        exact.append(exact[-1] + Fraction(x))                           # exact[i] is the exact sum in front of entry i
    delta = Fraction(_D(H), 1 << 53) * exact[-1]
    assert abs(Fraction(tot) - exact[-1]) <= Fraction(_D_u(H), 1 << 53) * exact[-1]
    out = _scan(np.broadcast_to(w, (len(u), H)), u)
    assert _same_bits(out["rowTotal"], np.full(len(u), tot))            # deterministic: the totals the u were made for
    r = tot * u                                                          # one multiplication, as in the kernel
    failures = []
    for q in range(len(u)):
        c, rn = int(out["chosen"][q]), float(out["rnOut"][q])
        if not 0 <= c < H:
            failures.append((labels[q], "chosen %d outside the row" % c))
        elif not w[c] > 0.0:
            failures.append((labels[q], "chosen %d has weight 0, rnOut %r" % (c, rn)))
        elif not math.isfinite(rn):
            failures.append((labels[q], "rnOut %r" % rn))
        elif not (exact[c] <= Fraction(r[q]) + delta and exact[c + 1] >= Fraction(r[q]) - delta):
            failures.append((labels[q], "chosen %d: prefix %.17g .. %.17g around r %.17g" % (c, float(exact[c]), float(exact[c + 1]), r[q])))
        elif not -delta / Fraction(w[c]) <= Fraction(rn) <= 1 + delta / Fraction(w[c]):
            failures.append((labels[q], "chosen %d: rnOut %r" % (c, rn)))
    return failures


@pytest.mark.parametrize("H", [1025, 2049, 4099])
def test_ulp_sweep_across_boundaries_never_chooses_a_zero_weight(H):
    rng = np.random.default_rng(7 * H)
    rows = _rounded_rows(H, rng)
    names = list(rows)
    W = np.array([rows[n] for n in names])
    row_total = _scan(W, np.full(len(W), 0.5))["rowTotal"]
    failures, checked = [], 0
    for n, w, tot in zip(names, W, row_total):
        S = np.cumsum(w)                                                 # only to place r: the host's left-to-right prefix
        bnd = _boundaries(w, rng)
        u0 = np.array([S[b] / tot for b in bnd])
        k = np.arange(-8, 9)
        ub = np.maximum(_bits(u0)[:, None] + k[None, :], 0).view(np.float64)   # u moved by k ulps, kept inside [0, 1]
        u = np.minimum(ub, 1.0).ravel()
        failures += _rounded_failures(w, tot, u, [(H, n, b, int(kk)) for b in bnd for kk in k])
        checked += len(u)
    assert not failures, "%d of %d rows (D = %d); first (H, row, boundary, ulps): %s" % (len(failures), checked, _D(H), failures[:6])


@pytest.mark.parametrize("H", [6, 7, 8, 1030, 1031, 4098, 4099])
def test_last_thread_whose_serial_sums_stay_below_its_tree_sum(H):
    """w[0] = 1 and two or three entries of 0.4 ulp(1) in the row's last thread, behind them nothing (H = 8: a zero): that thread's
    tree-order sum and the row total are 1 + ulp, while 1 + 0.4 ulp + ... added one by one stays 1.  With r at the total the
    refinement has to end on the thread's last positive entry, not on the register behind it, which for these H lies outside the row
    (and in the next row's memory)."""
    a = 0.4 * 2.0 ** -52
    w = np.zeros(H)
    w[0] = 1.0
    w[(H - 1) // PER * PER:min(H, (H - 1) // PER * PER + 3)] = a
    tot = _scan(w[None, :], np.array([0.5]))["rowTotal"][0]
    assert tot == 1.0 + 2.0 ** -52
    u = np.array([1.0, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -51, 0.5, 1.0])
    failures = _rounded_failures(w, tot, u, [(H, float(x)) for x in u])
    assert not failures, failures


# ---- 3. the update kernel --------------------------------------------------------------------------------------------------
def _update_inputs(rows, H, S, rng):
    inf = rng.integers(0, 4, size=(rows, H)) * (rng.random((rows, H)) < 0.5)
    return dict(infectious=inf, rates123=rng.random((rows, H, 3)), numToHap=rng.permutation(H), bRate=1.0 + rng.random(H),
                susceptibility=rng.random((H, S)), rowSusceptible=rng.integers(1, 10 ** 6, size=(rows, S)).astype(float),
                rowContact=rng.random(rows) * 1e-6, u=rng.random(rows))


def _update_in_numpy(a):
    """the rates in the kernel's operation order (the one test_hip_rowscan.py states)"""
    n2h = a["numToHap"]
    x = a["rowSusceptible"][:, None, :] * a["susceptibility"][n2h][None, :, :]
    ws = np.zeros(x.shape[:2])
    for sn in range(x.shape[2]):
        ws = ws + x[:, :, sn]
    birth = a["bRate"][n2h][None, :] * (ws * a["rowContact"][:, None])
    te = ((birth + a["rates123"][:, :, 0]) + a["rates123"][:, :, 1]) + a["rates123"][:, :, 2]
    return x, birth, te, te * a["infectious"].astype(np.float64)


def _check_update(a, out):
    x, birth, te, hpr = _update_in_numpy(a)
    assert _same_bits(out["susceptHapPopRate"], x) and _same_bits(out["birthRate"], birth)
    assert _same_bits(out["tEvent"], te) and _same_bits(out["hapPopRate"], hpr)
    H = hpr.shape[1]
    for r in range(len(hpr)):
        bound = _D_u(H) * 2.0 ** -53 * math.fsum(np.abs(hpr[r]))
        assert abs(out["rowTotal"][r] - math.fsum(hpr[r])) <= bound, (r, out["rowTotal"][r], math.fsum(hpr[r]), bound)
    return hpr


def _call(a, **kw):
    from vgsim_amd import _capi
    return _capi.propensity_scan(a["infectious"], a["rates123"], a["numToHap"], a["bRate"], a["susceptibility"], a["rowSusceptible"],
                                 a["rowContact"], a["u"], **kw)


@pytest.mark.parametrize("S", [1, 2, 3, 5])
@pytest.mark.parametrize("H", [4, 5, 1023, 1024, 1025])
def test_update_paths_elementwise_bit_for_bit(H, S):
    """S = 1 with whole groups of four takes the wide loads and stores, everything else the per-entry loop"""
    a = _update_inputs(3, H, S, np.random.default_rng(100 * H + S))
    _check_update(a, _call(a))


@pytest.mark.parametrize("H,S", [(8, 1), (5, 1), (6, 2)])
def test_update_large_counts(H, S):
    a = _update_inputs(2, H, S, np.random.default_rng(H))
    big = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 62 + 2 ** 9 + 1, 2 ** 63 - 1, 2 ** 52 + 1, 3]
    a["infectious"] = np.array([big[:H], big[::-1][:H]], dtype=np.int64)
    _check_update(a, _call(a))


@pytest.mark.parametrize("H,S", [(1024, 1), (1025, 1), (1025, 3)])
def test_update_subnormal_and_huge_magnitudes(H, S):
    rng = np.random.default_rng(H + S)
    a = _update_inputs(2, H, S, rng)
    a["susceptibility"] = rng.random((H, S)) * 1e-310                    # subnormal susceptHapPopRate
    a["rowSusceptible"] = rng.integers(1, 4, size=(2, S)).astype(float)
    a["rowContact"] = np.array([1e300, 1e-3])                            # birth rates of about 1e-10 and subnormal ones
    r = rng.random((2, H, 3))
    a["rates123"] = np.where(rng.random((2, H, 3)) < 0.5, r * 1e300, r * 1e-310)   # at most 3e300 per entry, 1e304 per row
    x, birth, te, hpr = _update_in_numpy(a)
    assert x.max() < 2.3e-308 and te.max() > 1e299 and np.isfinite(hpr.sum(axis=1)).all()
    assert ((hpr > 0) & (hpr < 2.3e-308)).any()                          # subnormal propensities among them
    _check_update(a, _call(a))


def test_row_total_over_64_tiles():
    a = _update_inputs(2, 65536, 1, np.random.default_rng(64))
    a["rates123"] *= 10.0 ** np.random.default_rng(65).uniform(-8, 8, size=(2, 65536, 1))
    _check_update(a, _call(a))


@pytest.mark.parametrize("H,S", [(5, 1), (1025, 1), (1025, 2)])
def test_zero_total_row_between_two_others(H, S):
    a = _update_inputs(3, H, S, np.random.default_rng(H * S))
    a["infectious"][:, 0] = 2
    a["infectious"][1] = 0
    out = _call(a)
    _check_update(a, out)
    assert _bits(out["rowTotal"])[1] == 0                                # +0.0; chosen / rnOut of that row: see include/vgx.h
    b = {k: (v[[0, 2]] if k in ("infectious", "rates123", "rowSusceptible", "rowContact", "u") else v) for k, v in a.items()}
    alone = _call(b)
    assert out["rowTotal"][0] > 0 and out["rowTotal"][2] > 0
    for k in alone:
        assert np.array_equal(alone[k].view(np.int64), np.ascontiguousarray(out[k][[0, 2]]).view(np.int64)), k


# ---- 4. the entry points ---------------------------------------------------------------------------------------------------
def test_measuring_call_returns_the_first_rows_outputs():
    a = _update_inputs(1, 2049, 2, np.random.default_rng(4))
    a["infectious"][0, :8] = 1
    plain, timed = _call(a), _call(a, bench_rows=3, repeats=1)
    for k in ("birthRate", "tEvent", "hapPopRate", "susceptHapPopRate", "rowTotal", "chosen", "rnOut"):
        assert timed[k].shape == plain[k].shape and np.array_equal(timed[k].view(np.int64), plain[k].view(np.int64)), k
    for k in ("ms_update", "ms_choose"):
        assert math.isfinite(timed[k]) and timed[k] > 0.0, (k, timed[k])


def test_bad_dimensions_are_refused_and_named():
    from vgsim_amd import _capi
    lib = _capi.load_library()
    a = _update_inputs(2, 6, 2, np.random.default_rng(9))
    good = _call(a)
    keep = dict(infectious=a["infectious"].astype(np.int64), eventRates123=a["rates123"], numToHap=a["numToHap"].astype(np.int64),
                bRate=a["bRate"], susceptibility=a["susceptibility"], rowSusceptible=a["rowSusceptible"], rowContact=a["rowContact"],
                u=a["u"])
    keep.update({k: np.zeros_like(v) for k, v in good.items()})
    for rows, H, S in [(0, 6, 2), (-1, 6, 2), (2, 0, 2), (2, -3, 2), (2, 6, 0), (2, 6, -1)]:
        io = _capi.VgxRowScan()
        io.rows, io.H, io.S = rows, H, S
        for k, v in keep.items():
            setattr(io, k, _capi._p(v))
        assert lib.vgx_propensity_scan(C.byref(io)) == 1                 # VGX_ERR_ARG
        msg = lib.vgx_propensity_scan_error().decode()
        assert "bad dimensions" in msg and "rows = %d, H = %d, S = %d" % (rows, H, S) in msg, msg
        assert all(not v.any() for k, v in keep.items() if k in good)   # nothing was written
    ms = (C.c_double(0), C.c_double(0))
    io.rows, io.H, io.S = 2, 6, 2
    assert lib.vgx_propensity_scan_bench(C.byref(io), 0, 1, C.byref(ms[0]), C.byref(ms[1])) == 1
    assert "rows = 0, H = 6, S = 2" in lib.vgx_propensity_scan_error().decode()
    again = _call(a)                                                     # the next good call works
    for k in good:
        assert np.array_equal(again[k].view(np.int64), good[k].view(np.int64)), k
