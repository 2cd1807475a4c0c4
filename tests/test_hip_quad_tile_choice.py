"""The haplotype choice of vgx_quad_kernel over lists longer than one 64-entry tile (vgx_quad.hip, q_long_select<1>) names the tile
by the running sums the rate refresh of that population (q_long_sum<1>) left at the end of every tile in a register of the row,
and streams the tiles only where a row has no such register.  Both forms, run on their own over synthetic lists (the hook
vgx_test_quad_tile_choice, four different rows per wavefront), must give what the reference's loop gives: the first entry whose
serial float64 prefix sum of fl(tE * count) is not below r, bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 1 << 16
LENGTHS = (0, 1025, 64, 129, 1, 1024, 65, 128)      # up to 16 tiles the register holds the sums; 17 tiles: every choice streams


def _prefix(counts, tE):
    """the reference's running sum: fl(tE * c) formed first, then added, left to right"""
    acc, out = np.float64(0.0), np.empty(len(counts), dtype=np.float64)
    for k, c in enumerate(counts):
        acc = acc + np.float64(tE) * np.float64(c)
        out[k] = acc
    return out


def _expected(counts, haps, tE, r):
    """(k_hit, pre_hit, w_hit, cnt_hit) of fastChoose over tE * counts (fast_choose.pxi:18-31) as the kernel reports them: no entry
    reaches r: the list's total and its last entry, chosen only if that is haplotype H - 1."""
    n = len(counts)
    if n == 0:
        return -1, 0.0, 0.0, 0
    p = _prefix(counts, tE)
    hit = np.nonzero(~(p < r))[0]
    if len(hit):
        k = int(hit[0])
        return k, p[k], np.float64(tE) * np.float64(counts[k]), int(counts[k])
    return (n - 1 if haps[-1] == H - 1 else -1), p[-1], np.float64(tE) * np.float64(counts[-1]), int(counts[-1])


def _cases():
    rng = np.random.default_rng(5)
    per_len = []
    for n in LENGTHS:
        counts = rng.integers(0, 4, size=n).astype(np.int32)                       # zeros among them
        big = rng.random(n) < 0.08
        counts[big] = rng.integers(256, 100000, size=int(big.sum()))               # counts above 255
        if n:
            counts[-1] = max(counts[-1], 1)
            counts[0] = max(counts[0], 1)
        haps = np.sort(rng.choice(H - 1, size=n, replace=False)).astype(np.int32)
        tE = float(rng.uniform(0.5, 5.0))
        rs = []
        if n == 0:
            rs = [(1.0, False)]
        else:
            p = _prefix(counts, tE)
            nt = (n + 63) // 64
            rs.append((p[min(n, 64) // 2] * 0.999, False))                          # in the first tile
            rs.append(((p[max(n - 2, 0)] + p[n - 1]) / 2 if n > 1 else p[0] / 2, False))     # in the last tile
            ends = sorted({min(64 * t, n) - 1 for t in (1, 2, (nt + 1) // 2, nt - 1, nt) if t >= 1})
            for e in ends:
                rs.append((p[e], False))                                            # an end-of-tile sum, met with equality
                rs.append((np.nextafter(p[e], np.inf), False))                      # one ulp above it
            rs.append((p[-1] * 1.5 + 1.0, False))                                   # above the total: no entry reaches it
            rs.append((p[-1] * 1.5 + 1.0, True))                                    # ... and the list's last entry is haplotype H - 1
        rows = []
        for r, last in rs:
            h = haps.copy()
            if last:
                h[-1] = H - 1
            rows.append((counts, h, tE, float(r)))
        per_len.append(rows)
    out = []
    for i in range(max(len(c) for c in per_len)):       # four different lengths in every wavefront
        for c in per_len:
            if i < len(c):
                out.append(c[i])
    return out


def test_tile_choice_from_the_kept_sums_and_streamed():
    from vgsim_amd import _capi
    lib = _capi.load_library()
    cases = _cases()
    if len(cases) % 4 == 0:
        cases = cases[:-1]                               # (a last wavefront with an idle row)
    rows, maxlen = len(cases), max(LENGTHS)
    counts = np.zeros((rows, maxlen), dtype=np.int32); haps = np.zeros((rows, maxlen), dtype=np.int32)
    n = np.zeros(rows, dtype=np.int32); tE = np.zeros(rows); r = np.zeros(rows)
    for i, (c, h, te, rr) in enumerate(cases):
        n[i] = len(c); counts[i, :len(c)] = c; haps[i, :len(c)] = h; tE[i] = te; r[i] = rr
    k_hit = np.full((2, rows), -99, dtype=np.int32); cnt_hit = np.full((2, rows), -99, dtype=np.int64)
    pre_hit = np.full((2, rows), np.nan); w_hit = np.full((2, rows), np.nan)
    I32, F, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rc = lib.vgx_test_quad_tile_choice(counts.ctypes.data_as(I32), haps.ctypes.data_as(I32), n.ctypes.data_as(I32), tE.ctypes.data_as(F),
                                       r.ctypes.data_as(F), rows, maxlen, H, k_hit.ctypes.data_as(I32), pre_hit.ctypes.data_as(F),
                                       w_hit.ctypes.data_as(F), cnt_hit.ctypes.data_as(I64))
    assert rc == 0
    seen = set()
    for i, (c, h, te, rr) in enumerate(cases):
        k, pre, w, cnt = _expected(c, h, te, rr)
        seen.add(len(c))
        for form, name in enumerate(("kept sums", "streamed")):
            got = (int(k_hit[form, i]), pre_hit[form, i], w_hit[form, i], int(cnt_hit[form, i]))
            same = (got[0] == k and np.float64(got[1]).view(np.uint64) == np.float64(pre).view(np.uint64)
                    and np.float64(got[2]).view(np.uint64) == np.float64(w).view(np.uint64) and got[3] == cnt)
            assert same, "row %d (%s, n = %d, tE = %r, r = %r): (k, prefix, weight, count) = %r, the serial loop gives %r" % (
                i, name, len(c), te, rr, got, (k, pre, w, cnt))
    assert seen == set(LENGTHS)
