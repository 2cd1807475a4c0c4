"""The serial prefix chains of the row kernels (vgx_rowprim.h row_scan16, vgx_quad.hip row_scan64) on their own: every lane's
prefix and the row total, bit for bit against a left-to-right sum on the host."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rows():
    """rows of 64 weights (finite, >= +0.0) and their carries"""
    rng = np.random.default_rng(20240611)
    w, c = [], []

    def add(ws, cs):
        w.append(np.ascontiguousarray(ws, dtype=np.float64).reshape(-1, 64))
        c.append(np.ascontiguousarray(cs, dtype=np.float64).reshape(-1))

    n = 512
    # random weights over the magnitudes of rates (sums that round at every step), carries of the same kind and +0.0
    add(rng.random((n, 64)) * 10.0 ** rng.integers(-8, 8, (n, 64)), rng.random(n) * 10.0 ** rng.integers(-8, 8, n))
    add(rng.random((n, 64)), np.zeros(n))
    # many exact zeros: most entries +0.0, whole rows of +0.0, zeros in front of / behind the only weight
    z = rng.random((n, 64)) * (rng.random((n, 64)) < 0.15)
    z[:16] = 0.0
    for k in range(64):
        z[16 + k] = 0.0
        z[16 + k, k] = 1.0 / 3.0
    add(z, np.where(rng.random(n) < 0.5, 0.0, rng.random(n)))
    # lists shorter than the tile, padded with +0.0 (every length 0..64)
    s = rng.random((65 * 4, 64)) * 1e3
    for i in range(65 * 4):
        s[i, i // 4:] = 0.0
    add(s, np.where(np.arange(65 * 4) % 2 == 0, 0.0, rng.random(65 * 4) * 1e3))
    # large carries: the weights vanish against them, or round at the last bit
    add(rng.random((n, 64)) * 10.0 ** rng.integers(-3, 3, (n, 64)), 10.0 ** rng.integers(6, 18, n) * (1.0 + rng.random(n)))
    add(rng.integers(0, 3, (n, 64)).astype(np.float64), 2.0 ** 53 - rng.integers(0, 64, n).astype(np.float64))
    # integer-valued weights (counts times a rate of 1.0)
    add(rng.integers(0, 1 << 20, (n, 64)).astype(np.float64), np.zeros(n))
    return np.concatenate(w), np.concatenate(c)


def _serial(w, carry):
    """carry + w[0] + ... + w[k], one rounding per addition, left to right"""
    out = np.empty_like(w)
    acc = carry.copy()
    for k in range(w.shape[1]):
        acc = acc + w[:, k]
        out[:, k] = acc
    return out


def test_row_scans_equal_the_serial_prefix():
    from vgsim_amd import _capi
    lib = _capi.load_library()
    w, carry = _rows()
    rows = len(carry)
    w = np.ascontiguousarray(w[:rows - 1]); carry = np.ascontiguousarray(carry[:rows - 1])     # (a last wavefront with an idle row)
    rows -= 1
    pre16 = np.full((rows, 16), np.nan); tot16 = np.full((rows, 16), np.nan); pre64 = np.full((rows, 64), np.nan)
    F = C.POINTER(C.c_double)
    rc = lib.vgx_test_row_scans(w.ctypes.data_as(F), carry.ctypes.data_as(F), rows, pre16.ctypes.data_as(F), tot16.ctypes.data_as(F),
                                pre64.ctypes.data_as(F))
    assert rc == 0
    want = _serial(w, carry)
    for name, got, ref in (("row_scan16 prefix", pre16, want[:, :16]), ("row_scan16 total", tot16, np.repeat(want[:, 15:16], 16, axis=1)),
                           ("row_scan64 prefix", pre64, want)):
        bad = np.argwhere(got.view(np.uint64) != ref.view(np.uint64))
        assert len(bad) == 0, "%s: %d mismatches, first at row %d lane %d: %r vs %r" % (
            name, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
