"""The device's exclusive prefix sum (glim_amd/csrc/scan.hpp) and radix sort (glim_amd/csrc/sort.hip) on their own, through their debug views,
against NumPy with 64-bit integers -- at every size where they take another path.

Scan: a tile is 4096 entries (1024 threads x int4, with a scalar tail for the last one to three entries); the tile sums are scanned by one
block in chunks of 1024 tiles with a serial carry, which an array of more than 1024 x 4096 = 4 194 304 entries is the first to use.  Every
comparison is an equality.  Sort: the tile shape (ROUNDS = 1, 2, 4, 8) switches at 32 768, 65 536 and 131 072 pairs, the offsets of a pass
move to a launch of their own above 524 288; every shape runs here with digits to rank, on both sides of every switch.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, CHUNK = 4096, 1024 * 4096
SCAN_SIZES = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
LARGEST = SCAN_SIZES[-3:]
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def _contents(T):
    """name -> int32 array of T entries"""
    rng = np.random.default_rng(T)
    out = {"ones": np.ones(T, dtype=np.int32)}
    flags = rng.integers(0, 2, size=T).astype(np.int32)
    flags[-1] = 0  # the form every consumer passes: the last entry's prefix is the count
    out["flags"] = flags
    out["counts"] = rng.integers(0, 16, size=T).astype(np.int32)
    two = np.zeros(T, dtype=np.int32)
    for i in (CHUNK - 1, CHUNK):  # the last entry of tile 1023 and the first of tile 1024: either side of the first carry
        if i < T:
            two[i] = 1
    out["two_ones_at_the_chunk_boundary"] = two
    if T in LARGEST:
        q, r = divmod(INT32_MAX, T)
        full = np.full(T, q, dtype=np.int32)
        full[:r] += 1
        assert int(full.sum(dtype=np.int64)) == INT32_MAX
        out["total_int32_max"] = full
    return out


def _reference(v):
    ref = np.concatenate([[0], np.cumsum(v[:-1], dtype=np.int64)])
    assert ref.max() <= INT32_MAX  # no partial sum overflows: the cast below loses nothing
    return ref.astype(np.int32)


@pytest.mark.parametrize("T", SCAN_SIZES)
def test_exclusive_scan_equals_the_cumulative_sum(ctx, T):
    from glim_amd import api

    for name, v in _contents(T).items():
        want = _reference(v)
        got = api.debug_exclusive_scan(v, ctx=ctx)
        bad = np.nonzero(got != want)[0]
        print(f"T {T} {name}: total {int(v.sum(dtype=np.int64))}, mismatches {len(bad)}" + (f", first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}" if len(bad) else ""))
        assert got.dtype == np.int32 and len(got) == T
        np.testing.assert_array_equal(got, want, err_msg=name)
        again = api.debug_exclusive_scan(v, ctx=ctx)
        assert again.tobytes() == got.tobytes(), name


def test_exclusive_scan_refusals_and_the_empty_array(ctx):
    from glim_amd import _lib, api

    f = _lib.lib().glim_amd_debug_exclusive_scan
    ip = C.POINTER(C.c_int32)
    a, b = np.arange(4, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    pa, pb = a.ctypes.data_as(ip), b.ctypes.data_as(ip)
    assert f(ctx._h, 0, None, None) == 0 and f(ctx._h, 0, pa, pb) == 0  # n == 0: OK, nothing is touched
    assert (b == -7).all()
    assert f(ctx._h, -1, pa, pb) == -1  # GLIM_AMD_ERR_INVALID
    assert f(ctx._h, 2**28 + 1, pa, pb) == -1
    assert f(ctx._h, 4, None, pb) == -1 and f(ctx._h, 4, pa, None) == -1
    assert f(None, 4, pa, pb) == -1
    assert (b == -7).all() and (a == np.arange(4)).all()
    assert f(ctx._h, 4, pa, pb) == 0 and b.tolist() == [0, 0, 1, 3]
    assert len(api.debug_exclusive_scan([], ctx=ctx)) == 0


# ---- sort ------------------------------------------------------------------------------------------------------------------------------------
SORT_CASES = [(32768, 16), (32769, 16),  # ROUNDS 1 | 2
              (65536, 24), (65537, 24),  # ROUNDS 2 | 4
              (100000, 40),  # ROUNDS 4, five passes
              (131072, 17), (131073, 17),  # ROUNDS 4 | 8
              (524288, 19), (524289, 19)]  # ROUNDS 8: offsets in the scatter kernel | in a launch of their own
KEY_SETS = ["duplicates", "all_equal", "sorted", "reversed", "ones_above_bits"]


def _keys(kind, n, bits, rng):
    mask = np.uint64((1 << bits) - 1)
    keys = rng.integers(0, 2**63, size=n, dtype=np.uint64)
    if kind == "duplicates":  # the recipe of tests/test_preprocess.py
        keys[::7] = keys[3]
    elif kind == "all_equal":
        keys[:] = keys[0] | np.uint64(0x5A5)  # digits to rank in every pass
    elif kind == "sorted":
        keys = np.sort(keys & mask)
    elif kind == "reversed":
        keys = np.sort(keys & mask)[::-1].copy()
    elif kind == "ones_above_bits":
        keys = keys | ~mask
    return keys, mask


@pytest.mark.parametrize("kind", KEY_SETS)
@pytest.mark.parametrize("n,bits", SORT_CASES)
def test_radix_sort_is_stable_and_exact_at_every_tile_shape(ctx, n, bits, kind):
    from glim_amd import api

    rng = np.random.default_rng(n + bits)
    keys, mask = _keys(kind, n, bits, rng)
    if kind == "ones_above_bits":
        assert ((keys >> np.uint64(bits)) == np.uint64((1 << (64 - bits)) - 1)).all()
    order = np.argsort(keys & mask, kind="stable")
    ko, vo = api.debug_sort_pairs(keys, None, bits, ctx=ctx)
    np.testing.assert_array_equal(vo, order.astype(np.uint32))
    np.testing.assert_array_equal(ko, keys[order])
    vals = rng.permutation(n).astype(np.uint32)  # explicit values travel with their keys
    ko2, vo2 = api.debug_sort_pairs(keys, vals, bits, ctx=ctx)
    np.testing.assert_array_equal(vo2, vals[order])
    np.testing.assert_array_equal(ko2, keys[order])
