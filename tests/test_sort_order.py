"""The batch-order sort (bsw_sort.hip) on its own, through the test hook bsw_sort_order_device: the
permutation must equal numpy's stable argsort of the keys' low key_bits bits, element for element.

Sizes walk the tile edges (T = 4096 keys per workgroup), the wave edges inside a tile, several tiles with a
partial last one, and one size whose table rows are longer than one iteration of a scan workgroup
(SCAN_CHUNK tiles).  Key sets choose how many bits vary, hence how many passes run and which buffers
the passes ping-pong through (0, 1, 2, 3 and 4 passes), with the key mask on (digits from the varying
bits, as the planned path runs it) and off (fixed digits over every bit below key_bits)."""

import numpy as np
import pytest

import bsw

pytestmark = pytest.mark.gpu

T = 4096                # bsw_sort.h: kSortTile
SCAN_CHUNK = 256        # bsw_sort.h: kSortScanChunk, tiles per iteration of a scan workgroup's loop
N_SCAN2 = SCAN_CHUNK * T + 1        # the first size with SCAN_CHUNK + 1 tiles: two iterations
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, N_SCAN2)

BITS9 = (0, 3, 7, 8, 12, 17, 21, 26, 31)
BITS17 = (0, 1, 2, 4, 5, 7, 9, 10, 12, 14, 16, 19, 20, 23, 27, 30, 31)


def _scattered(rng, n, bits, base):
    """Keys that differ from `base` only at the given bit positions, each position random."""
    k = np.full(n, base, dtype=np.uint32)
    for b in bits:
        k ^= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(b)
    return k


def _rand32(n):
    return np.random.default_rng(32).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


# name -> (keys(n), key_bits, use_mask)
KEYSETS = {
    "equal_0pass": (lambda n: np.full(n, 0x9A3C51E7, dtype=np.uint32), 32, True),
    "bit31_1pass": (lambda n: _scattered(np.random.default_rng(1), n, (31,), 0x12345678), 32, True),
    "bits9_2pass": (lambda n: _scattered(np.random.default_rng(9), n, BITS9, 0x0F0F00F0), 32, True),
    "bits17_3pass": (lambda n: _scattered(np.random.default_rng(17), n, BITS17, 0x00A00A00), 32, True),
    "rand32_4pass": (_rand32, 32, True),
    "rand32_nomask": (_rand32, 32, False),
    "keybits20": (_rand32, 20, True),
    "keybits20_nomask": (_rand32, 20, False),
}


@pytest.fixture(scope="module")
def eng():
    e = bsw.Engine(device=0)
    yield e
    e.close()


def _want(keys, key_bits):
    m = np.uint32((1 << key_bits) - 1)
    return np.argsort(keys & m, kind="stable").astype(np.int32)


def _check(eng, keys, key_bits, use_mask):
    got = eng.sort_order(keys, key_bits, use_mask)
    want = _want(keys, key_bits)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {len(keys)} places differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(KEYSETS))
def test_sort_order(eng, name, n):
    make, key_bits, use_mask = KEYSETS[name]
    _check(eng, make(n), key_bits, use_mask)


@pytest.mark.parametrize("use_mask", (True, False))
def test_many_duplicates(eng, use_mask):
    """32 distinct keys over 3 T + 5 items: long runs of equal keys keep their input order."""
    rng = np.random.default_rng(5)
    distinct = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32)
    keys = distinct[rng.integers(0, 32, 3 * T + 5)]
    _check(eng, keys, 32, use_mask)


def test_slot_reuse_after_larger_sort(eng):
    """A small sort after a large one on the same slot: stale table and buffer contents must not show."""
    _check(eng, _rand32(3 * T + 5), 32, True)
    _check(eng, _scattered(np.random.default_rng(3), 65, BITS9, 0), 32, True)
    _check(eng, np.full(T + 1, 7, dtype=np.uint32), 32, True)


def test_c2_key_distribution(eng):
    """Keys shaped like the planned path's on a C2 batch: plan_kernel's keymode-2 formula restated for the
    fields that need no sequence data (class, qlen, tlen / 32, h0), with the seed identities and the related
    bit held constant.  A key-distribution case for the sort, no check of plan_kernel."""
    pairs, _, _ = bsw.synth_batch(5000)
    qlen = np.maximum(pairs["len2"], 0).astype(np.int64)
    tlen = np.maximum(pairs["len1"], 0).astype(np.int64)
    h0 = pairs["h0"].astype(np.int64)
    mn = np.minimum(qlen, tlen)
    lane = np.select([qlen <= 32, qlen <= 64, qlen <= 96, qlen <= 128, qlen <= 160], [0, 1, 2, 3, 4], 10)
    packed = (lane < 5) & (h0 + mn <= 255) & (qlen + 1 <= 160)
    pk = 5 + np.select([qlen + 1 <= 32, qlen + 1 <= 64, qlen + 1 <= 96, qlen + 1 <= 128], [0, 1, 2, 3], 4)
    cls = np.where((h0 >= 0) & (np.maximum(h0, 0) + mn < 32768), np.where(packed, pk, lane), 10)
    mt, rel = 25, 1
    keys = ((cls << 28) | ((255 - np.minimum(qlen, 255)) << 20) | ((1 - rel) << 19) |
            ((63 - np.minimum(tlen >> 5, 63)) << 13) | ((31 - mt) << 8) |
            (255 - np.minimum(np.maximum(h0, 0), 255))).astype(np.uint32)
    assert len(np.unique(keys)) > 1
    _check(eng, keys, 32, True)
    _check(eng, keys, 32, False)
