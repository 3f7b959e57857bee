"""k_onesweep's run cuts from a plan per (bucket, sub-array).

A bucket thread works out once per sub-array where its output range meets the
next pass's sub-array boundaries (os_cut_plan, lsb_ostile.h) and cuts each
tile's run by two compares; a range over two boundaries keeps os_run_cut.
The next digit's histogram is built from those cuts, so a wrong cut shows as
a wrong sort one pass later.  Every case is compared with numpy's stable
argsort, and with lsb_verify where the input is the context's own (the check
is for generated records only; constructed keys take lsb_check_sorted):
  * packed and whole-record sorts at 61,441, 300,007 and 2^20 + 1 records:
    the seams of the three tile sizes, and runs that cross a next-pass
    boundary (61,441 is below the smallest packed sort, 2^16 records: both
    settings sort whole records there);
  * one bucket of the second byte with over a quarter of the records;
  * the same bucket filling a whole sub-array of the second pass's input, its
    output range placed over two boundaries of the third pass's: the
    `general` plan (the test checks that premise by the geometry's own
    arithmetic before it sorts);
  * a constant middle byte: a pass is skipped and next_shift jumps.
(One bucket with a quarter of the records, spread evenly over the input, has
an eighth of that in each sub-array: its ranges are 1/32 of the output and
never cover a next-pass sub-array.  That case checks the skewed count beside
the plans; the constructed one after it is what reaches the `general` plan.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u8"), ("val", "<u8")])
SIZES = [61_441, 300_007, (1 << 20) + 1]
N = 300_007
SUBS = 8


@pytest.fixture(autouse=True)
def small_regions(monkeypatch):
    monkeypatch.setenv("LSB_REGION_MIN", str(1 << 16))
    for name in ("LSB_PACK_VALUES", "LSB_REGION_FIRST", "LSB_PACKED_TILE", "LSB_EDGE_TILES"):
        monkeypatch.delenv(name, raising=False)


def _stable(a):
    return a[np.argsort(a["key"], kind="stable")]


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=DT)
    a["key"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    a["val"] = np.arange(n, dtype=np.uint64)
    return a


def _set_byte(keys, idx, byte, value):
    sh = np.uint64(8 * byte)
    keys[idx] = (keys[idx] & ~(np.uint64(0xFF) << sh)) | (np.asarray(value, dtype=np.uint64) << sh)


def _sort(L, a, packed, passes=8):
    """One sort of the constructed records `a`; packed: 12-byte records
    between the passes, else whole records."""
    with L.World(a.size, ranks=1) as w:
        w.set_option(L.OPT_PACK_VALUES, 1 if packed else 0)
        w.scatter_global(a)
        w.my_sort()
        assert w.check_sorted()
        assert w.last_records() == (L.RECORDS_PACKED if packed else L.RECORDS_FULL)
        assert w.last_sort()[0] == passes
        return w.gather_global()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "whole"])
@pytest.mark.parametrize("n", SIZES)
def test_seam_sizes_packed_and_whole(lsb_built, n, packed):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        w.set_option(L.OPT_PACK_VALUES, 1 if packed else 0)
        w.generate()
        inp = w.gather_global()
        w.my_sort()
        assert w.verify() == (True, -1)
        assert w.last_sort()[0] == 8
        assert w.last_records() == (L.RECORDS_PACKED if packed and n >= 1 << 16 else L.RECORDS_FULL)
        if packed and n >= 81_920:
            assert w.last_packed_tile() == 5120
        out = w.gather_global()
    assert out.tobytes() == _stable(inp).tobytes()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "whole"])
def test_a_quarter_of_the_records_in_one_bucket_of_the_second_byte(lsb_built, packed):
    a = _uniform(N, 61)
    hot = np.flatnonzero(np.random.default_rng(62).random(N) < 0.3)
    assert hot.size > N // 4
    _set_byte(a["key"], hot, 1, 0x5A)
    assert np.array_equal(_sort(lsb_built, a, packed), _stable(a))


def _first_tile(x, tt):
    return x * tt // SUBS


def _general_keys(tile):
    """N records whose second pass (byte 1, `tile` records per tile, reading
    records ordered by byte 0) finds sub-array 3 of its input filled by bucket
    0x5A alone, with that bucket's first output slot 100 slots before a
    next-pass boundary whose sub-array is shorter than the range: the range
    covers two boundaries."""
    tt = -(-N // tile)
    first = [_first_tile(x, tt) * tile for x in range(SUBS + 1)]
    first[SUBS] = N
    lo, hi = first[3], first[4]  # the input sub-array the hot bucket fills
    length = hi - lo
    # a next-pass sub-array (same tiles) shorter than the range, not the first
    x1 = next(x for x in range(1, SUBS - 1) if first[x + 1] - first[x] < length)
    base = first[x1] - 100
    assert 0 < base and first[x1 + 1] < base + length <= N  # two boundaries inside (base, base + length)
    rng = np.random.default_rng(71)
    a = _uniform(N, 72)
    k = a["key"]
    # Byte 0 by position: 0..99 before the hot sub-array, 100 inside it, 101..255 after,
    # then the records shuffled: the first pass puts them back in this order of byte 0.
    pos = np.arange(N)
    b0 = np.where(pos < lo, pos * 100 // lo, np.where(pos < hi, 100, 101 + (pos - hi) * 155 // (N - hi)))
    _set_byte(k, pos, 0, b0)
    inside = (pos >= lo) & (pos < hi)
    _set_byte(k, np.flatnonzero(inside), 1, 0x5A)
    # Outside it nothing takes 0x5A, and exactly `base` records lie below it.
    rest = rng.permutation(np.flatnonzero(~inside))
    assert rest.size > base
    _set_byte(k, rest[:base], 1, rng.integers(0, 0x5A, base))
    _set_byte(k, rest[base:], 1, rng.integers(0x5B, 256, rest.size - base))
    a = a[rng.permutation(N)]
    a["val"] = np.arange(N, dtype=np.uint64)
    # The premise, from the keys themselves: bucket 0x5A's range of input sub-array 3.
    order = np.argsort(a["key"] & np.uint64(0xFF), kind="stable")
    b1 = ((a["key"][order] >> np.uint64(8)) & np.uint64(0xFF)).astype(np.int64)
    assert np.all(b1[lo:hi] == 0x5A) and np.count_nonzero(b1 == 0x5A) == length
    assert np.count_nonzero(b1 < 0x5A) == base
    return a


@pytest.mark.parametrize("split", [1, 2], ids=["whole_stage", "split_stage"])
def test_a_bucket_that_covers_a_whole_next_pass_sub_array(lsb_built, monkeypatch, split):
    """Whole records from a counted start, 4096 per tile in every pass: the
    second pass's tiles are the dense input's, as _general_keys assumes.  Both
    stage forms: the split one re-reads the bucket's count on a sub-array
    change, the whole one holds it in registers."""
    L = lsb_built
    monkeypatch.setenv("LSB_REGION_FIRST", "0")
    a = _general_keys(4096)
    with L.World(N, ranks=1) as w:
        w.set_option(L.OPT_PACK_VALUES, 0)
        w.set_option(L.OPT_ONESWEEP_SPLIT, split)
        w.scatter_global(a)
        w.my_sort()
        assert w.check_sorted()
        assert w.first_pass() == L.FIRST_COUNT and w.last_records() == L.RECORDS_FULL
        assert w.last_sort()[0] == 8 and w.last_pass_tiles() == [4096] * 8
        out = w.gather_global()
    assert np.array_equal(out, _stable(a))


@pytest.mark.parametrize("n", [N, (1 << 20) + 1])
def test_a_constant_middle_byte_skips_a_pass(lsb_built, n):
    """Seven passes; the pass on byte 2 counts byte 4 as its next digit.  (A
    sort with a constant byte starts from a count and keeps whole records.)"""
    a = _uniform(n, 81)
    _set_byte(a["key"], np.arange(n), 3, 0xC3)
    assert np.array_equal(_sort(lsb_built, a, False, passes=7), _stable(a))
