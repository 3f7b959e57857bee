"""5120-record tiles for a packed sort's middle passes (LSB_PACKED_TILE).

The passes of a packed sort that read and write 12-byte records and count the
next digit (passes 2-6 of 8) take 512 x 10 records per tile where every
sub-array of the next pass holds at least a tile; the passes beside them keep
4096, so two passes count the next digit by another tile size than their own,
and the look-back rows are shared by launches of different tile counts.  The
output must be the stable sort bit for bit whichever size ran:
  * sizes at the applicability edge, whole and ragged in both tile sizes;
  * equal keys keep their value order across tile and sub-array boundaries;
  * a hot middle byte: runs longer than a tile that cross sub-array boundaries;
  * one context through every order of tile counts and both parities;
  * a launch that fails in a large-tile sort.
Every case runs at LSB_REGION_MIN = 65536 (the regional start, hence packed
records, from 2^16 records on).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u8"), ("val", "<u8")])
N = 300_007
BIG = 5120
SIZES = [65_536, 81_920, 81_921, 300_007, (1 << 20) + 12_345]


@pytest.fixture(autouse=True)
def small_regions(monkeypatch):
    monkeypatch.setenv("LSB_REGION_MIN", str(1 << 16))
    for name in ("LSB_PACK_VALUES", "LSB_REGION_FIRST", "LSB_PACKED_TILE"):
        monkeypatch.delenv(name, raising=False)


def _stable(a):
    return a[np.argsort(a["key"], kind="stable")]


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=DT)
    a["key"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    a["val"] = np.arange(n, dtype=np.uint64)
    return a


def _packed_sort(L, monkeypatch, a, tile, want_tile, generated=False):
    """One packed 8-pass sort of `a` with LSB_PACKED_TILE = tile (None: unset).
    generated: `a` is the context's own generated input, which verify() checks."""
    if tile is None:
        monkeypatch.delenv("LSB_PACKED_TILE", raising=False)
    else:
        monkeypatch.setenv("LSB_PACKED_TILE", str(tile))
    with L.World(a.size, ranks=1) as w:
        w.scatter_global(a)
        w.my_sort()
        out = w.gather_global()
        if generated:
            assert w.verify() == (True, -1)
        assert w.last_records() == L.RECORDS_PACKED
        assert w.last_sort()[0] == 8
        assert w.last_packed_tile() == want_tile
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_the_oracle_in_both_tile_sizes(lsb_built, oracle_mod, monkeypatch, n):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
    want = oracle_mod.stable_sort(inp)
    for tile, ran in ((None, BIG), (4096, 4096), (BIG, BIG)):
        out = _packed_sort(L, monkeypatch, inp, tile, ran, generated=True)
        assert out.tobytes() == want.tobytes(), (n, tile)


def test_equal_keys_keep_value_order(lsb_built, monkeypatch):
    L = lsb_built
    n = 2 * 150_004
    rng = np.random.default_rng(3)
    half = rng.integers(0, 2**64 - 1, n // 2, dtype=np.uint64)
    a = np.zeros(n, dtype=DT)
    a["key"] = rng.permutation(np.concatenate([half, half]))
    a["val"] = np.arange(n, dtype=np.uint64)
    want = _stable(a)
    for tile, ran in ((None, BIG), (4096, 4096)):
        out = _packed_sort(L, monkeypatch, a, tile, ran)
        assert np.array_equal(out, want), tile
        same = out["key"][1:] == out["key"][:-1]
        assert same.sum() >= n // 2
        assert np.all(out["val"][1:][same] > out["val"][:-1][same])


def test_the_size_between(lsb_built, monkeypatch):
    """LSB_PACKED_TILE=4608 (512 x 9, kept for measurements): the pass that
    reads the layout counts by 4608, passes 2-5 run 4608 -> 4608, pass 6 the
    4608 -> 4096 seam; the edge passes have no 4608 instance and keep 4096."""
    L = lsb_built
    a = _uniform(N, 11)
    monkeypatch.setenv("LSB_PACKED_TILE", "4608")
    with L.World(a.size, ranks=1) as w:
        w.scatter_global(a)
        w.my_sort()
        out = w.gather_global()
        assert w.last_records() == L.RECORDS_PACKED and w.last_packed_tile() == 4608
        assert w.last_pass_tiles() == [4096, 4096, 4608, 4608, 4608, 4608, 4608, 4096]
    assert np.array_equal(out, _stable(a))


def test_hot_middle_byte(lsb_built, monkeypatch):
    """Byte 0 uniform (the regional start is taken), half the records share
    byte 3: that pass's hot run is longer than a tile, the passes after it see
    runs that cross the next pass's sub-array boundaries, and the pass before
    it counts a skewed next digit."""
    L = lsb_built
    a = _uniform(N, 21)
    hot = np.random.default_rng(22).random(N) < 0.5
    a["key"][hot] = (a["key"][hot] & ~np.uint64(0xFF << 24)) | np.uint64(0x5A << 24)
    want = _stable(a)
    for tile, ran in ((None, BIG), (4096, 4096)):
        assert np.array_equal(_packed_sort(L, monkeypatch, a, tile, ran), want), tile


def test_one_context_through_every_order_of_tile_counts(lsb_built, monkeypatch):
    """packed, hybrid, whole records, packed, fewer passes, packed; twice
    round: the shared look-back rows see short launches after long ones and
    long after short, in both parities."""
    L = lsb_built
    span = _uniform(N, 31)
    span["key"] &= np.uint64(2**40 - 1)  # constant top bytes: 5 passes, counted start
    with L.World(N, ranks=1) as w:
        seed = 40
        for _ in range(2):
            for kind in ("packed", "hybrid", "full", "packed", "span", "packed"):
                seed += 1
                a = span if kind == "span" else _uniform(N, seed)
                w.set_option(L.OPT_HYBRID, 1 if kind == "hybrid" else 0)
                w.set_option(L.OPT_PACK_VALUES, 0 if kind == "full" else 1)
                w.scatter_global(a)
                w.my_sort()
                assert np.array_equal(w.gather_global(), _stable(a)), (kind, seed)
                if kind == "packed":
                    assert w.last_records() == L.RECORDS_PACKED and w.last_packed_tile() == BIG
                else:
                    assert w.last_records() == L.RECORDS_FULL and w.last_packed_tile() == 0
                if kind == "span":
                    assert w.last_sort()[0] == 5


@pytest.mark.parametrize("fail_at", [4, 8])
def test_failed_launch_in_a_large_tile_sort(lsb_built, oracle_mod, fail_at):
    """Launch 4 is a 5120-record middle pass, launch 8 the last pass (4096,
    after the rows' fill): A holds a permutation of the input as 16-byte
    records, and the next sort is exact and large-tile again."""
    L = lsb_built
    with L.World(N, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
        w.set_option(L.OPT_FAIL_ONESWEEP, fail_at)
        with pytest.raises(L.LsbError, match="injected"):
            w.my_sort()
        w.set_option(L.OPT_FAIL_ONESWEEP, 0)
        held = w.gather_global()
        assert np.array_equal(np.sort(held, order=["key", "val"]), np.sort(inp, order=["key", "val"]))
        w.my_sort()
        assert w.last_records() == L.RECORDS_PACKED and w.last_packed_tile() == BIG
        assert np.array_equal(w.gather_global(), oracle_mod.stable_sort(inp))
        assert w.verify() == (True, -1)
