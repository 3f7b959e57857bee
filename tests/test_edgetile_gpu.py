"""5120-record tiles for a packed sort's edge passes (LSB_EDGE_TILES).

Where a packed sort's middle passes take 5120 records per tile, its edge
passes take them too: the packing first pass (pass 0 of 8), which folds each
16-byte record to 12 bytes as it lands; the pass that reads the regional
layout (pass 1) when the regions' slots are whole tiles of 5120; the last
pass (pass 7), which stages keys and 32-bit values apart and widens the
values at the write-out.  LSB_EDGE_TILES names the edge passes that may
(1: the first, 2: the layout's pass, 4: the last); LSB_PACKED_TILE = 4096
puts every pass at 4096.  The output must be the stable sort bit for bit
whichever ran, and every case asserts through last_pass_tiles() which
instance did:
  * sizes whole and ragged in both tile sizes (regions of 4096 slots: the
    layout's pass stays at 4096), against the oracle, per edge selection;
  * 2^25 records (regions of 20480 slots): the layout's pass at 5120;
    2^24 (12288 slots): it stays at 4096;
  * equal keys keep their value order across tile and region boundaries of
    the first and the last pass;
  * a hot top byte: the last pass's runs are longer than a tile, and the pass
    before it counts a skewed next digit by 5120;
  * a value of 2^32 or more, in tile 0 and in the last, ragged tile: the
    large first pass reports it and the sort is redone with whole records;
  * a region that overflows under the large first pass: the sort starts over;
  * one context through every order of row counts on both look-back tracks;
  * a launch that fails in a large-tile sort.
Every case runs at LSB_REGION_MIN = 65536.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u8"), ("val", "<u8")])
N = 300_007
BIG = 5120
SMALL = 4096
FIRST, LAYOUT, LAST = 1, 2, 4
ALL = FIRST | LAYOUT | LAST
SIZES = [65_536, 81_920, 81_921, 300_007, (1 << 20) + 12_345]
N25 = 1 << 25


def _tiles(edge):
    """last_pass_tiles() of an 8-pass packed sort whose middle passes take 5120
    and whose edge passes in `edge` do."""
    return [BIG if edge & FIRST else SMALL, BIG if edge & LAYOUT else SMALL] + [BIG] * 5 + [BIG if edge & LAST else SMALL]


ALL_SMALL = [SMALL] * 8


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


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


def _packed_sort(L, monkeypatch, a, edge, tile, want_tiles, generated=False):
    """One packed 8-pass sort of `a` with LSB_EDGE_TILES = edge and
    LSB_PACKED_TILE = tile (None: unset).  generated: `a` is the context's own
    generated input, which verify() checks."""
    _setenv(monkeypatch, "LSB_EDGE_TILES", edge)
    _setenv(monkeypatch, "LSB_PACKED_TILE", tile)
    with L.World(a.size, ranks=1) as w:
        w.scatter_global(a)
        w.my_sort()
        out = w.gather_global()
        if generated:
            assert w.verify() == (True, -1)
        assert w.last_records() == L.RECORDS_PACKED
        assert w.last_sort()[0] == 8
        assert w.last_pass_tiles() == want_tiles, (edge, tile)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_the_oracle_per_edge_selection(lsb_built, oracle_mod, monkeypatch, n):
    """Regions of 4096 slots at these sizes: the layout's pass stays at 4096
    whatever the setting says; the first and the last pass follow their bits."""
    L = lsb_built
    with L.World(n, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
    want = oracle_mod.stable_sort(inp)
    for edge, tile, ran in ((0, None, _tiles(0)), (LAYOUT, None, _tiles(0)), (FIRST, None, _tiles(FIRST)),
                            (LAST, None, _tiles(LAST)), (FIRST | LAST, None, _tiles(FIRST | LAST)),
                            (None, None, _tiles(FIRST | LAST)), (None, SMALL, ALL_SMALL)):
        out = _packed_sort(L, monkeypatch, inp, edge, tile, ran, generated=True)
        assert out.tobytes() == want.tobytes(), (n, edge, tile)


@pytest.mark.parametrize("n", [N25, N25 + 12_345])
def test_the_layouts_pass_at_5120(lsb_built, monkeypatch, n):
    """Regions of 20480 = 4 x 5120 slots: the pass that reads them runs at 5120,
    and the whole output equals the all-4096 sort of the same input."""
    L = lsb_built
    outs = {}
    for edge, tile, ran in ((None, SMALL, ALL_SMALL), (None, None, _tiles(ALL)), (LAYOUT, None, _tiles(LAYOUT))):
        _setenv(monkeypatch, "LSB_EDGE_TILES", edge)
        _setenv(monkeypatch, "LSB_PACKED_TILE", tile)
        with L.World(n, ranks=1) as w:
            w.generate()
            w.my_sort()
            assert w.verify() == (True, -1)
            assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == ran, (edge, tile)
            outs[(edge, tile)] = w.gather_global()
    base = outs[(None, SMALL)]
    for k, out in outs.items():
        assert out.tobytes() == base.tobytes(), k


def test_regions_that_are_no_whole_large_tiles_keep_the_layouts_pass_at_4096(lsb_built, monkeypatch):
    """2^24 records: regions of 12288 slots, no multiple of 5120."""
    L = lsb_built
    monkeypatch.setenv("LSB_EDGE_TILES", str(ALL))
    with L.World(1 << 24, ranks=1) as w:
        w.generate()
        w.my_sort()
        assert w.verify() == (True, -1)
        assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == _tiles(FIRST | LAST)


def test_equal_keys_keep_value_order(lsb_built, monkeypatch):
    L = lsb_built
    n = 2 * 150_004
    rng = np.random.default_rng(3)
    half = rng.integers(0, 2**64 - 1, n // 2, dtype=np.uint64)
    a = np.zeros(n, dtype=DT)
    a["key"] = rng.permutation(np.concatenate([half, half]))
    a["val"] = np.arange(n, dtype=np.uint64)
    want = _stable(a)
    for edge, ran in ((ALL, _tiles(FIRST | LAST)), (FIRST, _tiles(FIRST)), (0, _tiles(0))):
        out = _packed_sort(L, monkeypatch, a, edge, None, ran)
        assert np.array_equal(out, want), edge
        same = out["key"][1:] == out["key"][:-1]
        assert same.sum() >= n // 2
        assert np.all(out["val"][1:][same] > out["val"][:-1][same])


def test_hot_top_byte(lsb_built, monkeypatch):
    """Half the records share byte 7: the last pass's hot run is longer than a
    tile, and the pass before it counts a skewed next digit by tiles of 5120."""
    L = lsb_built
    a = _uniform(N, 21)
    hot = np.random.default_rng(22).random(N) < 0.5
    a["key"][hot] = (a["key"][hot] & ~np.uint64(0xFF << 56)) | np.uint64(0x5A << 56)
    want = _stable(a)
    for edge, ran in ((ALL, _tiles(FIRST | LAST)), (FIRST, _tiles(FIRST)), (0, _tiles(0))):
        assert np.array_equal(_packed_sort(L, monkeypatch, a, edge, None, ran), want), edge


@pytest.mark.parametrize("where", ["tile0", "last_tile"])
def test_one_wide_value_under_the_large_first_pass_redoes_the_sort(lsb_built, where):
    """300007 = 58 x 5120 + 3047 records: the last tile is ragged."""
    L = lsb_built
    a = _uniform(N, 5)
    a["val"][5 if where == "tile0" else N - 3] = 2**32 + 7
    with L.World(N, ranks=1) as w:
        w.set_option(L.OPT_PACK_VALUES, 2)  # pack whatever the sample and earlier sorts saw
        b = _uniform(N, 6)
        w.scatter_global(b)
        w.my_sort()
        assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == _tiles(FIRST | LAST)
        w.scatter_global(a)
        w.my_sort()  # the same first pass, then whole records from the kept input
        assert w.last_records() == L.RECORDS_PACKED_REDONE
        assert w.last_pass_tiles() == ALL_SMALL
        assert np.array_equal(w.gather_global(), _stable(a))


def test_region_overflow_under_the_large_first_pass_starts_over(lsb_built):
    """The input of test_region_gpu's overflow case that the sample misses:
    2^24 records, 4700 more of digit-0 bucket 7 in sub-array 3, all in tiles
    the sample skips; region (7, 3) holds 12288 slots over a mean of 8192."""
    L = lsb_built
    n, extra = 1 << 24, 4700
    a = _uniform(n, 24)
    k = a["key"]
    idx = np.arange(n)
    lo = 3 * n // 8
    cand = np.flatnonzero((idx >= lo) & (idx < lo + n // 8) & ((idx // 4096) % 16 != 0) & ((k & np.uint64(0xFF)) != 7))
    pick = cand[:: max(1, cand.size // extra)][:extra]
    k[pick] = (k[pick] & ~np.uint64(0xFF)) | np.uint64(7)
    with L.World(n, ranks=1) as w:
        w.generate()
        w.my_sort()
        assert w.first_pass() == L.FIRST_REGIONAL and w.last_pass_tiles() == _tiles(FIRST | LAST)
        w.scatter_global(a)
        w.my_sort()  # the same first pass overflows region (7, 3)
        assert w.first_pass() == L.FIRST_REGIONAL_REDONE
        assert np.array_equal(w.gather_global(), _stable(a))


def test_one_context_through_every_order_of_row_counts_on_both_tracks(lsb_built, monkeypatch):
    """packed (the layout's pass at 5120: fewer rows on its track), whole
    records and the hybrid (4096: more rows there), twice round: each track
    sees short launches after long ones and long after short in both parities.
    A look-back that gave up fails the sort (lsb_sync reads its word)."""
    L = lsb_built
    monkeypatch.setenv("LSB_EDGE_TILES", str(ALL))
    with L.World(N25, ranks=1) as w:
        for _ in range(2):
            for kind in ("packed", "full", "packed", "hybrid", "packed"):
                w.set_option(L.OPT_HYBRID, 1 if kind == "hybrid" else 0)
                w.set_option(L.OPT_PACK_VALUES, 0 if kind == "full" else 1)
                w.generate()
                w.my_sort()
                assert w.verify() == (True, -1), kind
                if kind == "packed":
                    assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == _tiles(ALL)
                else:
                    assert w.last_records() == L.RECORDS_FULL
                    assert all(t in (0, SMALL) for t in w.last_pass_tiles()), kind
                if kind == "full":
                    assert w.last_pass_tiles() == ALL_SMALL


@pytest.mark.parametrize("fail_at", [1, 2])
def test_failed_launch_before_the_layout_is_read_keeps_the_input(lsb_built, monkeypatch, fail_at):
    """Launch 1 is the first pass at 5120, launch 2 the layout's pass at 5120:
    the input stays in A, and the next sort is exact with the same tiles."""
    L = lsb_built
    monkeypatch.setenv("LSB_EDGE_TILES", str(ALL))
    with L.World(N25, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
        w.set_option(L.OPT_FAIL_ONESWEEP, fail_at)
        with pytest.raises(L.LsbError, match="injected"):
            w.my_sort()
        w.set_option(L.OPT_FAIL_ONESWEEP, 0)
        assert w.gather_global().tobytes() == inp.tobytes()
        w.my_sort()
        assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == _tiles(ALL)
        assert w.verify() == (True, -1)


def test_failed_last_pass_leaves_whole_records(lsb_built, oracle_mod, monkeypatch):
    """Launch 8 is the last pass at 5120: A holds packed records by then, and
    the error return leaves them unpacked, a permutation of the input."""
    L = lsb_built
    monkeypatch.setenv("LSB_EDGE_TILES", str(ALL))
    with L.World(N, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
        w.set_option(L.OPT_FAIL_ONESWEEP, 8)
        with pytest.raises(L.LsbError, match="injected"):
            w.my_sort()
        w.set_option(L.OPT_FAIL_ONESWEEP, 0)
        held = w.gather_global()
        assert np.array_equal(np.sort(held, order=["key", "val"]), np.sort(inp, order=["key", "val"]))
        w.my_sort()
        assert w.last_records() == L.RECORDS_PACKED and w.last_pass_tiles() == _tiles(FIRST | LAST)
        assert np.array_equal(w.gather_global(), oracle_mod.stable_sort(inp))
        assert w.verify() == (True, -1)
