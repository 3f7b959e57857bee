"""Packed intermediate records (LSB_OPT_PACK_VALUES).

A P == 1 LSD sort that starts with the regional first pass hands 12-byte
records {key, low word of the value} from pass to pass when every value fits
32 bits: the first pass packs, the last one writes 16-byte records again.  The
output must be the stable sort bit for bit whichever records the passes used:
  * index values (the reference's input) take the packed passes;
  * values over 32 bits that the sample sees keep whole records from the start;
  * one that only the first pass sees makes the sort start over from its
    input, and the context stops trying;
  * a pass that fails to launch in the middle of a packed sort still leaves a
    permutation of the input in A as 16-byte records.
Every case runs at LSB_REGION_MIN = 65536, so that sorts of 2^16 - 2^20
records take the regional start.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u8"), ("val", "<u8")])
N = 300_007


@pytest.fixture(autouse=True)
def small_regions(monkeypatch):
    """Regional first pass from 2^16 records on (contexts created after this),
    and the option's built-in default whatever the environment says."""
    monkeypatch.setenv("LSB_REGION_MIN", str(1 << 16))
    monkeypatch.delenv("LSB_PACK_VALUES", raising=False)
    monkeypatch.delenv("LSB_REGION_FIRST", raising=False)


def _stable(a):
    return a[np.argsort(a["key"], kind="stable")]


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=DT)
    a["key"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    a["val"] = np.arange(n, dtype=np.uint64)
    return a


def _sort(L, a, pack=None):
    """(output, records form, first-pass form, local passes) of one sort."""
    with L.World(a.size, ranks=1) as w:
        if pack is not None:
            w.set_option(L.OPT_PACK_VALUES, pack)
        w.scatter_global(a)
        w.my_sort()
        return w.gather_global(), w.last_records(), w.first_pass(), w.last_sort()[0]


@pytest.mark.parametrize("n", [65_536, 300_007, (1 << 20) + 12_345])
def test_packed_path_against_the_oracle(lsb_built, oracle_mod, n):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        w.generate()
        inp = w.gather_global()
        w.my_sort()
        out = w.gather_global()
        assert np.array_equal(out, oracle_mod.stable_sort(inp))
        assert w.verify() == (True, -1)
        assert w.last_records() == L.RECORDS_PACKED
        assert w.last_sort()[0] == 8
        assert w.first_pass() == L.FIRST_REGIONAL


def test_values_at_both_ends_of_32_bits(lsb_built):
    L = lsb_built
    a = _uniform(N, 1)
    a["val"] = np.random.default_rng(2).integers(0, 2**32, N, dtype=np.uint64)
    a["val"][5] = 0
    a["val"][N - 7] = 2**32 - 1
    a["val"][N // 2] = 2**32 - 1
    out, form, first, passes = _sort(L, a)
    assert form == L.RECORDS_PACKED and first == L.FIRST_REGIONAL and passes == 8
    want = _stable(a)
    assert np.array_equal(out["key"], want["key"]) and np.array_equal(out["val"], want["val"])


def test_equal_keys_keep_value_order(lsb_built):
    L = lsb_built
    rng = np.random.default_rng(3)
    half = rng.integers(0, 2**64 - 1, N // 2 + 1, dtype=np.uint64)
    a = np.zeros(N, dtype=DT)
    a["key"] = rng.permutation(np.concatenate([half, half]))[:N]
    a["val"] = np.arange(N, dtype=np.uint64)
    out, form, _, _ = _sort(L, a)
    assert form == L.RECORDS_PACKED
    assert np.array_equal(out, _stable(a))
    same = out["key"][1:] == out["key"][:-1]
    assert same.sum() >= N // 2 - 1
    assert np.all(out["val"][1:][same] > out["val"][:-1][same])


def test_wide_values_in_the_sample_keep_whole_records(lsb_built):
    L = lsb_built
    a = _uniform(N, 4)
    a["val"] = a["val"] + np.uint64(2**63)
    out, form, first, passes = _sort(L, a, pack=1)
    assert form == L.RECORDS_FULL and first == L.FIRST_REGIONAL and passes == 8
    assert np.array_equal(out, _stable(a))


def test_one_wide_value_redoes_the_sort(lsb_built):
    L = lsb_built
    a = _uniform(N, 5)
    a["val"][123_456] = 2**32
    with L.World(N, ranks=1) as w:
        w.set_option(L.OPT_PACK_VALUES, 2)
        w.scatter_global(a)
        w.my_sort()
        assert w.last_records() == L.RECORDS_PACKED_REDONE
        assert np.array_equal(w.gather_global(), _stable(a))
        # the context remembers: index values again, but whole records
        w.set_option(L.OPT_PACK_VALUES, 1)
        b = _uniform(N, 6)
        w.scatter_global(b)
        w.my_sort()
        assert w.last_records() == L.RECORDS_FULL
        assert np.array_equal(w.gather_global(), _stable(b))


def test_option_0_never_packs(lsb_built):
    L = lsb_built
    a = _uniform(N, 7)
    out1, form1, _, _ = _sort(L, a, pack=1)
    out0, form0, first0, passes0 = _sort(L, a, pack=0)
    assert form1 == L.RECORDS_PACKED
    assert form0 == L.RECORDS_FULL and first0 == L.FIRST_REGIONAL and passes0 == 8
    assert np.array_equal(out0, out1)
    with L.World(10, ranks=1) as w:
        with pytest.raises(L.LsbError):
            w.set_option(L.OPT_PACK_VALUES, 3)


@pytest.mark.parametrize("fail_at", [4, 8])
def test_failed_launch_in_a_packed_sort(lsb_built, oracle_mod, fail_at):
    """The 4th launch is a packed middle pass, the 8th the unpacking last
    pass: A holds packed records by then, and the error return leaves them
    unpacked, a permutation of the input."""
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
        assert w.last_records() == L.RECORDS_PACKED
        assert np.array_equal(w.gather_global(), oracle_mod.stable_sort(inp))
        assert w.verify() == (True, -1)


def test_packed_and_hybrid_sorts_share_a_context(lsb_built, oracle_mod):
    """The hybrid permutes A, B and R; a packed sort between two of them, and
    after one, must find three distinct buffers: every sort exact."""
    L = lsb_built
    with L.World(N, ranks=1) as w:
        for hybrid in (0, 1, 0):
            w.set_option(L.OPT_HYBRID, hybrid)
            w.generate()
            inp = w.gather_global()
            w.my_sort()
            assert w.last_records() == (L.RECORDS_FULL if hybrid else L.RECORDS_PACKED)
            assert np.array_equal(w.gather_global(), oracle_mod.stable_sort(inp)), hybrid
            assert w.verify() == (True, -1)
