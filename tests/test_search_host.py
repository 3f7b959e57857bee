"""The search of the sorted records, host side (no GPU needed): the symbol and
its constants (include/lsb.h, "searching the sorted records"), the argument
checks that return before any device call, and the front ends' refusals that
need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

INVALID = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsb.h")


def test_error_codes_without_device(lsb_built):
    lib = lsb_built._lib()
    assert hasattr(lib, "lsb_search")
    q = np.arange(4, dtype=np.uint64)  # host memory: never reaches a device call with a null context
    out = np.full(4, -5, dtype=np.int64)
    for mode in (0, 1, 2, 4, 5, 6, 3, 7, 8, -1):
        assert lib.lsb_search(None, 0, 4, q.ctypes.data, 0, 0, mode, out.ctypes.data) == INVALID, mode
    assert lib.lsb_search(None, -1, -1, None, 6, 2, 3, None) == INVALID
    assert lib.lsb_search(None, 0, 0, None, 0, 0, 0, None) == INVALID  # m == 0 is no excuse for a null context
    assert np.all(out == -5) and np.array_equal(q, np.arange(4, dtype=np.uint64))


def test_constants(lsb_built):
    L = lsb_built
    assert (L.SEARCH_LOWER, L.SEARCH_UPPER, L.SEARCH_COUNT, L.SEARCH_ADD) == (0, 1, 2, 4)
    text = open(HEADER).read()
    for name, value in (("LOWER", 0), ("UPPER", 1), ("COUNT", 2), ("ADD", 4)):
        got = re.search(r"^#define\s+LSB_SEARCH_%s\s+(\d+)" % name, text, re.M)
        assert got and int(got.group(1)) == value == getattr(L, "SEARCH_" + name), name


def test_front_ends_refuse_without_device(lsb_built):
    torch = pytest.importorskip("torch")
    L = lsb_built
    k64, q64 = torch.arange(8, dtype=torch.int64), torch.arange(3, dtype=torch.int64)
    q32, qf = q64.to(torch.int32), q64.to(torch.float64)
    # a tensor that is not on a GPU, for either argument and every front end
    for call in (lambda: L.searchsorted(k64, q64), lambda: L.count_of(k64, q64), lambda: L.isin(q64, k64),
                 lambda: L.searchsorted(k64, q64, side="right", ranks=3)):
        with pytest.raises(ValueError):
            call()
    # a side that is none of the two (the World method knows "count", the front end's name for it is count_of)
    for side in ("middle", "", "LEFT", None, 0):
        with pytest.raises(ValueError, match="side"):
            L.searchsorted(k64, q64, side=side)
    # queries whose dtype maps to another key type than the keys'
    for q in (q32, qf):
        for call in (lambda: L.searchsorted(k64, q), lambda: L.count_of(k64, q), lambda: L.isin(q, k64)):
            with pytest.raises(ValueError):
                call()
    for bad in (None, np.arange(3), [1, 2, 3]):
        with pytest.raises(ValueError):
            L.searchsorted(k64, bad)
        with pytest.raises(ValueError):
            L.isin(bad, k64)


def test_mismatched_dtypes_are_told_apart(lsb_built):
    """The dtype rule itself, without a device: the key types the front ends
    compare, and the element-size rule under key_type=."""
    torch = pytest.importorskip("torch")
    L = lsb_built
    kt = L._key_type_of
    assert kt(torch.zeros(1, dtype=torch.int64)) == L.KEY_I64 != kt(torch.zeros(1, dtype=torch.float64))
    assert kt(torch.zeros(1, dtype=torch.int32)) == L.KEY_I32 != kt(torch.zeros(1, dtype=torch.float32))
    assert kt(torch.zeros(1, dtype=torch.int64), L.KEY_U64) == L.KEY_U64
    with pytest.raises(ValueError):
        kt(torch.zeros(1, dtype=torch.int32), L.KEY_U64)  # a 4-byte query column against 8-byte keys
