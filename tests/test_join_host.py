"""Lookup and join, host side (no GPU needed): the three symbols
(include/lsb.h, "the matches themselves"), the argument checks that return
before any device call, the Python bindings against the header, and the front
ends' refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsb.h")
SENT = 0x5555555555555555


def test_symbols(lsb_built):
    lib = lsb_built._lib()
    for name in ("lsb_lookup", "lsb_join_count", "lsb_store_join"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_null_context_touches_nothing(lsb_built):
    lib = lsb_built._lib()
    q = np.arange(4, dtype=np.uint64)  # host memory: never reaches a device call with a null context
    vals = np.full(4, SENT, dtype=np.uint64)
    found = np.full(4, 0x55, dtype=np.uint8)
    counts = np.full(4, SENT, dtype=np.int64)
    left, right, pos = (np.full(4, SENT, dtype=np.int64) for _ in range(3))
    total = np.full(1, SENT, dtype=np.int64)
    tp = total.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    for vb in (0, 4, 8, 3):
        assert lib.lsb_lookup(None, 0, 4, q.ctypes.data, 0, 0, vals.ctypes.data if vb else None, vb,
                              found.ctypes.data) == INVALID, vb
        assert lib.lsb_store_join(None, 0, 4, 0, left.ctypes.data, right.ctypes.data if vb else None, vb,
                                  pos.ctypes.data, tp) == INVALID, vb
    assert lib.lsb_lookup(None, 0, 0, None, 0, 0, None, 0, None) == INVALID  # m == 0 is no excuse for a null context
    assert lib.lsb_lookup(None, -1, -1, None, 6, 2, None, 8, None) == INVALID
    assert lib.lsb_join_count(None, 0, 4, q.ctypes.data, 0, 0, counts.ctypes.data, tp) == INVALID
    assert lib.lsb_join_count(None, 0, 0, None, 0, 0, None, None) == INVALID
    assert lib.lsb_join_count(None, -1, -1, None, 6, 2, None, tp) == INVALID
    assert lib.lsb_store_join(None, 0, 0, 0, None, None, 0, None, None) == INVALID
    assert lib.lsb_store_join(None, -1, -1, 7, None, None, 5, None, tp) == INVALID
    for a in (vals, counts, left, right, pos, total):
        assert np.all(a.view(np.uint64) == np.uint64(SENT))
    assert np.all(found == 0x55) and np.array_equal(q, np.arange(4, dtype=np.uint64))


def test_bindings_agree_with_the_header(lsb_built):
    """Every argument of the three prototypes has its ctypes twin: the count,
    and which ones are 32-bit integers, 64-bit integers and pointers."""
    ct = ctypes
    text = open(HEADER).read()
    lib = lsb_built._lib()
    kinds = {"int": ct.c_int, "int64_t": ct.c_int64}
    for name in ("lsb_lookup", "lsb_join_count", "lsb_store_join"):
        proto = re.search(r"^int\s+%s\(([^;]*)\);" % name, text, re.M)
        assert proto, name
        args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
        got = getattr(lib, name).argtypes
        assert len(args) == len(got), name
        for a, g in zip(args, got):
            if "*" in a:
                assert g is ct.c_void_p or issubclass(g, ct._Pointer), (name, a)
            else:
                assert g is kinds[a.split()[0]], (name, a)
        assert getattr(lib, name).restype is ct.c_int
    # the constants the calls take are the header's
    for name, value in (("KEY_U64", 0), ("KEY_F32", 5), ("ORDER_DESCENDING", 1)):
        got = re.search(r"^#define\s+LSB_%s\s+(\d+)" % name, text, re.M)
        assert got and int(got.group(1)) == value == getattr(lsb_built, name), name
    # the header says what the contract needs said
    section = re.sub(r"\s*\n \*\s*", " ", text[text.index("the matches themselves"):text.index("---- the hot path")])
    for phrase in ("from the last to the first", "LSB_ERR_NOMEM", "off_m = *total", "query_base + i", "rank * per + p"):
        assert phrase in section, phrase


def test_front_ends_refuse_without_device(lsb_built):
    torch = pytest.importorskip("torch")
    L = lsb_built
    k64, q64 = torch.arange(8, dtype=torch.int64), torch.arange(3, dtype=torch.int64)
    q32, qf = q64.to(torch.int32), q64.to(torch.float64)
    # a tensor that is not on a GPU, for every argument and both front ends
    for call in (lambda: L.lookup(k64, None, q64), lambda: L.lookup(k64, k64.clone(), q64),
                 lambda: L.lookup(k64, None, q64, default=-1, ranks=3), lambda: L.join(q64, k64),
                 lambda: L.join(q64, k64, how="left"), lambda: L.join(q64, k64, ranks=3)):
        with pytest.raises(ValueError):
            call()
    # a `how` that is neither, before anything else is looked at
    for how in ("outer", "right", "", "INNER", None, 0):
        with pytest.raises(ValueError, match="how"):
            L.join(q64, k64, how=how)
        with pytest.raises(ValueError, match="how"):
            L.join(None, None, how=how)
    # queries whose dtype maps to another key type than the keys'
    for q in (q32, qf):
        for call in (lambda: L.lookup(k64, None, q), lambda: L.join(q, k64)):
            with pytest.raises(ValueError):
                call()
    for bad in (None, np.arange(3), [1, 2, 3]):
        with pytest.raises(ValueError):
            L.lookup(k64, None, bad)
        with pytest.raises(ValueError):
            L.lookup(bad, None, q64)
        with pytest.raises(ValueError):
            L.join(bad, k64)
        with pytest.raises(ValueError):
            L.join(q64, bad)
