"""Key forms of caller-owned columns, on the CPU (include/lsb.h,
csrc/lsb_keyform.h): lsb_key_encode / lsb_key_decode.

The model of the encodings is written out here in numpy from the header's
table and never calls the library:
  u64 / u32   identity
  i64 / i32   sign bit flipped
  f64 / f32   sign set: ~bits; else sign bit flipped
  descending  the complement within the key's width
and the order it must give is numpy's own order of the typed values (integers,
finite floats without -0.0), or the header's list for float specials: NaNs
with the sign set, -inf, finite values with -0.0 before +0.0, +inf, NaNs with
the sign clear.
"""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsb.h")

# name, LSB_KEY_*, numpy dtype of the value, bits
TYPES = [("u64", 0, np.uint64, 64), ("i64", 1, np.int64, 64), ("f64", 2, np.float64, 64),
         ("u32", 3, np.uint32, 32), ("i32", 4, np.int32, 32), ("f32", 5, np.float32, 32)]
IDS = [t[0] for t in TYPES]


def model_encode(bits, kt, descending):
    """bits: uint64 array (a 32-bit key in the low word) -> uint64 keys."""
    width = 32 if kt >= 3 else 64
    mask = np.uint64((1 << width) - 1)
    sign = np.uint64(1 << (width - 1))
    k = bits.astype(np.uint64) & mask
    if kt in (1, 4):
        k = k ^ sign
    elif kt in (2, 5):
        k = np.where((k & sign) != 0, ~k & mask, k ^ sign)
    if descending:
        k = ~k & mask
    return k


def raw_bits(values):
    """Typed numpy values -> their bits, zero-extended to uint64."""
    u = values.view(np.uint32 if values.dtype.itemsize == 4 else np.uint64)
    return u.astype(np.uint64)


def specials(kt, bits):
    top = (1 << bits) - 1
    s = [0, 1, top, 1 << (bits - 1), (1 << (bits - 1)) - 1]  # 0, and every type's minimum and maximum
    if kt in (2, 5):
        exp = 0x7ff << 52 if bits == 64 else 0xff << 23
        sgn = 1 << (bits - 1)
        quiet = 1 << (51 if bits == 64 else 22)
        s += [0, sgn,                       # +0.0, -0.0
              exp, exp | sgn,               # +inf, -inf
              1, sgn | 1,                   # the smallest denormals
              exp | quiet | 5, exp | sgn | quiet | 5, exp | 1, exp | sgn | 1]  # NaNs of both signs
    return np.array(s, dtype=np.uint64)


def lib_map(L, fn, xs, kt, flags):
    return np.array([fn(int(x), kt, flags) for x in xs], dtype=np.uint64)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name,kt,dt,bits", TYPES, ids=IDS)
def test_round_trip_and_model(lsb_built, name, kt, dt, bits, descending):
    lib = lsb_built._lib()
    rng = np.random.default_rng(kt * 2 + descending)
    xs = np.concatenate([specials(kt, bits), rng.integers(0, 1 << bits, 2000, dtype=np.uint64, endpoint=False)
                         if bits == 32 else rng.integers(0, 2**64 - 1, 2000, dtype=np.uint64, endpoint=True)])
    flags = 1 if descending else 0
    enc = lib_map(lsb_built, lib.lsb_key_encode, xs, kt, flags)
    assert np.array_equal(enc, model_encode(xs, kt, descending))
    assert np.array_equal(lib_map(lsb_built, lib.lsb_key_decode, enc, kt, flags), xs)
    if bits == 32:
        assert not np.any(enc >> np.uint64(32))  # a zero upper word in both orders
        # the upper word of the input is ignored
        noisy = xs | np.uint64(0xdeadbeef << 32)
        assert np.array_equal(lib_map(lsb_built, lib.lsb_key_encode, noisy, kt, flags), enc)
    assert lsb_built.key_encode(int(xs[7]), kt, descending) == int(enc[7])
    assert lsb_built.key_decode(int(enc[7]), kt, descending) == int(xs[7])


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name,kt,dt,bits", TYPES, ids=IDS)
def test_order_equals_numpys(lsb_built, name, kt, dt, bits, descending):
    """Strictly monotone: the ascending order of the encoded keys is numpy's
    order of the typed values (integers; finite floats without -0.0)."""
    lib = lsb_built._lib()
    rng = np.random.default_rng(100 + kt)
    if kt in (2, 5):
        info = np.finfo(dt)
        vals = np.concatenate([
            rng.standard_normal(1500).astype(dt), (rng.standard_normal(300) * 1e30).astype(dt),
            np.array([0.0, info.max, info.min, info.tiny, -info.tiny, info.smallest_subnormal,
                      -info.smallest_subnormal], dtype=dt)])
        vals = vals[np.isfinite(vals)]
        assert not np.any(np.signbit(vals) & (vals == 0))
    else:
        info = np.iinfo(dt)
        vals = np.concatenate([rng.integers(info.min, info.max, 1800, dtype=dt, endpoint=True),
                               np.array([info.min, info.max, 0, 1], dtype=dt),
                               np.array([-1] if info.min < 0 else [2], dtype=dt)])
    vals = np.unique(vals)  # ascending, distinct
    enc = lib_map(lsb_built, lib.lsb_key_encode, raw_bits(vals), kt, 1 if descending else 0)
    d = np.diff(enc.astype(object))
    assert np.all(d < 0) if descending else np.all(d > 0)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt,kt", [(np.float64, 2), (np.float32, 5)], ids=["f64", "f32"])
def test_float_specials_order(lsb_built, dt, kt, descending):
    """The header's list: NaNs with the sign set, -inf, finite values with -0.0
    before +0.0, +inf, NaNs with the sign clear."""
    lib = lsb_built._lib()
    u = np.uint64 if dt == np.float64 else np.uint32
    bits = 64 if dt == np.float64 else 32
    exp = 0x7ff << 52 if bits == 64 else 0xff << 23
    sgn = 1 << (bits - 1)
    info = np.finfo(dt)
    finite_neg = np.array([info.min, -1.5, -info.tiny, -info.smallest_subnormal], dtype=dt)
    finite_pos = np.array([info.smallest_subnormal, info.tiny, 1.5, info.max], dtype=dt)
    # ascending, group by group (within the NaN groups: by payload, as the bits order them)
    groups = [np.array([exp | sgn | 9, exp | sgn | 1], dtype=u),          # -NaN: larger payload first
              np.array([exp | sgn], dtype=u),                             # -inf
              finite_neg.view(u), np.array([sgn], dtype=u),               # finite < 0, then -0.0
              np.array([0], dtype=u), finite_pos.view(u),                 # +0.0, finite > 0
              np.array([exp], dtype=u),                                   # +inf
              np.array([exp | 1, exp | 9], dtype=u)]                      # +NaN
    asc = np.concatenate(groups).astype(np.uint64)
    enc = lib_map(lsb_built, lib.lsb_key_encode, asc, kt, 1 if descending else 0)
    d = np.diff(enc.astype(object))
    assert np.all(d < 0) if descending else np.all(d > 0)
    assert np.array_equal(enc, model_encode(asc, kt, descending))


def test_unknown_type_or_flag_gives_zero(lsb_built):
    lib = lsb_built._lib()
    for kt in (-1, 6, 7, 1 << 20):
        assert lib.lsb_key_encode(12345, kt, 0) == 0 and lib.lsb_key_decode(12345, kt, 0) == 0
    for flags in (2, 3, 4, -1):
        for kt in range(6):
            assert lib.lsb_key_encode(12345, kt, flags) == 0 and lib.lsb_key_decode(12345, kt, flags) == 0
    assert lib.lsb_key_encode(12345, 0, 0) == 12345  # the same arguments, a known form


def test_null_context_is_invalid(lsb_built):
    lib = lsb_built._lib()
    col = np.arange(8, dtype=np.uint64)
    p = col.ctypes.data
    assert lib.lsb_load_columns(None, 0, 0, 8, p, 0, p, 8, 0) == 1
    assert lib.lsb_store_columns(None, 0, 0, 8, p, 0, p, 8, 0) == 1
    assert lib.lsb_load_columns(None, 0, 0, 0, None, 0, None, 0, 0) == 1
    assert lib.lsb_store_columns(None, 0, 0, 0, None, 0, None, 0, 0) == 1
    assert np.array_equal(col, np.arange(8, dtype=np.uint64))


def test_python_constants_equal_the_headers(lsb_built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(LSB_[A-Z0-9_]+)\s+(-?\w+)\s*$", src, re.M)
            if re.fullmatch(r"-?(0x[0-9a-fA-F]+|\d+)", m.group(2))}
    want = {"LSB_KEY_U64": 0, "LSB_KEY_I64": 1, "LSB_KEY_F64": 2, "LSB_KEY_U32": 3, "LSB_KEY_I32": 4,
            "LSB_KEY_F32": 5, "LSB_ORDER_DESCENDING": 1}
    for name, value in want.items():
        assert defs[name] == value, name
        assert getattr(lsb_built, name[len("LSB_"):]) == defs[name], name
    declared = set(re.findall(r"\b(lsb_[a-z_0-9]+)\s*\(", src))
    assert {"lsb_key_encode", "lsb_key_decode", "lsb_load_columns", "lsb_store_columns"} <= declared


def test_module_imports_without_torch():
    """lsbsort imports torch only inside the column functions."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(HEADER), "..", "distributed-lsb_amd")
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); import lsbsort; "
            "assert lsbsort.KEY_F32 == 5 and callable(lsbsort.sort)" % os.path.abspath(pkg))
    subprocess.run([sys.executable, "-c", code], check=True)
