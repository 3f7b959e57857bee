"""Caller-owned device columns (lsb_load_columns / lsb_store_columns,
lsbsort.sort; include/lsb.h, DESIGN.md "Caller-owned columns").

The order model is numpy on the CPU: a kind="stable" argsort of the encoded
uint64 keys, the encoding written out below from the header's table (it never
calls lsb_key_encode).  Where floats are compared with torch.sort(stable=True)
on the CPU the inputs hold no NaN and no -0.0: torch orders only those
differently from the bits.

The columns are torch CUDA tensors, and torch brings a HIP runtime of its
own: a process can use both torch's GPU side and this library only when torch
is imported before the library is loaded (the library then binds to the
runtime already in the process).  The pytest process loads the
library first, for every other test file, so the tests below run in one child
pytest process over this same file that imports torch first
(LSB_COLUMNS_CHILD=1), once per session; here each test reports what its
namesake did there.
"""
import functools
import inspect
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_COLUMNS_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

N = 300_007
# name -> (LSB_KEY_*, numpy dtype)
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}
ORDERS = [False, True]
ORDER_IDS = ["asc", "desc"]


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("columns") / "child.xml"
    env = dict(os.environ, LSB_COLUMNS_CHILD="1")
    for name in ("LSB_REGION_MIN", "LSB_PACK_VALUES", "LSB_REGION_FIRST"):  # the tests that want them set them
        env.pop(name, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider",
                        "--junitxml", str(xml)], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    out = {}
    if xml.exists():
        for case in ET.parse(str(xml)).getroot().iter("testcase"):
            bad = [(c.tag, (c.get("message") or "") + "\n" + (c.text or "")) for c in case
                   if c.tag in ("failure", "error", "skipped")]
            out[case.get("name")] = bad[0] if bad else ("passed", "")
    out[None] = p.stdout[-4000:] + p.stderr[-2000:]
    return out


def torch_first(fn):
    """The test as it runs in the child process; in the pytest process that
    started it, a test of the same name and parameters that passes exactly
    when the child's did."""
    if IN_CHILD:
        return fn

    @functools.wraps(fn)
    def reported(*args, request, child_outcomes, **kwargs):
        got = child_outcomes.get(request.node.name)
        assert got is not None, "the child process did not run this test:\n" + child_outcomes[None]
        assert got[0] == "passed", got[1]

    sig = inspect.signature(fn)
    extra = [inspect.Parameter(n, inspect.Parameter.KEYWORD_ONLY) for n in ("request", "child_outcomes")]
    reported.__signature__ = sig.replace(parameters=list(sig.parameters.values()) + extra)
    return reported


# ------------------------------------------------------------------ the model
def model_encode(bits, kt, descending):
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


def bits_of(a):
    """A typed numpy array's bits, zero-extended to uint64."""
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def model_order(keys, kt, descending):
    return np.argsort(model_encode(bits_of(keys), kt, descending), kind="stable")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits_of(a), bits_of(b))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def float_specials(dt):
    u = np.uint64 if dt == np.float64 else np.uint32
    bits = 64 if dt == np.float64 else 32
    exp = 0x7ff << 52 if bits == 64 else 0xff << 23
    sgn = 1 << (bits - 1)
    quiet = 1 << (51 if bits == 64 else 22)
    s = [0, sgn, exp, exp | sgn, 1, sgn | 1, exp | quiet | 5, exp | sgn | quiet | 5, exp | 1, exp | sgn | 1,
         exp | quiet, exp | sgn | quiet | 0x1234]
    return np.array(s, dtype=u).view(dt)


@functools.lru_cache(maxsize=None)
def raw_keys(name, n=N + 9):
    """Random bits of the type (for floats: NaNs, infinities, zeros of both
    signs and denormals among them), specials and extremes first."""
    kt, dt = KEYS[name]
    rng = np.random.default_rng(10 + kt)
    u = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    a = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
    top = np.iinfo(u).max
    sp = np.array([0, top, top // 2, top // 2 + 1, 1], dtype=u)
    if kt in (2, 5):
        sp = np.concatenate([float_specials(dt).view(u), sp])
    a[:sp.size] = sp
    a[-sp.size:] = sp[::-1]
    a[4000:4000 + sp.size] = sp
    a.setflags(write=False)
    return a.view(dt)


@functools.lru_cache(maxsize=None)
def tie_keys(name, n=N):
    """n keys of at most 2^12 distinct values spread over every byte of the
    type, negative ones included; floats without NaN and without -0.0."""
    kt, dt = KEYS[name]
    v = np.random.default_rng(20 + kt).integers(0, 4096, n).astype(np.int64)
    if name == "u64":
        a = v.astype(np.uint64) * np.uint64(0x0004_0010_0400_1001)
    elif name == "i64":
        a = (v - 2048) * np.int64(0x0002_0008_0200_0801)
    elif name == "u32":
        a = (v * 0x00100401 % (1 << 32)).astype(np.uint32)
    elif name == "i32":
        a = ((v - 2048) * 0x00080201).astype(np.int32)
    else:
        a = ((v - 2048) * 0.37).astype(dt) * np.where(v % 3 == 0, dt(1e20), dt(1.0)).astype(dt)
        assert np.all(np.isfinite(a)) and not np.any(np.signbit(a) & (a == 0))
    a = a.astype(dt)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def some_values(vbytes, n=N + 9):
    rng = np.random.default_rng(30 + vbytes)
    if vbytes == 8:
        a = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True).view(np.int64)
    else:
        a = rng.integers(0, 2**32 - 1, n, dtype=np.uint32, endpoint=True).view(np.float32)  # any 4-byte dtype
    a.setflags(write=False)
    return a


def sort_columns(L, keys, values, kt, descending, ranks=1, radix_bits=8):
    """Load the blocks of a World(n, ranks), sort, store into fresh tensors.
    -> (keys, values or indices) as numpy, and the world's (last_sort,
    last_records, first_pass)."""
    import torch
    n = keys.size
    dk = dev(keys)
    dv = None if values is None else dev(values)
    with L.World(n, ranks=ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, dk[lo:lo + h], None if dv is None else dv[lo:lo + h], descending=descending,
                               key_type=kt)
        w.my_sort()
        assert w.check_sorted()
        ok, ov = [], []
        for r in range(ranks):
            h = w.here(r)
            tk = torch.empty(h, dtype=dk.dtype, device="cuda")
            tv = torch.empty(h, dtype=torch.int64 if dv is None else dv.dtype, device="cuda")
            if h:
                w.store_columns(r, tk, tv, descending=descending, key_type=kt)
            ok.append(host(tk))
            ov.append(host(tv))
        info = (w.last_sort(), w.last_records(), w.first_pass())
    assert same_bits(host(dk), keys)  # the inputs are left untouched
    return np.concatenate(ok), np.concatenate(ov), info


# ------------------------------------------------- 1. round trip, no sort
@pytest.mark.parametrize("descending", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", list(KEYS))
@torch_first
def test_round_trip_without_a_sort(lsb_built, name, descending):
    """Load, copy_out, store: cnt in {1, 2, 3, 4097, 300007} x values of 8
    bytes, 4 bytes and none x whole tensors (16-byte path) and t[1:] views of
    both columns (element path).  Records equal the model's; keys and values
    come back bit for bit, and nothing is written outside the columns."""
    L = lsb_built
    kt, dt = KEYS[name]
    with L.World(N + 16, ranks=1) as w:
        for cnt in (1, 2, 3, 4097, N):
            for vbytes in (8, 4, 0):
                for mode in ("whole", "sliced") + (("mixed",) if cnt == 4097 else ()):
                    lead_k = 1 if mode == "sliced" else 0
                    lead_v = 1 if mode in ("sliced", "mixed") else 0
                    off = 0 if mode == "whole" else 7
                    keys = raw_keys(name)[3:3 + cnt] if cnt < 4097 else raw_keys(name)[:cnt]
                    vals = None if vbytes == 0 else some_values(vbytes)[:cnt]
                    # t[1:] views: one element in front, so the view is aligned to its element only
                    dk = dev(np.concatenate([keys[:lead_k], keys]))[lead_k:]
                    dv = None if vals is None else dev(np.concatenate([vals[:lead_v], vals]))[lead_v:]
                    assert (dk.data_ptr() % 16 == 0) == (lead_k == 0)
                    w.load_columns(0, dk, dv, off=off, descending=descending, key_type=kt)
                    rec = w.copy_out(0, off, cnt)
                    what = (cnt, vbytes, mode)
                    assert np.array_equal(rec["key"], model_encode(bits_of(keys), kt, descending)), what
                    want_v = bits_of(vals) if vals is not None else np.arange(off, off + cnt, dtype=np.uint64)
                    assert np.array_equal(rec["val"], want_v), what
                    # store into fresh columns between sentinels
                    vdt = np.int64 if vals is None else vals.dtype

                    def fresh():
                        return (dev(np.full(lead_k + cnt + 4, 0x55, dtype=keys.dtype)),
                                dev(np.full(lead_v + cnt + 4, 0x55, dtype=vdt)))

                    def check(t, lead, want_bits):
                        h = host(t)
                        assert np.array_equal(bits_of(h[lead:lead + cnt]), want_bits), what
                        assert np.all(h[:lead] == 0x55) and np.all(h[lead + cnt:] == 0x55), what

                    ok, ov = fresh()
                    w.store_columns(0, ok[lead_k:lead_k + cnt], ov[lead_v:lead_v + cnt], off=off,
                                    descending=descending, key_type=kt)
                    check(ok, lead_k, bits_of(keys))
                    check(ov, lead_v, want_v)
                    if cnt == 4097:  # one output column alone
                        ok, ov = fresh()
                        w.store_columns(0, ok[lead_k:lead_k + cnt], None, off=off, descending=descending,
                                        key_type=kt)
                        w.store_columns(0, None, ov[lead_v:lead_v + cnt], off=off, descending=descending,
                                        key_type=kt)
                        check(ok, lead_k, bits_of(keys))
                        check(ov, lead_v, want_v)
                    assert same_bits(host(dk), keys), what  # the input columns are untouched


# ------------------------------------------------- 2. sort against the model
@pytest.mark.parametrize("vform", ["val8", "val4", "argsort"])
@pytest.mark.parametrize("descending", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", list(KEYS))
@torch_first
def test_sort_against_the_model(lsb_built, name, descending, vform):
    import torch
    kt, dt = KEYS[name]
    keys = tie_keys(name)
    vals = {"val8": some_values(8)[:N], "val4": some_values(4)[:N], "argsort": None}[vform]
    out_k, out_v, _ = sort_columns(lsb_built, keys, vals, kt, descending)
    perm = model_order(keys, kt, descending)
    assert same_bits(out_k, keys[perm])
    assert same_bits(out_v, vals[perm]) if vals is not None else np.array_equal(out_v, perm)
    ties = np.count_nonzero(out_k[1:] == out_k[:-1])
    assert ties > N - 4097 - 1  # many equal keys: the order inside them is the input's
    if name in ("i64", "i32", "f32", "f64"):
        tv, ti = torch.sort(torch.from_numpy(keys.copy()), stable=True, descending=descending)
        assert same_bits(out_k, tv.numpy())
        assert same_bits(out_v, vals[ti.numpy()]) if vals is not None else np.array_equal(out_v, ti.numpy())


# ------------------------------------------------- 3. float specials
def float_class(a):
    """Place of each float in the header's ascending list (zeros of both signs
    and the finite values on either side of them told apart)."""
    neg = np.signbit(a)
    c = np.full(a.shape, -1)
    c[np.isnan(a) & neg] = 0
    c[np.isneginf(a)] = 1
    c[np.isfinite(a) & (a < 0)] = 2
    c[(a == 0) & neg] = 3
    c[(a == 0) & ~neg] = 4
    c[np.isfinite(a) & (a > 0)] = 5
    c[np.isposinf(a)] = 6
    c[np.isnan(a) & ~neg] = 7
    assert np.all(c >= 0)
    return c


@pytest.mark.parametrize("descending", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", ["f64", "f32"])
@torch_first
def test_float_specials_through_a_sort(lsb_built, name, descending):
    kt, dt = KEYS[name]
    n = 4097
    rng = np.random.default_rng(40 + kt)
    keys = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(dt)
    sp = float_specials(dt)
    where = rng.permutation(n)[:sp.size * 40]
    keys[where] = np.tile(sp, 40)  # every special 40 times, scattered
    out_k, out_v, _ = sort_columns(lsb_built, keys, None, kt, descending)
    cls = float_class(out_k)
    assert len(set(cls)) == 8
    d = np.diff(cls)
    assert np.all(d <= 0) if descending else np.all(d >= 0)
    fin = np.isfinite(out_k)
    df = np.diff(out_k[fin].astype(np.float64))
    assert np.all(df <= 0) if descending else np.all(df >= 0)
    # bit for bit: payloads and zero signs intact, equal keys in input order
    perm = model_order(keys, kt, descending)
    assert same_bits(out_k, keys[perm]) and np.array_equal(out_v, perm)
    assert same_bits(keys[out_v], out_k)


# ------------------------------------------------- 4. 32-bit keys skip passes
@pytest.mark.parametrize("descending", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name,passes", [("u32", 4), ("i32", 4), ("f32", 4), ("i64", 8)])
@torch_first
def test_32_bit_keys_take_4_passes(lsb_built, name, passes, descending, monkeypatch):
    monkeypatch.delenv("LSB_REGION_MIN", raising=False)
    kt, dt = KEYS[name]
    keys = raw_keys(name)[:N]
    out_k, out_v, info = sort_columns(lsb_built, keys, None, kt, descending)
    assert info[0][0] == passes
    perm = model_order(keys, kt, descending)
    assert same_bits(out_k, keys[perm]) and np.array_equal(out_v, perm)


# ------------------------------------------------- 5. packed records compose
@pytest.fixture
def small_regions(monkeypatch):
    """Regional first pass, and with it packed records, from 2^16 records on."""
    monkeypatch.setenv("LSB_REGION_MIN", str(1 << 16))
    monkeypatch.delenv("LSB_PACK_VALUES", raising=False)
    monkeypatch.delenv("LSB_REGION_FIRST", raising=False)


@pytest.mark.parametrize("vform", ["argsort", "val4"])
@torch_first
def test_packed_records_compose(lsb_built, small_regions, vform):
    L = lsb_built
    keys = raw_keys("u64")[:N]
    vals = None if vform == "argsort" else some_values(4)[:N]
    out_k, out_v, info = sort_columns(L, keys, vals, 0, False)
    assert info[1] == L.RECORDS_PACKED and info[2] == L.FIRST_REGIONAL and info[0][0] == 8
    perm = model_order(keys, 0, False)
    assert same_bits(out_k, keys[perm])
    assert same_bits(out_v, vals[perm]) if vals is not None else np.array_equal(out_v, perm)


@torch_first
def test_one_wide_value_among_narrow_ones(lsb_built, small_regions):
    L = lsb_built
    keys = raw_keys("u64")[:N]
    vals = np.arange(N, dtype=np.int64)
    vals[123_456] = 2**32 + 5
    out_k, out_v, info = sort_columns(L, keys, vals, 0, True)
    perm = model_order(keys, 0, True)
    assert same_bits(out_k, keys[perm]) and np.array_equal(out_v, vals[perm])


# ------------------------------------------------- 6. several ranks
@pytest.mark.parametrize("descending", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", ["i64", "f32"])
@pytest.mark.parametrize("radix_bits", [8, 16, 64])
@torch_first
def test_three_ranks(lsb_built, radix_bits, name, descending):
    """per = 33335 is odd: ranks 1 and 2 load from blocks aligned to their
    element only."""
    kt, dt = KEYS[name]
    n = 100_003
    assert lsb_built.per_rank(n, 3) % 2 == 1
    keys = tie_keys(name)[:n]
    out_k, out_v, info = sort_columns(lsb_built, keys, None, kt, descending, ranks=3, radix_bits=radix_bits)
    perm = model_order(keys, kt, descending)
    assert same_bits(out_k, keys[perm]) and np.array_equal(out_v, perm)


@torch_first
def test_empty_rank_and_empty_input(lsb_built):
    import torch
    L = lsb_built
    k = torch.tensor([5, -3], dtype=torch.int64, device="cuda")
    sk, si = L.sort(k, ranks=3)
    assert host(sk).tolist() == [-3, 5] and host(si).tolist() == [1, 0]
    sk, sv = L.sort(k, torch.tensor([1.5, 2.5], dtype=torch.float32, device="cuda"), descending=True, ranks=3)
    assert host(sk).tolist() == [5, -3] and host(sv).tolist() == [1.5, 2.5]
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    sk, si = L.sort(e, ranks=3)
    assert sk.numel() == 0 and si.numel() == 0 and si.dtype == torch.int64 and sk.dtype == torch.float32


# ------------------------------------------------- 7. the existing oracle
@torch_first
def test_columns_of_generated_records_against_the_oracle(lsb_built, oracle_mod):
    import torch
    L = lsb_built
    n, P = 65_537, 2
    with L.World(n, ranks=P) as w1, L.World(n, ranks=P) as w2:
        w1.generate()
        inp = w1.gather_global()
        dk, dv = dev(inp["key"]), dev(inp["val"])
        for r in range(P):
            lo, h = r * w2.per, w2.here(r)
            w2.load_columns(r, dk[lo:lo + h], dv[lo:lo + h])
        assert np.array_equal(w2.gather_global(), inp)
        w1.my_sort()
        w2.my_sort()
        want = oracle_mod.stable_sort(inp)
        assert np.array_equal(w1.gather_global(), want)
        ok = torch.empty(n, dtype=torch.uint64, device="cuda")
        ov = torch.empty(n, dtype=torch.uint64, device="cuda")
        for r in range(P):
            lo, h = r * w2.per, w2.here(r)
            w2.store_columns(r, ok[lo:lo + h], ov[lo:lo + h])
        assert np.array_equal(host(ok), want["key"]) and np.array_equal(host(ov), want["val"])
        assert w2.check_sorted()


# ------------------------------------------------- 8. lsbsort.sort
@pytest.mark.parametrize("with_values", [False, True], ids=["argsort", "values"])
@pytest.mark.parametrize("ranks", [1, 2])
@torch_first
def test_sort_function_against_torch(lsb_built, ranks, with_values):
    import torch
    L = lsb_built
    for name, descending in (("i64", False), ("f32", True), ("i32", True), ("f64", False)):
        keys = tie_keys(name)[:50_001]
        vals = some_values(4)[:50_001] if with_values else None
        dk = dev(keys)
        dv = None if vals is None else dev(vals)
        sk, sv = L.sort(dk, dv, descending=descending, ranks=ranks)
        assert sk.device == dk.device and sv.device == dk.device and sk.dtype == dk.dtype
        tv, ti = torch.sort(torch.from_numpy(keys.copy()), stable=True, descending=descending)
        assert same_bits(host(sk), tv.numpy())
        if with_values:
            assert sv.dtype == dv.dtype and same_bits(host(sv), vals[ti.numpy()])
            assert same_bits(host(dv), vals)
        else:
            assert sv.dtype == torch.int64 and np.array_equal(host(sv), ti.numpy())
        assert same_bits(host(dk), keys)  # inputs unchanged bit for bit


@torch_first
def test_sort_function_refuses_before_any_library_call(lsb_built, monkeypatch):
    import torch
    L = lsb_built
    good = torch.arange(10, dtype=torch.int64, device="cuda")

    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(L, "_lib", no_library)
    bad = [torch.arange(20, dtype=torch.int64, device="cuda")[::2],            # not contiguous
           torch.zeros((4, 4), dtype=torch.float32, device="cuda"),            # 2-D
           torch.arange(10, dtype=torch.int64)]                                # on the CPU
    for t in bad:
        with pytest.raises(ValueError):
            L.sort(t)
        with pytest.raises(ValueError):
            L.sort(good, t)
    with pytest.raises(ValueError):
        L.sort(good, torch.arange(9, dtype=torch.int64, device="cuda"))       # lengths differ
    with pytest.raises(ValueError):
        L.sort(torch.zeros(10, dtype=torch.int16, device="cuda"))             # no key type under 32 bits


# ------------------------------------------------- 9. rejections
@torch_first
def test_rejections_leave_the_context_usable(lsb_built):
    """Every bad call returns LSB_ERR_INVALID before a kernel is launched (the
    checks of lsb_load_columns / lsb_store_columns in lsb_abi.cpp all precede
    the launch, and a column must lie inside the allocation the runtime
    reports for it), and the context sorts correctly afterwards."""
    import torch
    L = lsb_built
    lib = L._lib()
    INVALID = 1
    big = (1 << 20) + (1 << 18)
    with L.World(big, ranks=1) as w:
        h = w._h
        k = torch.arange(4096, dtype=torch.int64, device="cuda")
        v = torch.arange(4096, dtype=torch.int64, device="cuda")
        kp, vp, c = k.data_ptr(), v.data_ptr(), 4096
        host_arr = np.arange(4096, dtype=np.uint64)
        small = torch.zeros(1 << 17, dtype=torch.int64, device="cuda")  # a fresh 1 MiB tensor
        bigk = torch.zeros(big, dtype=torch.int64, device="cuda")       # as long as the rank's block
        torch.cuda.synchronize()
        load, store = lib.lsb_load_columns, lib.lsb_store_columns
        cases = [
            ("off + cnt > per", lambda f: f(h, 0, big - 100, c, kp, 1, vp, 8, 0)),
            ("rank", lambda f: f(h, 1, 0, c, kp, 1, vp, 8, 0)),
            ("negative off", lambda f: f(h, 0, -1, c, kp, 1, vp, 8, 0)),
            ("key type 6", lambda f: f(h, 0, 0, c, kp, 6, vp, 8, 0)),
            ("flags 2", lambda f: f(h, 0, 0, c, kp, 1, vp, 8, 2)),
            ("val_bytes 3", lambda f: f(h, 0, 0, c, kp, 1, vp, 3, 0)),
            ("val_bytes 8, no values", lambda f: f(h, 0, 0, c, kp, 1, None, 8, 0)),
            ("val_bytes 0 with values", lambda f: f(h, 0, 0, c, kp, 1, vp, 0, 0)),
            ("keys off by 4 bytes", lambda f: f(h, 0, 0, c - 1, kp + 4, 1, vp, 8, 0)),
            ("values off by 4 bytes", lambda f: f(h, 0, 0, c - 1, kp, 1, vp + 4, 8, 0)),
            ("32-bit keys off by 2 bytes", lambda f: f(h, 0, 0, c, kp + 2, 4, None, 0, 0)),
            ("host keys", lambda f: f(h, 0, 0, c, host_arr.ctypes.data, 0, vp, 8, 0)),
            ("host values", lambda f: f(h, 0, 0, c, kp, 0, host_arr.ctypes.data, 8, 0)),
            ("cnt beyond the keys' allocation", lambda f: f(h, 0, 0, big, small.data_ptr(), 0, None, 0, 0)),
            ("cnt beyond the values' allocation", lambda f: f(h, 0, 0, big, bigk.data_ptr(), 0,
                                                              small.data_ptr(), 8, 0)),
        ]
        for what, call in cases:
            for f in (load, store):
                assert call(f) == INVALID, what
            w.generate()
            w.my_sort()
            assert w.verify() == (True, -1), what
        assert store(h, 0, 0, c, None, 0, None, 0, 0) == INVALID      # both pointers NULL on store
        assert load(h, 0, 0, c, None, 0, None, 0, 0) == INVALID       # no keys on load
        assert load(h, 0, 0, 0, None, 0, None, 0, 0) == 0             # cnt == 0: nothing to do
        with pytest.raises(L.LsbError):
            w.load_columns(0, k, off=big - 100)
        # nothing was written by any of them
        assert np.array_equal(host(k), np.arange(4096)) and np.array_equal(host(v), np.arange(4096))
        assert np.array_equal(host_arr, np.arange(4096, dtype=np.uint64))
        # and the columns still work
        w.load_columns(0, k, v, descending=True)
        rec = w.copy_out(0, 0, c)
        assert np.array_equal(rec["val"], np.arange(4096, dtype=np.uint64))
        assert np.array_equal(rec["key"], model_encode(np.arange(4096, dtype=np.uint64), 1, True))
