"""Ordering by several columns on the device: lsb_rekey_columns and
lsb_rekey_index (k_rekey, lsb_columns.hip) and the front ends built on them,
lsbsort.sort_by, sort_rows, segment_sort and group_quantile; include/lsb.h
"ordering by several columns", DESIGN.md §7.9.

The oracle is numpy over the mapped keys: a vectorised encode (checked against
lsbsort.key_encode), a gather for the rekey, numpy.lexsort for the orders.
Everything is integer and is compared exactly.

The columns are torch CUDA tensors, so (as tests/test_join_gpu.py) the tests
run in one child pytest process over this same file that imports torch before
the library is loaded (LSB_REKEY_CHILD=1), once per session; here each test
reports what its namesake did there.
"""
import functools
import inspect
import itertools
import os
import re
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_REKEY_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, STATE = 0, 1, 7
SENT = 0x5555555555555555
U64_MAX = 0xFFFFFFFFFFFFFFFF
GRID_CAP, BLOCK = 8192, 256
ELEM = np.dtype([("key", "<u8"), ("val", "<u8")])
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("rekey") / "child.xml"
    env = dict(os.environ, LSB_REKEY_CHILD="1")
    for name in ("LSB_REGION_MIN", "LSB_PACK_VALUES", "LSB_REGION_FIRST"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider",
                        "--junitxml", str(xml)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
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


def group():
    """E: the records one thread of k_rekey takes per iteration."""
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_columns.hip")).read()
    return int(re.search(r"#define LSB_REKEY_GROUP (\d+)", src).group(1))


# ------------------------------------------------------------------ the model
def bits_of(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def encode(a, kt, descending=False):
    """lsb_key_encode over a typed numpy column, vectorised."""
    width = 32 if kt >= 3 else 64
    mask = np.uint64((1 << width) - 1)
    sign = np.uint64(1 << (width - 1))
    k = bits_of(a) & mask
    if kt in (1, 4):
        k = k ^ sign
    elif kt in (2, 5):
        k = np.where((k & sign) != 0, ~k & mask, k ^ sign)
    if descending:
        k = ~k & mask
    return k


def typed_column(name, n, seed, distinct=None):
    """A numpy column of one key type: the type's extremes, a few small
    values (ties) and random ones; floats with NaNs of both signs, both zeros
    and both infinities."""
    kt, dt = KEYS[name]
    rng = np.random.default_rng(seed)
    width = 8 * np.dtype(dt).itemsize
    if np.issubdtype(dt, np.floating):
        ut = np.uint32 if width == 32 else np.uint64
        special = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan], dtype=dt)
        neg_nan = (special[-1:].view(ut) | ut(1 << (width - 1))).view(dt)
        pool = np.concatenate([special, neg_nan, rng.standard_normal(24).astype(dt)])
    else:
        raw = rng.integers(0, 1 << 63, 24, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        pool = np.concatenate([np.array([0, 1, 7], dtype=np.uint64), raw,
                               np.array([U64_MAX, 1 << (width - 1), (1 << (width - 1)) - 1], dtype=np.uint64)])
        pool = pool.astype(np.uint32).view(dt) if width == 32 else pool.view(dt)
    if distinct:
        pool = pool[:distinct]
    return np.ascontiguousarray(pool[rng.integers(0, pool.size, n)])


def dev(a):
    """A numpy column as the CUDA tensor that carries its bits."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def host(t):
    return t.cpu().numpy()


def records(vals, seed=1):
    """Records with the given values and keys no rekey would give by chance."""
    rec = np.zeros(len(vals), dtype=ELEM)
    rec["val"] = np.asarray(vals, dtype=np.uint64)
    rec["key"] = np.uint64(SENT) ^ (np.arange(len(vals), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 + seed))
    return rec


def raw_rekey(L, w, rank, ptr, n_col, kt, flags):
    import torch
    torch.cuda.synchronize()
    return L._lib().lsb_rekey_columns(w._h, rank, ptr, n_col, kt, flags)


def check_rekey(L, vals, col, name, descending=False, col_t=None):
    """Records with `vals` rekeyed by `col` (numpy, of key type `name`):
    keys = encode(col[vals]), values and count unchanged."""
    kt = KEYS[name][0]
    vals = np.asarray(vals, dtype=np.uint64)
    t = dev(col) if col_t is None else col_t
    with L.World(len(vals), ranks=1) as w:
        w.copy_in(0, records(vals))
        w.rekey(0, t, descending=descending, key_type=kt)
        got = w.copy_out(0)
    assert np.array_equal(got["val"], vals), (name, "values changed")
    want = encode(col, kt, descending)[vals.astype(np.int64)]
    bad = np.flatnonzero(got["key"] != want)
    assert bad.size == 0, (name, descending, len(vals), "first wrong slot", bad[:5])
    assert np.array_equal(bits_of(host(t)), bits_of(col)), "the column changed"


# ------------------------------------------------- 0. the oracle's encode
@torch_first
def test_model_encode(lsb_built):
    L = lsb_built
    for name, (kt, _) in KEYS.items():
        col = typed_column(name, 200, 5)
        for desc in (False, True):
            assert encode(col, kt, desc).tolist() == [L.key_encode(int(b), kt, desc) for b in bits_of(col)]


# ------------------------------------------------- 1. counts around the group and the block
def counts():
    E = group()
    return sorted({1, max(E - 1, 1), E, E + 1, BLOCK * E - 1, BLOCK * E, BLOCK * E + 1, 4097})


@pytest.mark.parametrize("cnt", counts())
@torch_first
def test_counts(lsb_built, cnt):
    """A random permutation's worth of values into a column of cnt keys."""
    rng = np.random.default_rng(cnt)
    col = typed_column("i64", cnt, cnt + 1)
    check_rekey(lsb_built, rng.permutation(cnt), col, "i64")
    col32 = typed_column("f32", cnt, cnt + 2)
    check_rekey(lsb_built, rng.permutation(cnt), col32, "f32", descending=True)


@torch_first
def test_grid_stride(lsb_built):
    """More groups than the grid cap has threads: the second trip of the
    grid-stride loop, and the tail behind it.  Rekey only, no sort."""
    E = group()
    cnt = GRID_CAP * BLOCK * E + BLOCK * E + E - 1
    rng = np.random.default_rng(9)
    n_col = 100003
    col = typed_column("u64", n_col, 10)
    check_rekey(lsb_built, rng.integers(0, n_col, cnt, dtype=np.int64), col, "u64")


# ------------------------------------------------- 2. values
@torch_first
def test_values_repeat_into_one_key(lsb_built):
    """n_col = 1: every record gathers the same element."""
    col = typed_column("i32", 1, 3)
    check_rekey(lsb_built, np.zeros(3001, dtype=np.uint64), col, "i32")


@torch_first
def test_values_heavy_repeats(lsb_built):
    rng = np.random.default_rng(4)
    col = typed_column("f64", 5, 5)
    check_rekey(lsb_built, rng.integers(0, 5, 5000), col, "f64")


@torch_first
def test_column_much_longer_than_the_records(lsb_built):
    rng = np.random.default_rng(6)
    n_col = 1 << 21
    col = typed_column("u64", n_col, 7)
    vals = np.concatenate([[0, n_col - 1], rng.integers(0, n_col, 1000)])
    check_rekey(lsb_built, vals, col, "u64")


@torch_first
def test_values_loaded_as_32_bit(lsb_built):
    """Values that came through lsb_load_columns with val_bytes 4."""
    import torch
    L = lsb_built
    n = 5003
    rng = np.random.default_rng(8)
    vals = rng.permutation(n).astype(np.int32)
    col = typed_column("f64", n, 9)
    with L.World(n, ranks=1) as w:
        w.load_columns(0, dev(np.arange(n, dtype=np.int64)), dev(vals))
        w.rekey(0, dev(col))
        got = w.copy_out(0)
    assert np.array_equal(got["val"], vals.astype(np.uint64))
    assert np.array_equal(got["key"], encode(col, 2)[vals])


# ------------------------------------------------- 3. column forms
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", list(KEYS))
@torch_first
def test_key_forms(lsb_built, name, descending):
    n = 2 * BLOCK * group() + 77
    rng = np.random.default_rng(11)
    check_rekey(lsb_built, rng.integers(0, n, n), typed_column(name, n, 12), name, descending=descending)


@pytest.mark.parametrize("name", ["i64", "f32"])
@torch_first
def test_column_aligned_to_its_element_only(lsb_built, name):
    """A slice that starts at element 1: 8- or 4-byte alignment, not 16."""
    n = 3000
    rng = np.random.default_rng(13)
    full = typed_column(name, n + 1, 14)
    t = dev(full)[1:]
    assert t.data_ptr() % 16 != 0 and t.data_ptr() % full.dtype.itemsize == 0
    check_rekey(lsb_built, rng.integers(0, n, n), full[1:], name, col_t=t)


# ------------------------------------------------- 4. the slots behind `here`
@torch_first
def test_last_rank_slots_beyond_here_stay(lsb_built):
    """here < per on the last rank: its other slots, filled through copy_in
    with values no column has, are not read, not written and not reported."""
    L = lsb_built
    n, P = 10, 4
    col = typed_column("i64", n, 15)
    t = dev(col)
    with L.World(n, ranks=P) as w:
        assert w.per == 3 and w.here(3) == 1
        fill = records([7, U64_MAX, n], seed=2)
        w.copy_in(3, fill)
        for r in range(3):
            w.copy_in(r, records([(3 * r + j) % n for j in range(3)]))
        for r in range(P):
            w.rekey(r, t)
        got = w.copy_out(3, 0, 3)
        assert got[0]["key"] == encode(col, 1)[7] and got[0]["val"] == 7
        assert got[1:].tobytes() == fill[1:].tobytes()
        for r in range(3):
            assert np.array_equal(w.copy_out(r)["key"], encode(col, 1)[[(3 * r + j) % n for j in range(3)]])


# ------------------------------------------------- 5. rekey_index
@torch_first
def test_rekey_index_one_restores_input_order(lsb_built):
    L = lsb_built
    n = 40001
    keys = typed_column("i64", n, 16)
    for P in (1, 3):
        with L.World(n, ranks=P) as w:
            for r in range(P):
                lo, h = r * w.per, w.here(r)
                w.load_columns(r, dev(keys[lo:lo + h]))
            w.my_sort()
            assert not np.array_equal(w.gather_global()["val"], np.arange(n, dtype=np.uint64))
            for r in range(P):
                w.rekey_index(r, 1)
            w.my_sort()
            got = w.gather_global()
        assert np.array_equal(got["val"], np.arange(n, dtype=np.uint64))
        assert np.array_equal(got["key"], np.arange(n, dtype=np.uint64))


@pytest.mark.parametrize("divisor", [33, 4099, (1 << 32) + 5])
@torch_first
def test_rekey_index_divides(lsb_built, divisor):
    L = lsb_built
    rng = np.random.default_rng(17)
    vals = np.concatenate([rng.integers(0, 1 << 63, 3000, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                           np.array([0, divisor - 1, divisor, U64_MAX], dtype=np.uint64)])
    with L.World(len(vals), ranks=1) as w:
        w.copy_in(0, records(vals))
        w.rekey_index(0, divisor)
        got = w.copy_out(0)
    assert np.array_equal(got["val"], vals)
    assert np.array_equal(got["key"], vals // np.uint64(divisor))


@torch_first
def test_rekey_index_above_every_value_gives_constant_keys(lsb_built):
    """All-zero keys, and the next sort runs no pass beyond what a sort of
    constant keys runs."""
    L = lsb_built
    n = 20000
    rng = np.random.default_rng(18)
    with L.World(n, ranks=1) as w:
        const = np.zeros(n, dtype=ELEM)
        const["val"] = np.arange(n)
        w.copy_in(0, const)
        w.my_sort()
        constant_passes = w.last_sort()[0]
        w.copy_in(0, records(rng.permutation(n)))
        w.rekey_index(0, n)
        got = w.copy_out(0)
        assert not got["key"].any()
        w.my_sort()
        assert w.last_sort()[0] <= constant_passes, (w.last_sort(), constant_passes)
        assert np.array_equal(w.copy_out(0)["val"], got["val"])  # stable: nothing moved


# ------------------------------------------------- 6. values that are no index
@pytest.mark.parametrize("where", ["first", "middle", "last", "all ones"])
@torch_first
def test_out_of_range(lsb_built, where):
    """LSB_ERR_INVALID after the kernel; every value and every out-of-range
    record bit for bit as before, the others rekeyed; a correct rekey and a
    sort afterwards give the oracle's order."""
    L = lsb_built
    n = n_col = 3 * BLOCK * group() + 5
    rng = np.random.default_rng(19)
    room = typed_column("i64", n_col + 1, 20)  # one element more than the call is told of
    t = dev(room)
    vals = rng.permutation(n).astype(np.uint64)
    at = {"first": 0, "middle": n // 2, "last": n - 1, "all ones": n // 3}[where]
    vals[at] = U64_MAX if where == "all ones" else n_col
    rec = records(vals)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, rec)
        assert raw_rekey(L, w, 0, t.data_ptr(), n_col, 1, 0) == INVALID
        got = w.copy_out(0)
        assert np.array_equal(got["val"], vals)
        assert got[at].tobytes() == rec[at].tobytes()
        others = np.arange(n) != at
        assert np.array_equal(got["key"][others], encode(room, 1)[vals[others].astype(np.int64)])
        if where == "all ones":  # no column is that long: the caller mends the record
            vals[at] = 3
            w.copy_in(0, records(vals[at:at + 1]), off=at)
        assert raw_rekey(L, w, 0, t.data_ptr(), n_col + 1, 1, 0) == OK
        w.my_sort()
        got = w.copy_out(0)
    want = vals[np.argsort(encode(room, 1)[vals.astype(np.int64)], kind="stable")]
    assert np.array_equal(got["val"], want)


# ------------------------------------------------- 7. refusals before the launch
@torch_first
def test_refusals_before_launch(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = 1000
    col = dev(np.arange(n, dtype=np.int64))
    col32 = dev(np.arange(n, dtype=np.int32))
    small = torch.zeros(16, dtype=torch.int64, device="cuda")
    host_arr = np.zeros(n, dtype=np.int64)
    big = (1 << 20) + (1 << 18)
    rec = records(np.arange(n) % 7)
    with L.World(n, ranks=2) as w:
        h = w._h
        for r in range(2):
            w.copy_in(r, rec[r * w.per:(r + 1) * w.per])
        kp = col.data_ptr()
        torch.cuda.synchronize()
        f, g = lib.lsb_rekey_columns, lib.lsb_rekey_index
        cases = [("rank -1", lambda: f(h, -1, kp, n, 1, 0)),
                 ("rank P", lambda: f(h, 2, kp, n, 1, 0)),
                 ("null column", lambda: f(h, 0, None, n, 1, 0)),
                 ("n_col 0", lambda: f(h, 0, kp, 0, 1, 0)),
                 ("n_col negative", lambda: f(h, 0, kp, -5, 1, 0)),
                 ("key type 6", lambda: f(h, 0, kp, n, 6, 0)),
                 ("key type -1", lambda: f(h, 0, kp, n, -1, 0)),
                 ("flag bit 1", lambda: f(h, 0, kp, n, 1, 2)),
                 ("64-bit column off by 4 bytes", lambda: f(h, 0, kp + 4, n - 1, 1, 0)),
                 ("32-bit column off by 2 bytes", lambda: f(h, 0, col32.data_ptr() + 2, n - 1, 4, 0)),
                 ("host column", lambda: f(h, 0, host_arr.ctypes.data, n, 1, 0)),
                 ("n_col beyond the allocation", lambda: f(h, 0, small.data_ptr(), big, 1, 0)),
                 ("index: rank -1", lambda: g(h, -1, 1)),
                 ("index: rank P", lambda: g(h, 2, 1)),
                 ("divisor 0", lambda: g(h, 0, 0))]
        for what, call in cases:
            assert call() == INVALID, what
            got = np.concatenate([w.copy_out(r) for r in range(2)])
            assert got.tobytes() == rec.tobytes(), (what, "changed the records")
        assert f(None, 0, kp, n, 1, 0) == INVALID and g(None, 0, 1) == INVALID
        # and the context is usable afterwards
        for r in range(2):
            w.rekey(r, col)
        got = np.concatenate([w.copy_out(r) for r in range(2)])
        assert np.array_equal(got["key"], encode(np.arange(n, dtype=np.int64), 1)[np.arange(n) % 7])


@torch_first
def test_empty_rank_does_not_examine_the_pointer(lsb_built):
    L = lsb_built
    with L.World(5, ranks=4) as w:
        assert w.here(3) == 0
        assert raw_rekey(L, w, 3, None, 5, 1, 0) == OK
        assert raw_rekey(L, w, 3, 12345, 5, 1, 0) == OK
        assert L._lib().lsb_rekey_index(w._h, 3, 1) == OK


# ------------------------------------------------- 8. plans end
@pytest.mark.parametrize("call", ["rekey", "rekey_index"])
@torch_first
def test_plans_end(lsb_built, call):
    """After either call store_runs, store_reduce, store_scan, store_select
    and store_join return LSB_ERR_STATE; a search after the next sort answers
    for the new keys."""
    import torch
    L = lsb_built
    n = 6000
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 50, n).astype(np.int64)
    other = rng.integers(0, 1000, n).astype(np.int64)
    kt, ot = dev(keys), dev(other)
    out = lambda m=n: torch.zeros(m, dtype=torch.int64, device="cuda")  # noqa: E731
    with L.World(n, ranks=1) as w:
        w.load_columns(0, kt)
        w.my_sort()
        w.count_runs()
        w.plan_reduce(L.REDUCE_SUM, L.KEY_I64)
        w.plan_scan(L.SCAN_SUM, L.KEY_I64)
        w.select(10)
        q = dev(np.arange(60, dtype=np.int64))
        cnt = out(60)
        w.search(0, q, cnt, side="count")
        assert np.array_equal(host(cnt), np.bincount(keys, minlength=60))
        assert w.join_count(0, q) == n
        # every plan answers now
        assert w.store_runs(0, keys=out(), starts=out(), counts=out()) == 50
        assert w.store_reduce(0, out()) == 50 and w.store_scan(0, out()) == n
        assert w.store_select(0, keys=out(), values=out()) == 11
        assert w.store_join(0, left=out(), right=out(), pos=out()) == n
        if call == "rekey":
            w.rekey(0, ot)
            new = other
        else:
            w.rekey_index(0, 7)
            new = np.arange(n, dtype=np.int64) // 7
        for what, store in [("store_runs", lambda: w.store_runs(0, keys=out(), starts=out(), counts=out())),
                            ("store_reduce", lambda: w.store_reduce(0, out())),
                            ("store_scan", lambda: w.store_scan(0, out())),
                            ("store_select", lambda: w.store_select(0, keys=out(), values=out())),
                            ("store_join", lambda: w.store_join(0, left=out(), right=out(), pos=out()))]:
            with pytest.raises(L.LsbError) as e:
                store()
            assert e.value.code == STATE, what
        w.my_sort()
        q2 = dev(np.arange(1000, dtype=np.int64))
        cnt2 = out(1000)
        w.search(0, q2, cnt2, side="count", key_type=None if call == "rekey" else L.KEY_U64)  # index keys are raw
        assert np.array_equal(host(cnt2), np.bincount(new, minlength=1000)[:1000])


# ------------------------------------------------- 9. sort_by
def sort_by_columns(n, seed):
    """int32 with 7 distinct values as primary; float32 with NaNs of both
    signs and both zeros; int64 as last."""
    a = typed_column("i32", n, seed, distinct=7)
    b = typed_column("f32", n, seed + 1, distinct=10)
    c = typed_column("i64", n, seed + 2)
    return [(a, 4), (b, 5), (c, 1)]


def lexsort_oracle(cols, desc):
    enc = [encode(c, kt, d) for (c, kt), d in zip(cols, desc)]
    return np.lexsort(enc[::-1])


@pytest.mark.parametrize("n,P", [(10000, 1), (10000, 3), (5, 4)])
@torch_first
def test_sort_by_three_columns(lsb_built, n, P):
    L = lsb_built
    cols = sort_by_columns(n, 30 + n)
    if n == 10000:
        b = cols[1][0]
        assert np.isnan(b).any() and (bits_of(b) == 0x80000000).any() and (bits_of(b) == 0).any()
        assert (np.isnan(b) & (bits_of(b) >> np.uint64(31) == 1)).any()
    ts = [dev(c) for c, _ in cols]
    keep = [host(t).copy() for t in ts]
    for desc in [(False, False, False), (True, False, True)]:
        got = L.sort_by(ts, list(desc), ranks=P)
        assert got.dtype == __import__("torch").int64
        assert np.array_equal(host(got), lexsort_oracle(cols, desc)), (n, P, desc)
    assert all(np.array_equal(bits_of(host(t)), bits_of(k)) for t, k in zip(ts, keep)), "the inputs changed"


@pytest.mark.parametrize("desc", list(itertools.product((False, True), repeat=2)),
                         ids=lambda d: "".join("d" if x else "a" for x in d))
@torch_first
def test_sort_by_two_columns_every_direction(lsb_built, desc):
    L = lsb_built
    n = 10000
    cols = sort_by_columns(n, 50)[:2]
    got = L.sort_by([dev(c) for c, _ in cols], list(desc))
    assert np.array_equal(host(got), lexsort_oracle(cols, desc))
    one = L.sort_by([dev(c) for c, _ in cols], desc[0]) if desc[0] == desc[1] else None
    if one is not None:  # one bool stands for every column
        assert np.array_equal(host(one), host(got))


@torch_first
def test_sort_by_one_column_is_sort(lsb_built):
    L = lsb_built
    x = dev(typed_column("f32", 10000, 60, distinct=12))
    for desc in (False, True):
        assert np.array_equal(host(L.sort_by([x], desc)), host(L.sort(x, descending=desc)[1]))
    assert L.sort_by([x[:0]]).numel() == 0


@torch_first
def test_sort_by_int32_primary_passes(lsb_built):
    """The final sort of an LSD sort over columns, keyed by an int32 column,
    runs at most 4 local passes; after sort_rows' rekey on 300 rows, at most 2."""
    L = lsb_built
    n = 300 * 33
    rng = np.random.default_rng(61)
    prim = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    last = typed_column("i64", n, 62)
    with L.World(n, ranks=1) as w:
        w.load_columns(0, dev(last))
        w.my_sort()
        w.rekey(0, dev(prim))
        w.my_sort()
        assert w.last_sort()[0] <= 4, w.last_sort()
        got = w.copy_out(0)["val"]
        assert np.array_equal(got, np.lexsort([encode(last, 1), encode(prim, 4)]))
        w.rekey_index(0, 33)
        w.my_sort()
        assert w.last_sort()[0] <= 2, w.last_sort()


# ------------------------------------------------- 10. sort_rows
@pytest.mark.parametrize("name", ["i64", "i32", "f32"])
@pytest.mark.parametrize("shape", [(1, 4099), (4099, 1), (7, 4099), (300, 33)], ids=lambda s: "%dx%d" % s)
@torch_first
def test_sort_rows(lsb_built, shape, name):
    import torch
    L = lsb_built
    R, C = shape
    flat = typed_column(name, R * C, 70 + R, distinct=None if name != "f32" else 14)
    x = dev(flat).reshape(R, C)
    for desc in (False, True):
        sk, idx = L.sort_rows(x, descending=desc, ranks=1 if R != 7 else 2)
        assert sk.shape == x.shape and idx.shape == x.shape and idx.dtype == torch.int64 and sk.dtype == x.dtype
        if name == "f32":  # the mapped-key oracle: stable argsort per row
            enc = encode(flat, 5, desc).reshape(R, C)
            want = np.argsort(enc, axis=1, kind="stable")
            assert np.array_equal(host(idx), want)
            assert np.array_equal(bits_of(host(sk).reshape(-1)),
                                  bits_of(np.take_along_axis(flat.reshape(R, C), want, axis=1).reshape(-1)))
        else:
            tk, ti = torch.sort(x, dim=-1, stable=True, descending=desc)
            assert torch.equal(idx, ti) and torch.equal(sk, tk)
    assert np.array_equal(bits_of(host(x).reshape(-1)), bits_of(flat)), "the input changed"


# ------------------------------------------------- 11. segment_sort
def segment_oracle(keys, kt, offsets, desc):
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return np.lexsort([encode(keys, kt, desc), seg])


@pytest.mark.parametrize("case", ["empty segments", "one segment", "segments of one"])
@torch_first
def test_segment_sort(lsb_built, case):
    import torch
    L = lsb_built
    n = 3001
    keys = typed_column("f64", n, 80, distinct=20)
    offsets = {"empty segments": [0, 0, 5, 5, n], "one segment": [0, n], "segments of one": list(range(n + 1))}[case]
    kt = dev(keys)
    for desc in (False, True):
        for off in (torch.tensor(offsets, dtype=torch.int64), torch.tensor(offsets, dtype=torch.int64).cuda()):
            sk, idx = L.segment_sort(kt, off, descending=desc)
            want = segment_oracle(keys, 2, np.array(offsets), desc)
            assert np.array_equal(host(idx), want), (case, desc)
            assert np.array_equal(bits_of(host(sk)), bits_of(keys[want]))
    if case == "segments of one":
        assert np.array_equal(host(idx), np.arange(n))
    for bad in ([0, 5, 4, n], [0, n + 1], [1, n], [0, n - 1]):
        with pytest.raises(ValueError):
            L.segment_sort(kt, torch.tensor(bad, dtype=torch.int64))


# ------------------------------------------------- 12. group_quantile
def quantile_oracle(keys, kkt, values, vkt, q, desc):
    ek, ev = encode(keys, kkt, desc), encode(values, vkt)
    order = np.lexsort([ev, ek])
    uk, uv = [], []
    i = 0
    while i < len(order):
        j = i
        while j < len(order) and ek[order[j]] == ek[order[i]]:
            j += 1
        uk.append(keys[order[i]])
        uv.append(values[order[i + int(np.floor(np.float64(q) * np.float64(j - i - 1)))]])
        i = j
    return np.array(uk, dtype=keys.dtype), np.array(uv, dtype=values.dtype)


@pytest.mark.parametrize("q", [0, 0.25, 0.5, 1])
@torch_first
def test_group_quantile(lsb_built, q):
    L = lsb_built
    n = 4000
    keys = typed_column("i32", n, 90, distinct=9)
    values = typed_column("f64", n, 91)
    for desc in (False, True):
        uk, uv = L.group_quantile(dev(keys), dev(values), q=q, descending=desc)
        wk, wv = quantile_oracle(keys, 4, values, 2, q, desc)
        assert np.array_equal(host(uk), wk) and np.array_equal(bits_of(host(uv)), bits_of(wv)), (q, desc)


@torch_first
def test_group_quantile_group_across_ranks(lsb_built):
    """Two ranks, and a group whose records lie on both."""
    L = lsb_built
    n = 1001
    rng = np.random.default_rng(92)
    keys = np.where(rng.random(n) < 0.6, 5, rng.integers(0, 10, n)).astype(np.int64)
    values = rng.integers(-1000, 1000, n).astype(np.int64)
    srt = np.sort(keys)
    assert srt[500] == srt[501] == 5  # the group of 5 spans the ranks' boundary
    for q in (0, 0.5, 1):
        uk, uv = L.group_quantile(dev(keys), dev(values), q=q, ranks=2)
        wk, wv = quantile_oracle(keys, 1, values, 1, q, False)
        assert np.array_equal(host(uk), wk) and np.array_equal(host(uv), wv), q
    with pytest.raises(ValueError):
        L.group_quantile(dev(keys), dev(values), q=1.5)
