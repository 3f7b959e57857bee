"""A column of queries against the sorted records on the device: lower bound,
upper bound and match count (lsb_search, lsbsort.searchsorted / count_of / isin;
include/lsb.h "searching the sorted records").

The oracle is numpy.searchsorted(mapped sorted keys, mapped queries, side) on
the host, the key mapping written out below from the header's table
(tests/test_select_gpu.py's model).  Records are loaded with copy_in, sorted on
the host, so no test depends on the sort.

The columns are torch CUDA tensors, so (as tests/test_select_gpu.py) the tests
run in one child pytest process over this same file that imports torch before
the library is loaded (LSB_SEARCH_CHILD=1), once per session; here each test
reports what its namesake did there.
"""
import functools
import inspect
import os
import re
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_SEARCH_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
OK, INVALID = 0, 1
LOWER, UPPER, COUNT, ADD = 0, 1, 2, 4
SIDES = ("left", "right", "count")
SENT = 0x5555555555555555
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
ELEM = np.dtype([("key", "<u8"), ("val", "<u8")])
# name -> (LSB_KEY_*, numpy dtype)
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("search") / "child.xml"
    env = dict(os.environ, LSB_SEARCH_CHILD="1")
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


def host(t):
    return t.cpu().numpy()


def records(keys):
    """Records of these mapped keys whose value is the global index."""
    rec = np.zeros(keys.size, dtype=ELEM)
    rec["key"] = keys
    rec["val"] = np.arange(keys.size, dtype=np.uint64)
    return rec


def model(sorted_keys, queries):
    """{side: int64 counts} of mapped queries against mapped sorted keys."""
    sorted_keys = np.ascontiguousarray(sorted_keys, dtype=np.uint64)
    queries = np.ascontiguousarray(queries, dtype=np.uint64)
    lo = np.searchsorted(sorted_keys, queries, "left").astype(np.int64)
    hi = np.searchsorted(sorted_keys, queries, "right").astype(np.int64)
    return {"left": lo, "right": hi, "count": hi - lo}


def column(q):
    """uint64 queries as the int64 CUDA tensor that carries their bits."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, dtype=np.uint64).view(np.int64).copy()).cuda()


def search(w, rank, qt, side, add=False, out=None, **kw):
    """World.search into a fresh sentinel column (or into out) -> numpy."""
    import torch
    if out is None:
        out = torch.full((qt.numel(),), SENT, dtype=torch.int64, device="cuda")
    w.search(rank, qt, out, side=side, add=add, key_type=kw.pop("key_type", 0), **kw)
    return host(out)


def check_one_rank(w, sorted_keys, q, what):
    want = model(sorted_keys, q)
    qt = column(q)
    for side in SIDES:
        got = search(w, 0, qt, side)
        assert np.array_equal(got, want[side]), (what, side, q.size)


def query_pool(sorted_keys, seed):
    """first and last key, 0 and 2^64 - 1, then every distinct key and every
    key - 1 and + 1 (wrapping), shuffled."""
    d = np.unique(sorted_keys)
    rest = np.concatenate([d, d - np.uint64(1), d + np.uint64(1)])
    np.random.default_rng(seed).shuffle(rest)
    return np.concatenate([np.array([sorted_keys[0], sorted_keys[-1], 0, U64_MAX], dtype=np.uint64), rest])


# ------------------------------------------------- 1. tile and block edges, one rank
def edge_keys(n):
    """Sorted keys: sparse odd keys (so key - 1 and key + 1 miss) with short
    runs of equal keys among them; and the same with 0 and 2^64 - 1 at the ends."""
    rng = np.random.default_rng(31 + n)
    sparse = rng.integers(1, 1 << 62, n, dtype=np.int64).astype(np.uint64) * np.uint64(4) + np.uint64(1)
    runs = sparse.copy()
    for at in rng.integers(0, n, max(1, n // 50)):
        runs[at:at + int(rng.integers(2, 40))] = runs[at]
    ends = np.sort(runs)
    ends[0], ends[-1] = 0, U64_MAX
    return {"sparse": np.sort(sparse), "short runs": np.sort(runs), "0 and 2^64 - 1 at the ends": ends}


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@torch_first
def test_tile_and_block_edges_one_rank(lsb_built, n):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        for name, keys in edge_keys(n).items():
            w.copy_in(0, records(keys))
            pool = query_pool(keys, n)
            for j, m in enumerate((1, 63, 64, 65, 257, 1000)):  # a window of the pool each
                check_one_rank(w, keys, np.resize(np.roll(pool, -4 * j), m), name)
            check_one_rank(w, keys, pool, (name, "the whole pool"))


# ------------------------------------------------- 2. runs longer than a tile
LONG_N = 5 * TILE + 7


def long_run_layouts():
    """Keys of 3 values over LONG_N records, sorted: the middle value covers
    whole tiles, so adjacent fences are equal.  (records of 10, of 20)."""
    return {"inside the tiles": (100, 3 * TILE + 500), "from a tile's first record": (TILE, 2 * TILE + 9),
            "up to a tile's last record": (777, 3 * TILE - 777), "whole tiles exactly": (TILE, 3 * TILE),
            "one record into the next tile": (TILE - 1, 2 * TILE + 2), "the first value fills two tiles": (2 * TILE, 5),
            "the last value is one record": (TILE + 3, LONG_N - TILE - 4)}


@torch_first
def test_runs_longer_than_a_tile(lsb_built):
    L = lsb_built
    q = np.array([0, 9, 10, 11, 19, 20, 21, 29, 30, 31, 1 << 63, U64_MAX] * 11, dtype=np.uint64)  # 132: three waves
    with L.World(LONG_N, ranks=1) as w:
        for name, (a, b) in long_run_layouts().items():
            keys = np.repeat(np.array([10, 20, 30], dtype=np.uint64), [a, b, LONG_N - a - b])
            w.copy_in(0, records(keys))
            check_one_rank(w, keys, q, name)
            want = model(keys, q[:12])
            assert want["left"][5] == a and want["right"][5] == a + b and want["count"][5] == b  # the oracle sees the run
        for value in (0, 20, int(U64_MAX)):
            keys = np.full(LONG_N, value, dtype=np.uint64)
            w.copy_in(0, records(keys))
            check_one_rank(w, keys, q, ("all equal", value))


# ------------------------------------------------- 3. more queries than one grid sweep
@torch_first
def test_more_queries_than_one_sweep(lsb_built):
    L = lsb_built
    n, m = TILE + 1, (1 << 20) + 3
    rng = np.random.default_rng(3)
    keys = np.sort(rng.integers(0, 1 << 16, n).astype(np.uint64) << np.uint64(40))
    q = rng.integers(0, 1 << 17, m).astype(np.uint64) << np.uint64(39)  # every other one can hit
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        check_one_rank(w, keys, q, "2^20 + 3 queries")
    assert model(keys, q)["count"].max() >= 1


# ------------------------------------------------- 4. loopback ranks
def rank_cases(P):
    """(name, sorted keys) whose last rank is short: random keys with ties; a
    run that straddles the first rank boundary; from three ranks on, a value
    that fills a whole middle rank and both its neighbours' edges."""
    rng = np.random.default_rng(40 + P)
    per = TILE + 37
    n = P * per - (P - 1)  # ceil(n / P) == per, the last rank P - 1 records short
    base = np.sort(rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(20))
    out = [("random with ties", base)]
    straddle = base.copy()
    straddle[per - 600:per + 900] = straddle[per - 600]
    out.append(("a run over a rank boundary", np.sort(straddle)))
    if P >= 3:
        mid = base.copy()
        mid[per - 5:2 * per + 11] = mid[per - 5]
        out.append(("a value fills a whole middle rank", np.sort(mid)))
    return out


def search_all_ranks(w, qt, side):
    """ADD over the non-empty ranks, from the second on, into one column."""
    import torch
    out = torch.full((qt.numel(),), SENT, dtype=torch.int64, device="cuda")
    ranks = [r for r in range(w.P) if w.here(r)]
    for i, r in enumerate(ranks):
        w.search(r, qt, out, side=side, add=i > 0, key_type=0)
    return host(out)


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_loopback_ranks(lsb_built, P):
    L = lsb_built
    for name, keys in rank_cases(P):
        n = keys.size
        q = query_pool(keys, P)
        qt = column(q)
        want = model(keys, q)
        with L.World(n, ranks=P) as w:
            assert w.per == TILE + 37 and 0 < w.here(P - 1) < w.per
            w.scatter_global(records(keys))
            for side in SIDES:
                assert np.array_equal(search_all_ranks(w, qt, side), want[side]), (name, side)
            if name == "a value fills a whole middle rank":  # the middle rank alone: every record of it, or none
                v = keys[w.per]
                alone = search(w, 1, column(np.array([v, v - np.uint64(1), v + np.uint64(1)])), "count")
                assert list(alone) == [w.per, 0, 0]
    # a trailing rank without records
    n = 6 if P == 5 else P - 1
    keys = np.array([0, 1, 3, 3, 3, 3][:n], dtype=np.uint64)
    q = np.array([0, 1, 2, 3, 4, U64_MAX] * 11, dtype=np.uint64)
    qt = column(q)
    want = model(keys, q)
    with L.World(n, ranks=P) as w:
        assert w.here(P - 1) == 0
        w.scatter_global(records(keys))
        for side in SIDES:
            assert np.array_equal(search_all_ranks(w, qt, side), want[side]), ("empty ranks", side)
            assert not search(w, P - 1, qt, side).any(), ("an empty rank writes zeros", side)


# ------------------------------------------------- 5. ADD
@torch_first
def test_add(lsb_built):
    import torch
    L = lsb_built
    n = TILE + 9
    rng = np.random.default_rng(5)
    keys = np.sort(rng.integers(0, 500, n).astype(np.uint64))
    q = rng.integers(0, 520, 777).astype(np.uint64)
    start = rng.integers(-(1 << 40), 1 << 40, q.size).astype(np.int64)
    qt = column(q)
    want = model(keys, q)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        for side in SIDES:
            got = search(w, 0, qt, side, add=True, out=torch.from_numpy(start.copy()).cuda())
            assert np.array_equal(got, start + want[side]), side
            assert np.array_equal(search(w, 0, qt, side), want[side]), side  # without ADD the column's contents do not matter
    with L.World(1, ranks=2) as w:  # rank 1 holds nothing
        w.copy_in(0, records(keys[:1]))
        for side in SIDES:
            got = search(w, 1, qt, side, add=True, out=torch.from_numpy(start.copy()).cuda())
            assert np.array_equal(got, start), side
            assert not search(w, 1, qt, side).any(), side


# ------------------------------------------------- 6. typed front ends
N = 20_003


@functools.lru_cache(maxsize=None)
def typed_keys(name, n=N, seed=20):
    """n keys of at most 2^12 distinct values spread over every byte of the
    type, negative ones included; f32 without NaN and -0.0 (test_every_key_form
    has them); f64 with both zeros, both infinities and NaNs of both signs."""
    kt, dt = KEYS[name]
    v = np.random.default_rng(seed + kt).integers(0, 4096, n).astype(np.int64)
    if name == "i64":
        a = (v - 2048) * np.int64(0x0002_0008_0200_0801)
    elif name == "u64":
        a = v.astype(np.uint64) * np.uint64(0x0010_0401_0040_1001)  # up to the top bit
    elif name == "u32":
        a = (v * 0x00100401 % (1 << 32)).astype(np.uint32)
    elif name == "i32":
        a = ((v - 2048) * 0x00080201).astype(np.int32)
    else:
        a = ((v - 2048) * 0.37).astype(dt) * np.where(v % 3 == 0, dt(1e20), dt(1.0)).astype(dt)
        if name == "f64":
            b = a.view(np.uint64).copy()
            for val, bits in ((7, 0x8000000000000000), (9, 0), (11, 0x7ff8000000000001), (13, 0xfff8000000000002),
                              (15, 0x7ff0000000000000), (17, 0xfff0000000000000)):
                b[v == val] = bits
            a = b.view(np.float64)
    a = np.ascontiguousarray(a.astype(dt))
    a.setflags(write=False)
    return a


def typed_queries(name):
    """Half drawn like the keys from another seed (hits and misses), half of
    them with the lowest bit flipped; f64: every special of the keys, and a
    NaN with another payload of each sign, which equals no key."""
    kt, dt = KEYS[name]
    a = typed_keys(name, 6001, seed=77)
    b = bits_of(a).copy()
    b[::2] ^= np.uint64(1)
    if name == "f64":
        b[:10] = [0x8000000000000000, 0, 0x7ff8000000000001, 0xfff8000000000002, 0x7ff0000000000000,
                  0xfff0000000000000, 0x7ff8000000000003, 0xfff8000000000004, 0x0000000000000001, 0x8000000000000001]
    wide = np.dtype(dt).itemsize == 8
    return np.ascontiguousarray(b.astype(np.uint64 if wide else np.uint32).view(dt))


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("name,descending", [("i64", False), ("f32", True), ("u32", False), ("f64", False),
                                             ("u64", False), ("i32", True)])
@torch_first
def test_typed_front_ends(lsb_built, name, descending, ranks):
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    keys, queries = typed_keys(name), typed_queries(name)
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)  # uint columns travel as tensors of the same width
    dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
    dq = torch.from_numpy(queries.view(key_np).copy()).cuda()
    if name == "u32":  # a column that starts 4 bytes into its allocation
        dq = dq[1:]
        queries = queries[1:]
    key_type = kt if name in ("u64", "u32") else None
    kw = dict(descending=descending, ranks=ranks, key_type=key_type)
    want = model(np.sort(model_encode(bits_of(keys), kt, descending)), model_encode(bits_of(queries), kt, descending))
    assert want["count"].max() > 1 and (want["count"] == 0).sum() > 100  # hits with ties, and misses
    for side in ("left", "right"):
        got = L.searchsorted(dk, dq, side=side, **kw)
        assert got.dtype == torch.int64 and got.device == dk.device and got.shape == dq.shape
        assert np.array_equal(host(got), want[side]), side
    counts = L.count_of(dk, dq, **kw)
    assert counts.dtype == torch.int64 and np.array_equal(host(counts), want["count"])
    found = L.isin(dq, dk, **kw)
    assert found.dtype == torch.bool and found.shape == dq.shape and np.array_equal(host(found), want["count"] > 0)
    assert np.array_equal(bits_of(host(dk)), bits_of(keys)) and np.array_equal(bits_of(host(dq)), bits_of(queries))
    # keys that are sorted already, in the order asked for: no sort, the same answers
    order = np.argsort(model_encode(bits_of(keys), kt, descending), kind="stable")
    ds = torch.from_numpy(keys[order].view(key_np).copy()).cuda()
    assert np.array_equal(host(L.searchsorted(ds, dq, side="right", assume_sorted=True, **kw)), want["right"])
    if name == "f64":  # the header's order, not torch's: the zeros differ, a NaN equals its own bits only
        c = host(counts)
        b = bits_of(keys)
        for i, bits in enumerate((0x8000000000000000, 0, 0x7ff8000000000001, 0xfff8000000000002)):
            assert c[i] == (b == np.uint64(bits)).sum() > 0, hex(bits)
        assert c[6] == 0 and c[7] == 0
        lo = host(L.searchsorted(dk, dq, **kw))
        assert lo[3] == 0 and lo[2] == N - c[2] and lo[0] + c[0] == lo[1]  # NaNs at both ends, -0.0 right below +0.0
    if name in ("i64", "u32"):  # all finite, ascending, no signed zero: torch agrees
        tk = torch.from_numpy(keys.astype(np.int64)).cuda()
        tq = torch.from_numpy(queries.astype(np.int64)).cuda()
        for side in ("left", "right"):
            tw = torch.searchsorted(torch.sort(tk).values, tq, side=side)
            assert torch.equal(L.searchsorted(dk, dq, side=side, **kw), tw), side
    # no keys, no queries
    z = L.searchsorted(dk[:0], dq, **kw)
    assert z.dtype == torch.int64 and z.shape == dq.shape and not bool(z.any())
    assert not bool(L.count_of(dk[:0], dq, **kw).any())
    f = L.isin(dq, dk[:0], **kw)
    assert f.dtype == torch.bool and f.shape == dq.shape and not bool(f.any())
    assert L.searchsorted(dk, dq[:0], **kw).numel() == 0 and L.isin(dq[:0], dk, **kw).dtype == torch.bool
    other = torch.zeros(4, dtype=torch.float32 if dk.element_size() == 8 else torch.float64, device="cuda")
    for bad in (lambda: L.searchsorted(dk, dq, side="middle", **kw), lambda: L.searchsorted(dk, dq, side="count", **kw),
                lambda: L.searchsorted(dk, other, **kw), lambda: L.count_of(dk, other, **kw),
                lambda: L.isin(other, dk, **kw), lambda: L.searchsorted(dk, dq.cpu(), **kw),
                lambda: L.isin(dq, dk.cpu(), **kw), lambda: L.count_of(dk, dq, ranks=0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------- 7. the fence table's lifetime
@torch_first
def test_fence_lifetime(lsb_built):
    L = lsb_built
    n = 3 * TILE + 5
    rng = np.random.default_rng(7)
    first = np.sort(rng.integers(0, 1 << 40, n).astype(np.uint64))
    second = np.sort(rng.integers(1 << 50, 1 << 60, n).astype(np.uint64))  # every fence differs
    q = np.concatenate([first[::7], second[::7], first[::11] + np.uint64(1)])
    qt = column(q)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(first))
        check_one_rank(w, first, q, "first records")
        w.copy_in(0, records(second))
        check_one_rank(w, second, q, "after copy_in: the answers follow the new records")
        # lsb_select reads A and writes B: the records and the answers stay
        before = {side: search(w, 0, qt, side) for side in SIDES}
        plan = w.select(n // 2)
        assert plan["key"] == int(second[n // 2])
        for side in SIDES:
            assert np.array_equal(search(w, 0, qt, side), before[side]), side
        # every other call that can change A: searched again, the answers are the new records'
        w.copy_in(0, records(first[:TILE + 1]), off=0)  # the front of the rank: no longer sorted as a whole
        mixed = np.concatenate([first[:TILE + 1], second[TILE + 1:]])
        assert np.all(mixed[1:] >= mixed[:-1])  # first's keys lie below second's: still sorted
        check_one_rank(w, mixed, q, "after a partial copy_in")
        unsorted = rng.permutation(second)
        w.copy_in(0, records(unsorted))
        w.my_sort()
        check_one_rank(w, second, q, "after my_sort")


@torch_first
def test_fence_lifetime_every_entry_point(lsb_built):
    """Each call that can change A ends the fence table on its own: a search
    right before it builds the table from other keys, every fence of which
    differs from the keys after it.  (copy_in: test_fence_lifetime.)"""
    L = lsb_built
    n = 3 * TILE + 5
    rng = np.random.default_rng(70)
    first = np.sort(rng.integers(0, 1 << 40, n).astype(np.uint64))
    second = np.sort(rng.integers(1 << 50, 1 << 60, n).astype(np.uint64))
    one = np.uint64(1)
    ends = np.array([0, U64_MAX], dtype=np.uint64)

    def pool(keys):
        return np.concatenate([first[::7], second[::7], first[::11] + one, keys[::5], keys[::13] + one, ends])

    def load_first(w, vals=None):
        """first's keys (values: vals, or the indices) and a search of them."""
        rec = records(first)
        if vals is not None:
            rec["val"] = vals
        w.copy_in(0, rec)
        check_one_rank(w, first, pool(first), "first records")

    def answers(w, q):
        qt = column(q)
        return {side: search(w, 0, qt, side) for side in SIDES}

    def changed(w, before, what, expect=None):
        """A's keys now: sorted, every fence another than before; the answers are theirs."""
        keys = w.copy_out(0)["key"]
        assert np.all(keys[1:] >= keys[:-1]), what
        assert expect is None or np.array_equal(keys, expect), what
        assert np.all(keys[::TILE] != before[::TILE]), what
        check_one_rank(w, keys, pool(keys), what)

    with L.World(n, ranks=1) as w:
        # lsb_sort alone: the table is built from the generated, unsorted records first
        load_first(w)
        w.generate()
        unsorted = w.copy_out(0)["key"]
        assert not w.check_sorted()
        got = answers(w, pool(first))  # unspecified counts, in bounds
        assert all(g.min() >= 0 and g.max() <= n for g in got.values())
        w.my_sort()
        changed(w, unsorted, "after generate and my_sort", np.sort(unsorted))
        # lsb_load_columns
        load_first(w)
        w.load_columns(0, column(second), key_type=0)
        changed(w, first, "after load_columns", second)
        # lsb_pass: the groups of the top byte in falling order, each sorted, so the stable pass on it sorts
        load_first(w)
        top_byte = second >> np.uint64(56)
        assert np.unique(top_byte).size >= 8
        groups = np.concatenate([second[top_byte == b] for b in np.unique(top_byte)[::-1]])
        w.copy_in(0, records(groups))
        assert not w.check_sorted()
        got = answers(w, pool(second))
        assert all(g.min() >= 0 and g.max() <= n for g in got.values())
        w.global_shuffle(7)
        changed(w, groups, "after global_shuffle", second)
        # lsb_label_runs, lsb_scan_runs, BY_VALUE: the old values become the keys
        load_first(w, vals=second)
        w.count_runs()
        w.label_runs(L.LABEL_BY_VALUE)
        changed(w, first, "after label_runs(BY_VALUE)", second)
        load_first(w, vals=second)
        w.count_runs()
        w.plan_scan(L.SCAN_SUM, L.KEY_U64)
        w.scan_runs(L.LABEL_BY_VALUE)
        changed(w, first, "after scan_runs(BY_VALUE)", second)
        # KEEP changes no key: the same answers
        load_first(w)
        q = pool(first)
        before = answers(w, q)
        w.count_runs()
        w.label_runs(L.LABEL_KEEP)
        assert np.array_equal(w.copy_out(0)["key"], first)
        after = answers(w, q)
        assert all(np.array_equal(after[side], before[side]) for side in SIDES), "after label_runs(KEEP)"
        w.count_runs()
        w.plan_scan(L.SCAN_SUM, L.KEY_U64)
        w.scan_runs(L.LABEL_KEEP)
        assert np.array_equal(w.copy_out(0)["key"], first)
        after = answers(w, q)
        assert all(np.array_equal(after[side], before[side]) for side in SIDES), "after scan_runs(KEEP)"
    # lsb_generate alone: one record is sorted whatever it holds
    with L.World(1, ranks=1) as w:
        old = np.array([U64_MAX], dtype=np.uint64)
        w.copy_in(0, records(old))
        check_one_rank(w, old, np.concatenate([old, old - one, ends]), "one record")
        w.generate()
        new = w.copy_out(0)["key"]
        assert new[0] != old[0]
        check_one_rank(w, new, np.concatenate([new, new - one, new + one, old, ends]), "after generate")


# ------------------------------------------------- 8. refusals
@torch_first
def test_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n, m = TILE + 3, 300
    keys = np.sort(np.random.default_rng(8).integers(0, 1000, n).astype(np.uint64))
    q = np.arange(m, dtype=np.uint64) * np.uint64(3)
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, records(keys))
        qt = column(q)
        out = torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda")
        both = torch.full((2 * m,), SENT, dtype=torch.int64, device="cuda")  # queries and out cut from one tensor
        qp, op, bp = qt.data_ptr(), out.data_ptr(), both.data_ptr()
        host_q = q.copy()
        host_out = np.full(m, SENT, dtype=np.int64)
        big_q = torch.zeros(1 << 22, dtype=torch.int32, device="cuda")  # 16 MiB: an allocation of its own

        def call(ctx=h, rank=0, m=m, queries=qp, kt=0, flags=0, mode=LOWER, out=op):
            torch.cuda.synchronize()
            return lib.lsb_search(ctx, rank, m, queries, kt, flags, mode, out)

        def untouched():
            torch.cuda.synchronize()
            return (bool((out == SENT).all()) and bool((both == SENT).all()) and bool(np.all(host_out == SENT))
                    and np.array_equal(host(qt).view(np.uint64), q) and np.array_equal(host_q, q))

        refusals = [
            ("null context", lambda: call(ctx=None)),
            ("rank 1 of 1", lambda: call(rank=1)),
            ("rank -1", lambda: call(rank=-1)),
            ("m < 0", lambda: call(m=-1)),
            ("key type 6", lambda: call(kt=6)),
            ("key type -1", lambda: call(kt=-1)),
            ("flags 2", lambda: call(flags=2)),
            ("mode 3", lambda: call(mode=3)),
            ("mode 3 with ADD", lambda: call(mode=7)),
            ("mode 8", lambda: call(mode=8)),
            ("mode -1", lambda: call(mode=-1)),
            ("null queries", lambda: call(queries=None)),
            ("null out", lambda: call(out=None)),
            ("host queries", lambda: call(queries=host_q.ctypes.data)),
            ("host out", lambda: call(out=host_out.ctypes.data)),
            ("8-byte queries off by 4 bytes", lambda: call(queries=qp + 4, m=m - 1)),
            ("4-byte queries off by 2 bytes", lambda: call(queries=qp + 2, kt=3)),
            ("out off by 4 bytes", lambda: call(out=op + 4)),
            ("queries leave their allocation", lambda: call(m=1 << 40)),
            ("out leaves its allocation", lambda: call(m=1 << 22, queries=big_q.data_ptr(), kt=3)),
            ("out is the query column", lambda: call(queries=bp, out=bp)),
            ("out starts on the last query", lambda: call(queries=bp, out=bp + 8 * (m - 1))),
            ("the queries start on the last result", lambda: call(queries=bp + 8 * (m - 1), out=bp)),
            ("4-byte queries that end inside out's first element", lambda: call(queries=bp + 8 * m - 4 * m + 4, kt=3,
                                                                                out=bp + 8 * m)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
        for bad in (lambda: w.search(0, qt, out[:m], side="middle"), lambda: w.search(0, qt, out),
                    lambda: w.search(0, qt, out[:m].to(torch.int32)), lambda: w.search(0, qt.cpu(), out[:m]),
                    lambda: w.search(0, qt, out[:m].cpu())):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(L.LsbError) as e:
            w.search(1, qt, out[:m])
        assert e.value.code == INVALID and untouched()
        # m == 0: nothing is looked at, nothing is written
        assert call(m=0) == OK and call(m=0, queries=None, out=None) == OK and call(m=0, mode=COUNT | ADD) == OK
        assert untouched()
        # columns that touch but share no byte are fine: queries in front of out, and behind it
        want = model(keys, q)
        both[:m] = qt
        assert call(queries=bp, out=bp + 8 * m, mode=UPPER) == OK
        assert np.array_equal(host(both[m:]), want["right"]) and np.array_equal(host(both[:m]).view(np.uint64), q)
        both[m:] = qt
        assert call(queries=bp + 8 * m, out=bp, mode=COUNT) == OK
        assert np.array_equal(host(both[:m]), want["count"]) and np.array_equal(host(both[m:]).view(np.uint64), q)
        # and after the refusals the call works, inside its m elements
        assert call() == OK
        got = host(out)
        assert np.array_equal(got[:m], want["left"]) and np.all(got[m:] == SENT)


# ------------------------------------------------- 9. unsorted records stay in bounds
@torch_first
def test_unsorted_records_stay_in_bounds(lsb_built):
    """The caller's error, not detected: the counts are unspecified, but every
    one lies in [0, n], nothing outside the output is written and the call
    succeeds.  The probe indices are bounded by how the ranges are built."""
    import torch
    L = lsb_built
    n, m, pad = 3 * TILE + 5, 5000, 64
    rng = np.random.default_rng(9)
    q = np.concatenate([rng.integers(0, 1 << 63, m - 4).astype(np.uint64) * np.uint64(2),
                        np.array([0, U64_MAX, 1, 1 << 63], dtype=np.uint64)])
    qt = column(q)
    shapes = {"random": rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2),
              "descending": np.sort(rng.integers(0, 1 << 63, n).astype(np.uint64))[::-1].copy(),
              "sorted tiles in the wrong order": np.sort(rng.integers(0, 1 << 63, n).astype(np.uint64))[
                  np.concatenate([np.arange(2 * TILE, n), np.arange(0, 2 * TILE)])].copy()}
    with L.World(n, ranks=1) as w:
        for name, keys in shapes.items():
            w.copy_in(0, records(keys))
            assert not w.check_sorted()
            for side in SIDES:
                for add in (False, True):
                    full = torch.full((m + 2 * pad,), SENT, dtype=torch.int64, device="cuda")
                    full[pad:pad + m] = 0
                    w.search(0, qt, full[pad:pad + m], side=side, add=add, key_type=0)  # LSB_OK, or it raises
                    got = host(full)
                    assert np.all(got[:pad] == SENT) and np.all(got[pad + m:] == SENT), (name, side, add)
                    assert got[pad:pad + m].min() >= 0 and got[pad:pad + m].max() <= n, (name, side, add)


# ------------------------------------------------- 10. more tiles than staged fences
def search_top():
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_search.hip")).read()
    return int(re.search(r"kSearchTop = (\d+);", src).group(1))


def fence_levels(tiles, top):
    """(step, tops, fences of the last staged group, its staged one included)
    as k_search derives them from the rank's tiles."""
    step = -(-tiles // top)
    tops = -(-tiles // step)
    return step, tops, tiles - (tops - 1) * step


def sparse_keys(n, seed):
    """n sorted distinct keys = 1 mod 4, so key - 1 and key + 1 miss and
    nothing wraps: a running sum of random gaps, no sort."""
    assert n << 37 < 1 << 62
    gaps = np.random.default_rng(seed).integers(1, 1 << 37, n, dtype=np.int64)
    return np.cumsum(gaps).astype(np.uint64) * np.uint64(4) + np.uint64(1)


def staged_runs(n, step, tops):
    """[a, b) record ranges that one value each fills, placed against the
    staged fences s = a multiple of step (tiles [t0, t1] whole unless said):
    [s - 1, s + 1], equal fences across a staged one; from step 3 on
    [s + 1, s + step - 1], equal fences strictly between two staged ones;
    [s, s + 2 step], equal adjacent staged ones; [s, s + step - 1], one staged
    group exactly; a run that starts and ends inside tiles, over a group and
    more; the last staged group up to the rank's last record."""
    s = [step * (j * tops // 7) for j in range(1, 6)]

    def whole(t0, t1):
        return t0 * TILE, (t1 + 1) * TILE

    runs = [whole(s[0] - 1, s[0] + 1)]
    if step >= 3:
        runs.append(whole(s[1] + 1, s[1] + step - 1))
    runs += [whole(s[2], s[2] + 2 * step), whole(s[3], s[3] + step - 1),
             (s[4] * TILE - 100, (s[4] + step + 1) * TILE + 7), ((tops - 1) * step * TILE, n)]
    assert runs[0][0] > 0 and all(a < b for a, b in runs) and all(x[1] < y[0] for x, y in zip(runs, runs[1:]))
    return runs


def fence_layouts(n, step, tops, seed):
    """(name, sorted keys, whether a value fills more than a staged group)."""
    keys = sparse_keys(n, seed)
    yield "distinct sparse keys", keys, False
    keys = keys.copy()
    runs = staged_runs(n, step, tops)
    for a, b in runs:
        keys[a:b] = keys[a]
    yield "runs of whole tiles against the staged fences", keys, True
    keys = keys.copy()
    keys[0] = 0
    keys[runs[-1][0]:] = U64_MAX
    yield "the same with 0 and 2^64 - 1 at the ends", keys, True


def aimed_queries(keys, starts, seed):
    """For every tile (starts: its first record's index) its fence and the
    record in front of it, each with - 1 and + 1; the first and last key, 0
    and 2^64 - 1; 2000 keys with - 1 and + 1 and 1000 draws; shuffled."""
    one = np.uint64(1)
    rng = np.random.default_rng(seed)
    f = keys[starts]
    p = keys[starts[starts > 0] - 1]
    hits = keys[rng.integers(0, keys.size, 2000)]
    q = np.concatenate([f, f - one, f + one, p, p - one, p + one, hits, hits - one, hits + one,
                        rng.integers(0, 1 << 63, 1000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + one,
                        np.array([keys[0], keys[-1], 0, U64_MAX], dtype=np.uint64)])
    rng.shuffle(q)
    return q


# name -> (a, b, step, fences of the last staged group): a * kSearchTop + b tiles
FENCE_TILES = {"top": (1, 0, 1, 1),            # every LDS slot used, the second level still empty
               "top_plus_1": (1, 1, 2, 1),     # the smallest step > 1; the last group short, fend clamped to tiles
               "2top_plus_2": (2, 2, 3, 1),    # a second level of 2 fences: both branches of its loop
               "4top_plus_3": (4, 3, 5, 4)}    # a second level of 4 fences (3 in the last group): up to 3 probes
LAST_TILE = {"full": lambda tiles: tiles * TILE, "short": lambda tiles: tiles * TILE - 1234,
             "one_record": lambda tiles: (tiles - 1) * TILE + 1}


@pytest.mark.parametrize("last_tile", list(LAST_TILE))
@pytest.mark.parametrize("size", list(FENCE_TILES))
@torch_first
def test_two_level_fence_table(lsb_built, size, last_tile):
    """Ranks of kSearchTop tiles and more: from kSearchTop + 1 on only every
    step-th fence is staged and the fences between two staged ones are
    searched too.  The sizes are derived from the kernel's constant and the
    levels they reach are asserted, so another constant cannot turn this into
    a test of one level."""
    L = lsb_built
    top = search_top()
    a, b, want_step, want_last = FENCE_TILES[size]
    tiles = a * top + b
    step, tops, last = fence_levels(tiles, top)
    assert (step, last) == (want_step, want_last) and tops <= top
    assert tops == top if size == "top" else (step > 1 and last < step and (tops - 1) * step + last == tiles)
    n = LAST_TILE[last_tile](tiles)
    assert -(-n // TILE) == tiles
    starts = np.arange(tiles, dtype=np.int64) * TILE
    with L.World(n, ranks=1) as w:
        for name, keys, long_runs in fence_layouts(n, step, tops, tiles):
            q = aimed_queries(keys, starts, tiles + 1)
            want = model(keys, q)
            # the oracle: answers in every staged group that holds one (a group inside a run holds none), the
            # last included; with the runs, a value that fills more than a staged group
            ends = np.append(np.flatnonzero(keys[1:] != keys[:-1]) + 1, n)
            holds = np.unique((ends - 1) // TILE // step)
            ans = np.concatenate([want["left"], want["right"]])
            assert np.array_equal(np.unique((ans[ans > 0] - 1) // TILE // step), holds) and holds[-1] == tops - 1, name
            if long_runs:
                assert (want["right"] - want["left"]).max() > step * TILE, name
            else:
                assert np.array_equal(holds, np.arange(tops)), name
            w.copy_in(0, records(keys))
            check_one_rank(w, keys, q, (name, tiles, n))


@torch_first
def test_two_level_fence_table_loopback(lsb_built):
    """Two ranks of kSearchTop + 2 tiles each, the last one record short: each
    rank's own fence table has two levels, and the ranks' answers add up,
    also for a value that runs over the rank boundary."""
    L = lsb_built
    top = search_top()
    P, per = 2, (top + 1) * TILE + 37
    n = P * per - 1
    tiles = -(-per // TILE)
    assert -(-(per - 1) // TILE) == tiles  # the last rank's too
    step, tops, last = fence_levels(tiles, top)
    assert step == 2 and tops <= top and (tops - 1) * step + last == tiles
    starts = np.concatenate([r * per + np.arange(tiles, dtype=np.int64) * TILE for r in range(P)])
    sparse = sparse_keys(n, 11)
    runs = sparse.copy()
    over = (per - 3 * TILE - 100, per + (2 * step + 1) * TILE + 500)  # over the boundary, whole staged groups of both
    spans = (staged_runs(per, step, tops)[:-1] + [over] +  # the first rank's last group belongs to `over`
             [(per + x, per + y) for x, y in staged_runs(per - 1, step, tops)])
    assert all(x[1] < y[0] for x, y in zip(spans, spans[1:])) and spans[-1][1] == n
    for x, y in spans:
        runs[x:y] = runs[x]
    with L.World(n, ranks=P) as w:
        assert w.per == per and w.here(P - 1) == per - 1
        for name, keys in (("distinct sparse keys", sparse), ("runs, one over the rank boundary", runs)):
            q = np.append(aimed_queries(keys, starts, 12), keys[per])
            qt = column(q)
            want = model(keys, q)
            w.scatter_global(records(keys))
            for side in SIDES:
                assert np.array_equal(search_all_ranks(w, qt, side), want[side]), (name, side)
        assert want["left"][-1] == over[0] < per < over[1] == want["right"][-1]  # the oracle sees the run on both ranks
        assert min(per - over[0], over[1] - per) > step * TILE


# ------------------------------------------------- 11. every key form at the kernel
def form_bits(name):
    """Distinct raw bit patterns of the type, zero-extended: 600 draws over
    every byte, the integers' minimum, -1, 0, 1 and maximum, the floats' two
    zeros, two infinities, NaNs of both signs with two payloads each (a quiet
    and a signalling one), the smallest subnormals and the largest finite
    values of both signs."""
    kt, dt = KEYS[name]
    width = 8 * np.dtype(dt).itemsize
    mask, sign = (1 << width) - 1, 1 << (width - 1)
    draws = np.random.default_rng(200 + kt).integers(0, 256, (600, 8), dtype=np.uint8).view(np.uint64).ravel()
    if name in ("f32", "f64"):
        inf, quiet = (0x7f800000, 0x00400000) if width == 32 else (0x7ff0000000000000, 0x0008000000000000)
        special = [0, sign, inf, sign | inf, inf | quiet | 1, inf | 2, sign | inf | quiet | 1, sign | inf | 2,
                   1, sign | 1, inf - 1, sign | (inf - 1)]
    else:
        special = [sign, mask, 0, 1, sign - 1, sign + 1, mask - 1]
    return np.unique(np.concatenate([draws & np.uint64(mask), np.array(special, dtype=np.uint64)]))


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("name", list(KEYS))
@torch_first
def test_every_key_form(lsb_built, name, descending):
    """k_search encodes the queries on the device from (key type, flags): all
    12 forms against records whose keys are the model's encoding of typed
    values, the specials of every type among them."""
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    n = 3 * TILE + 5
    wide = np.dtype(dt).itemsize == 8
    mask = U64_MAX if wide else np.uint64(0xFFFFFFFF)
    one = np.uint64(1)
    rng = np.random.default_rng(210 + kt)
    pool = form_bits(name)
    bits = np.concatenate([pool, rng.choice(pool, n - pool.size)])  # every value, with ties
    keys = np.sort(model_encode(bits, kt, descending))
    qbits = np.concatenate([pool, (pool + one) & mask, (pool - one) & mask,
                            rng.integers(0, 256, (600, 8), dtype=np.uint8).view(np.uint64).ravel() & mask])
    rng.shuffle(qbits)
    want = model(keys, model_encode(qbits, kt, descending))
    assert want["count"].max() > 1 and (want["count"] == 0).sum() > 100  # hits with ties, and misses
    # the model's order is the type's: the values that compare, by value; NaNs at both ends, by sign
    typed = bits.astype(np.uint64 if wide else np.uint32).view(dt)[np.argsort(model_encode(bits, kt, descending))]
    if name in ("f32", "f64"):
        assert np.isnan(typed[0]) and np.isnan(typed[-1]) and np.signbit(typed[0]) != descending
        typed = typed[~np.isnan(typed)]
    assert np.all(typed[1:] <= typed[:-1] if descending else typed[1:] >= typed[:-1])
    assert typed[0] != typed[-1]
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)  # uint columns travel as tensors of the same width
    dq = torch.from_numpy(qbits.astype(np.uint64 if wide else np.uint32).view(key_np).copy()).cuda()
    columns = [("", dq)]
    if not wide:  # a column that starts 4 bytes into its allocation
        room = torch.zeros(dq.numel() + 1, dtype=dq.dtype, device="cuda")
        room[1:] = dq
        columns.append(("4 bytes into its allocation", room[1:]))
        assert room[1:].data_ptr() % 8 == 4
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        for what, col in columns:
            assert np.array_equal(bits_of(host(col)), qbits)
            for side in SIDES:
                got = search(w, 0, col, side, key_type=kt, descending=descending)
                assert np.array_equal(got, want[side]), (name, descending, side, what)


# ------------------------------------------------- 12. COUNT's gallop at its ends
@torch_first
def test_count_gallop_ends(lsb_built):
    """Runs of 2^j - 1, 2^j and 2^j + 1 records, j = 0..13, where the gallop's
    last step and the binary search behind it end: inside the rank, on the
    rank's last record, and from a tile's last record on."""
    import torch
    L = lsb_built
    n = 3 * TILE + 5
    lengths = sorted({r for j in range(14) for r in ((1 << j) - 1, 1 << j, (1 << j) + 1) if r > 0})
    assert lengths[-1] == (1 << 13) + 1 and TILE - 1 + lengths[-1] <= n
    base = np.arange(n, dtype=np.uint64) * np.uint64(8) + np.uint64(5)
    one = np.uint64(1)
    rng = np.random.default_rng(12)
    with L.World(n, ranks=1) as w:
        for r in lengths:
            for what, a in (("inside the rank", 1001), ("up to the rank's last record", n - r),
                            ("from a tile's last record", TILE - 1)):
                keys = base.copy()
                keys[a:a + r] = keys[a]
                v = keys[a]
                q = np.concatenate([np.array([v, v - one, v + one, keys[a - 1], keys[min(a + r, n - 1)], keys[0],
                                              keys[-1], 0, U64_MAX], dtype=np.uint64), keys[::97], keys[::89] + one])
                qt = column(q)
                want = model(keys, q)["count"]
                assert want[0] == r and want[1] == 0 and want[2] == 0
                start = rng.integers(-(1 << 40), 1 << 40, q.size).astype(np.int64)
                w.copy_in(0, records(keys))
                assert np.array_equal(search(w, 0, qt, "count"), want), (r, what)
                got = search(w, 0, qt, "count", add=True, out=torch.from_numpy(start.copy()).cuda())
                assert np.array_equal(got, start + want), (r, what, "ADD")
