"""The matches of a column of queries in the sorted records, on the device:
the first match's value per query (lsb_lookup, lsbsort.lookup) and the matched
pairs (lsb_join_count + lsb_store_join, lsbsort.join); include/lsb.h "the
matches themselves", DESIGN.md §7.8.

The oracle is numpy.searchsorted over the mapped keys on the host: lower and
count per query, then the pairs by numpy.repeat.  Everything is integer and is
compared exactly and in order.  Records are loaded with copy_in, sorted on the
host, so no test depends on the sort.

The columns are torch CUDA tensors, so (as tests/test_search_gpu.py) the tests
run in one child pytest process over this same file that imports torch before
the library is loaded (LSB_JOIN_CHILD=1), once per session; here each test
reports what its namesake did there.
"""
import ctypes
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

IN_CHILD = os.environ.get("LSB_JOIN_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096   # records per fence, and queries per tile sum
OK, INVALID, STATE = 0, 1, 7
SENT = 0x5555555555555555
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
ELEM = np.dtype([("key", "<u8"), ("val", "<u8")])
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("join") / "child.xml"
    env = dict(os.environ, LSB_JOIN_CHILD="1")
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


def source_constant(name):
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_search.hip")).read()
    return int(re.search(r"%s = (\d+);" % name, src).group(1))


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
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def host(t):
    return t.cpu().numpy()


def value_of(index):
    """A record's value from its global index: both words depend on it, and
    neither is the index."""
    i = np.asarray(index).astype(np.uint64)
    return i * np.uint64(0x0000000300000007) + np.uint64(0x0000000900000005)


def records(keys, base=0):
    rec = np.zeros(keys.size, dtype=ELEM)
    rec["key"] = keys
    rec["val"] = value_of(np.arange(base, base + keys.size))
    return rec


def model(sorted_keys, queries):
    """Per query lower and count; per pair the query and the record, ordered
    by query, then by record."""
    sorted_keys = np.ascontiguousarray(sorted_keys, dtype=np.uint64)
    queries = np.ascontiguousarray(queries, dtype=np.uint64)
    lo = np.searchsorted(sorted_keys, queries, "left").astype(np.int64)
    c = np.searchsorted(sorted_keys, queries, "right").astype(np.int64) - lo
    off = np.cumsum(c) - c
    left = np.repeat(np.arange(queries.size, dtype=np.int64), c)
    p = np.repeat(lo, c) + np.arange(int(c.sum()), dtype=np.int64) - np.repeat(off, c)
    return {"lower": lo, "count": c, "off": off, "total": int(c.sum()), "left": left, "p": p}


def column(q):
    """uint64 queries as the int64 CUDA tensor that carries their bits."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, dtype=np.uint64).view(np.int64).copy()).cuda()


def sentinels(n, dtype=None):
    import torch
    dtype = dtype or torch.int64
    return torch.full((n,), SENT if dtype == torch.int64 else 0x55555555, dtype=dtype, device="cuda")


PAD = 64


def store(w, rank, total, outputs=("left", "right", "pos"), vb=8, query_base=0):
    """World.store_join into sentinel columns with PAD elements of room behind
    the pairs -> {name: numpy}, the room checked."""
    import torch
    cols = {name: sentinels(total + PAD, torch.int32 if name == "right" and vb == 4 else None) for name in outputs}
    assert w.store_join(rank, query_base=query_base, **cols) == total
    out = {}
    for name, t in cols.items():
        got = host(t)
        assert np.all(got[total:] == (0x55555555 if got.dtype == np.int32 else SENT)), (name, "written behind the pairs")
        out[name] = got[:total]
    return out


def check_pairs(got, want, gbase=0, vb=8, query_base=0, what=""):
    if "left" in got:
        assert np.array_equal(got["left"], want["left"] + query_base), (what, "left")
    if "pos" in got:
        assert np.array_equal(got["pos"], want["p"] + gbase), (what, "pos")
    if "right" in got:
        v = value_of(want["p"] + gbase)
        if vb == 4:
            assert np.array_equal(got["right"].view(np.uint32), (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (what, "right")
        else:
            assert np.array_equal(got["right"].view(np.uint64), v), (what, "right")


def check_join(w, sorted_keys, q, what, rank=0, gbase=0):
    """Count (with counts_dev), then store all three outputs: against the model."""
    want = model(sorted_keys, q)
    qt = column(q)
    counts = sentinels(q.size)
    total = w.join_count(rank, qt, counts, key_type=0)
    assert total == want["total"], (what, total, want["total"])
    assert np.array_equal(host(counts), want["count"]), (what, "counts")
    assert np.array_equal(host(qt).view(np.uint64), q), (what, "the queries changed")
    if total:
        check_pairs(store(w, rank, total), want, gbase=gbase, what=what)
    return want


def short_run_keys(n, seed):
    """Sorted keys = 1 mod 4 (key - 1 and key + 1 miss) with short runs."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, 1 << 60, n, dtype=np.int64).astype(np.uint64) * np.uint64(4) + np.uint64(1)
    for at in rng.integers(0, n, max(1, n // 50)):
        keys[at:at + int(rng.integers(2, 40))] = keys[at]
    return np.sort(keys)


def query_pool(sorted_keys, seed):
    d = np.unique(sorted_keys)
    rest = np.concatenate([d, d - np.uint64(1), d + np.uint64(1)])
    np.random.default_rng(seed).shuffle(rest)
    return np.concatenate([np.array([sorted_keys[0], sorted_keys[-1], 0, U64_MAX], dtype=np.uint64), rest])


def odd_keys(n):
    """n distinct sorted keys 1, 3, 5, ...: every even number misses."""
    return np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)


# ------------------------------------------------- 1. tiles of queries, sweeps of the scan
def query_sizes():
    sweep = source_constant("kJoinScanSweep")
    return [1, TILE - 1, TILE, TILE + 1, sweep * TILE + 1]


@pytest.mark.parametrize("m", query_sizes())
@torch_first
def test_query_tiles(lsb_built, m):
    """m around the 4096-query tile, and one m with more tiles than the scan
    workgroup takes in one sweep, so that the carry between sweeps counts."""
    L = lsb_built
    sweep = source_constant("kJoinScanSweep")
    if m > 2 * TILE:
        assert -(-m // TILE) == sweep + 1 > sweep
    n = 3 * TILE + 5
    keys = short_run_keys(n, 101)
    pool = query_pool(keys, m)
    q = np.resize(pool, m)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        want = check_join(w, keys, q, ("m", m))
        if m > 2 * TILE:  # pairs in the second sweep's tiles, and in front of them
            assert want["count"][sweep * TILE:].sum() > 0 and want["off"][sweep * TILE] > 0
            assert want["count"].max() > 1 and (want["count"] == 0).sum() > m // 4


# ------------------------------------------------- 2. tiles of outputs
@pytest.mark.parametrize("delta", [-1, 0, 1, None], ids=["T-1", "T", "T+1", "none"])
@torch_first
def test_output_tiles(lsb_built, delta):
    """Totals of T - 1, T and T + 1 pairs; and no pair at all: nothing is
    launched and the outputs stay as they were."""
    import torch
    L = lsb_built
    T = source_constant("kJoinTile")
    n = T + 10
    keys = odd_keys(n)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        if delta is None:
            q = np.arange(0, 2 * n, 2, dtype=np.uint64)  # every query misses
            want = check_join(w, keys, q, "no pair")
            assert want["total"] == 0
            cols = [sentinels(8) for _ in range(3)]
            assert w.store_join(0, left=cols[0], right=cols[1], pos=cols[2]) == 0
            assert all(bool((c == SENT).all()) for c in cols)
            # the pointers are not examined: host memory, unaligned, overlapping
            bad = np.zeros(4, dtype=np.int64)
            cnt = np.zeros(1, dtype=np.int64)
            torch.cuda.synchronize()
            assert L._lib().lsb_store_join(w._h, 0, 0, 0, bad.ctypes.data + 1, bad.ctypes.data + 1, 8, None,
                                           cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == OK
            return
        total = T + delta
        q = np.empty(2 * total, dtype=np.uint64)  # a hit and a miss in turn
        q[0::2] = keys[:total]
        q[1::2] = keys[:total] + np.uint64(1)
        want = check_join(w, keys, q, ("total", total))
        assert want["total"] == total


# ------------------------------------------------- 3. a run longer than the output tiles
@pytest.mark.parametrize("start", ["a tile's last slot", "slot 5", "slot 0"])
@torch_first
def test_long_run(lsb_built, start):
    """One query whose run is 3 T + 5 records: its pairs span four or five
    output tiles, each of which stages the one offset."""
    L = lsb_built
    T = source_constant("kJoinTile")
    run = 3 * T + 5
    before = {"a tile's last slot": T - 1, "slot 5": 5, "slot 0": 0}[start]
    head = 2 * T
    keys = np.concatenate([odd_keys(head), np.full(run, 2 * head + 1, dtype=np.uint64),
                           odd_keys(head + 40)[head + 1:]])
    n = keys.size
    q = np.concatenate([keys[:before], [np.uint64(2 * head + 1)], keys[-7:], [np.uint64(0)], keys[3:5]])
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        want = check_join(w, keys, q, start)
    assert want["count"][before] == run and want["off"][before] == before and want["lower"][before] == head
    assert want["total"] == before + run + 7 + 2


# ------------------------------------------------- 4. spans of queries longer than the staged offsets
def span_cases():
    S = source_constant("kJoinSpan")
    return [("S", S), ("S+1", S + 1), ("more", S + 1003)]


@pytest.mark.parametrize("name,span", span_cases())
@torch_first
def test_span_of_missing_queries(lsb_built, name, span):
    """Matching queries, then missing ones, then matching ones, all inside one
    output tile: the tile's span of queries is exactly S entries (staged),
    S + 1 and more (searched in global memory)."""
    L = lsb_built
    T, S = source_constant("kJoinTile"), source_constant("kJoinSpan")
    n = TILE + 9
    keys = odd_keys(n)
    keys[100:104] = keys[100]  # a run of 4
    lead, a, b = 17, 3, 2
    misses = span - a - b
    q = np.concatenate([np.arange(0, 2 * lead, 2, dtype=np.uint64),           # misses in front of the first match
                        [keys[100], keys[7], keys[7]],                        # a matches
                        np.arange(0, 2 * misses, 2, dtype=np.uint64) % np.uint64(2 * n),
                        [keys[n - 1], keys[100]],                             # b matches
                        np.arange(0, 20, 2, dtype=np.uint64)])                # misses behind the last
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        want = check_join(w, keys, q, name)
    hits = np.flatnonzero(want["count"])
    assert hits[-1] - hits[0] + 1 == span and want["total"] == 4 + 1 + 1 + 1 + 4 < T
    assert (span <= S) == (name == "S") and misses > (S if name == "more" else 0)


# ------------------------------------------------- 5. many queries on one key
@torch_first
def test_many_queries_on_one_key(lsb_built):
    L = lsb_built
    n = TILE + 100
    keys = odd_keys(n)
    keys[3000:3100] = keys[3000]
    q = np.full(1000, keys[3000], dtype=np.uint64)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        want = check_join(w, keys, q, "1000 x 100")
    assert want["total"] == 100_000 and np.all(want["count"] == 100)
    assert np.array_equal(want["p"][:200], np.tile(np.arange(3000, 3100), 2))


# ------------------------------------------------- 6. totals beyond 32 bits
@torch_first
def test_total_beyond_32_bits(lsb_built):
    """2^16 equal records and 2^16 queries of that key: 2^32 pairs, counted
    and never stored."""
    import torch
    L = lsb_built
    n = m = 1 << 16
    keys = np.full(n, 77, dtype=np.uint64)
    qt = column(np.full(m, 77, dtype=np.uint64))
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        counts = sentinels(m)
        assert w.join_count(0, qt, counts, key_type=0) == 1 << 32
        assert bool((counts == n).all())
        small = sentinels(16)
        cnt = ctypes.c_int64(-1)
        torch.cuda.synchronize()
        assert L._lib().lsb_store_join(w._h, 0, 16, 0, small.data_ptr(), None, 0, None, ctypes.byref(cnt)) == INVALID
        assert cnt.value == 1 << 32 and bool((small == SENT).all())


# ------------------------------------------------- 7. the outputs
@torch_first
def test_outputs(lsb_built):
    """Every subset of (left, right, pos), values of 8 and 4 bytes, a query
    base, and a second store from the same plan."""
    L = lsb_built
    T = source_constant("kJoinTile")
    n = 2 * TILE + 77
    keys = short_run_keys(n, 7)
    q = np.resize(query_pool(keys, 7), 3 * T + 11)
    want = model(keys, q)
    assert want["total"] > T + 1
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        assert w.join_count(0, column(q), key_type=0) == want["total"]
        first = None
        for k in (1, 2, 3):
            for outputs in itertools.combinations(("left", "right", "pos"), k):
                for vb in ((8, 4) if "right" in outputs else (8,)):
                    for base in (0, 1 << 40, -5):
                        got = store(w, 0, want["total"], outputs, vb=vb, query_base=base)
                        check_pairs(got, want, vb=vb, query_base=base, what=(outputs, vb, base))
                        if outputs == ("left", "right", "pos") and vb == 8 and base == 0:
                            first = got
        again = store(w, 0, want["total"])
        assert all(np.array_equal(again[k], first[k]) for k in first)


# ------------------------------------------------- 8. cap below the total
@torch_first
def test_cap_below_total(lsb_built):
    import torch
    L = lsb_built
    n = TILE + 3
    keys = short_run_keys(n, 8)
    q = np.resize(query_pool(keys, 8), 900)
    want = model(keys, q)
    total = want["total"]
    assert total > 100
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        assert w.join_count(0, column(q), key_type=0) == total
        cols = [sentinels(total) for _ in range(3)]
        cnt = ctypes.c_int64(-1)
        torch.cuda.synchronize()
        assert L._lib().lsb_store_join(w._h, 0, total - 1, 0, cols[0].data_ptr(), cols[1].data_ptr(), 8,
                                       cols[2].data_ptr(), ctypes.byref(cnt)) == INVALID
        torch.cuda.synchronize()
        assert cnt.value == total and all(bool((c == SENT).all()) for c in cols)
        with pytest.raises(L.LsbError) as e:
            w.store_join(0, left=cols[0][:total - 1])
        assert e.value.code == INVALID
        check_pairs(store(w, 0, total), want, what="the plan survives the refusal")


# ------------------------------------------------- 9. the plan's lifetime
@torch_first
def test_plan_lifetime(lsb_built):
    L = lsb_built
    n = 3 * TILE + 5
    keys = short_run_keys(n, 9)
    other = np.sort(np.random.default_rng(90).integers(1 << 61, 1 << 62, n).astype(np.uint64))
    q = np.resize(query_pool(keys, 9), 700)
    qt = column(q)
    want = model(keys, q)
    assert want["total"] > 0

    def no_plan(w, what, rank=0):
        with pytest.raises(L.LsbError) as e:
            w.store_join(rank, left=sentinels(want["total"] + 1))
        assert e.value.code == STATE, what

    def plan(w):
        w.copy_in(0, records(keys))
        assert w.join_count(0, qt, key_type=0) == want["total"]
        check_pairs(store(w, 0, want["total"]), want, what="a fresh plan")

    with L.World(n, ranks=1) as w:
        no_plan(w, "before any count")
        enders = {
            "generate": lambda: w.generate(),
            "generate(zipf)": lambda: w.generate("zipf"),
            "copy_in": lambda: w.copy_in(0, records(other)),
            "load_columns": lambda: w.load_columns(0, column(other), key_type=0),
            "my_sort": lambda: w.my_sort(),
            "global_shuffle": lambda: w.global_shuffle(0),
            "label_runs": lambda: (w.count_runs(), w.label_runs(L.LABEL_KEEP)),
            "scan_runs": lambda: (w.count_runs(), w.plan_scan(L.SCAN_SUM, L.KEY_U64), w.scan_runs(L.LABEL_KEEP)),
        }
        for name, end in enders.items():
            plan(w)
            end()
            no_plan(w, "after " + name)
        # the calls that leave A alone keep the plan: lsb_select, the reads, a search
        plan(w)
        assert w.select(n // 2)["key"] == int(keys[n // 2])
        w.copy_out(0)
        assert w.check_sorted()
        w.count_runs()
        w.search(0, qt, sentinels(q.size), side="count", key_type=0)
        lone = sentinels(q.size)
        w.lookup(0, qt, lone, key_type=0)
        check_pairs(store(w, 0, want["total"]), want, what="after select and the reads")
        # a count with more queries regrows the scratch; a smaller one after it fits
        big = np.resize(query_pool(keys, 10), 5 * TILE + 3)
        check_join(w, keys, big, "regrown")
        check_join(w, keys, q[:50], "smaller again")
        # a refused count leaves the plan it found
        with pytest.raises(L.LsbError):
            w.join_count(0, qt, qt, key_type=0)  # the counts would overwrite the queries
        check_pairs(store(w, 0, model(keys, q[:50])["total"]), model(keys, q[:50]), what="after a refused count")
    # plans are per rank
    P, per = 2, TILE + 37
    n2 = 2 * per - 1
    keys2 = short_run_keys(n2, 11)
    with L.World(n2, ranks=P) as w:
        w.scatter_global(records(keys2))
        pool2 = query_pool(keys2, 11)
        q0, q1 = np.resize(pool2, 600), np.resize(pool2[::-1], 2 * TILE + 1)
        w0, w1 = model(keys2[:per], q0), model(keys2[per:], q1)
        assert w.join_count(0, column(q0), key_type=0) == w0["total"] > 0
        no_plan(w, "rank 1 has none yet", rank=1)
        assert w.join_count(1, column(q1), key_type=0) == w1["total"] > 0
        check_pairs(store(w, 0, w0["total"]), w0, what="rank 0's plan after rank 1 counted")
        check_pairs(store(w, 1, w1["total"]), w1, gbase=per, what="rank 1's plan")


# ------------------------------------------------- 10. loopback ranks
def join_all_ranks(w, q):
    """The union of the ranks' pairs (left, pos, right), in rank order."""
    qt = column(q)
    parts = []
    for r in range(w.P):
        total = w.join_count(r, qt, key_type=0)
        if total:
            parts.append(store(w, r, total))
        else:
            assert w.store_join(r, left=sentinels(1)) == 0
    return {k: np.concatenate([p[k] for p in parts]) for k in ("left", "right", "pos")}


@torch_first
def test_two_loopback_ranks(lsb_built):
    L = lsb_built
    P, per = 2, TILE + 37
    n = P * per - 1
    keys = short_run_keys(n, 12)
    keys[per - 600:per + 900] = keys[per - 600]  # a run across the rank boundary
    keys = np.sort(keys)
    q = np.concatenate([query_pool(keys, 12)[:900], [keys[per]] * 3])
    want = model(keys, q)
    assert want["lower"][-1] < per < want["lower"][-1] + want["count"][-1]
    with L.World(n, ranks=P) as w:
        assert w.per == per
        w.scatter_global(records(keys))
        got = join_all_ranks(w, q)
        order = np.lexsort((got["pos"], got["left"]))
        assert np.array_equal(got["left"][order], want["left"]) and np.array_equal(got["pos"][order], want["p"])
        assert np.array_equal(got["right"][order].view(np.uint64), value_of(want["p"]))
        # each rank alone, in its own order, with global positions
        for r in range(P):
            part = model(keys[r * per:(r + 1) * per], q)
            check_join(w, keys[r * per:(r + 1) * per], q, ("rank", r), rank=r, gbase=r * per)
            assert part["total"] > 0
        # lookup: last to first leaves the global first match, first to last the last rank's
        qt = column(q)
        down, up = sentinels(q.size), sentinels(q.size)
        for r in (1, 0):
            w.lookup(r, qt, down, key_type=0)
        for r in (0, 1):
            w.lookup(r, qt, up, key_type=0)
        hit = want["count"] > 0
        assert np.array_equal(host(down).view(np.uint64)[hit], value_of(want["lower"][hit]))
        assert np.all(host(down)[~hit] == SENT) and np.all(host(up)[~hit] == SENT)
        last_rank_first = np.where(want["lower"] + want["count"] > per, np.maximum(want["lower"], per), want["lower"])
        assert np.array_equal(host(up).view(np.uint64)[hit], value_of(last_rank_first[hit]))
        assert not np.array_equal(host(up), host(down))  # the run across the boundary tells them apart


@torch_first
def test_three_ranks_one_empty(lsb_built):
    import torch
    L = lsb_built
    keys = np.array([3, 3, 5, 9], dtype=np.uint64)  # per = 2: rank 2 holds nothing
    q = np.array([3, 4, 5, 9, 3, 0, 9] * 20, dtype=np.uint64)
    want = model(keys, q)
    with L.World(4, ranks=3) as w:
        assert w.per == 2 and w.here(2) == 0
        w.scatter_global(records(keys))
        qt = column(q)
        counts = sentinels(q.size)
        assert w.join_count(2, qt, counts, key_type=0) == 0 and not bool(counts.any())
        assert w.store_join(2, left=sentinels(4)) == 0
        vals, found = sentinels(q.size), torch.full((q.size,), 0x55, dtype=torch.uint8, device="cuda")
        w.lookup(2, qt, vals, found, key_type=0)
        assert bool((vals == SENT).all()) and bool((found == 0x55).all())
        got = join_all_ranks(w, q)
        order = np.lexsort((got["pos"], got["left"]))
        assert np.array_equal(got["left"][order], want["left"]) and np.array_equal(got["pos"][order], want["p"])
        assert np.array_equal(got["right"][order].view(np.uint64), value_of(want["p"]))


# ------------------------------------------------- 11. lookup
@torch_first
def test_lookup(lsb_built):
    """Hits, misses and repeated queries; the first record of runs of 2 and of
    4097 records; values of 8 and 4 bytes; either output alone."""
    import torch
    L = lsb_built
    n = 3 * TILE + 5
    keys = odd_keys(n)
    keys[10:12] = keys[10]
    keys[TILE - 3:TILE - 3 + 4097] = keys[TILE - 3]
    rng = np.random.default_rng(13)
    q = np.concatenate([keys[rng.integers(0, n, 3000)], keys[rng.integers(0, n, 2000)] + np.uint64(1),
                        [keys[10]] * 5, [keys[TILE - 3]] * 5, [0, U64_MAX, keys[0], keys[-1]]]).astype(np.uint64)
    rng.shuffle(q)
    want = model(keys, q)
    hit = want["count"] > 0
    assert set(want["count"]) >= {0, 1, 2, 4097} and hit.sum() > 3000 and (~hit).sum() > 1500
    qt = column(q)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        vals, found = sentinels(q.size), torch.full((q.size,), 0x55, dtype=torch.uint8, device="cuda")
        w.lookup(0, qt, vals, found, key_type=0)
        v, f = host(vals).view(np.uint64), host(found)
        assert np.array_equal(v[hit], value_of(want["lower"][hit])) and np.all(v[~hit] == np.uint64(SENT))
        assert np.all(f[hit] == 1) and np.all(f[~hit] == 0x55)
        v4 = sentinels(q.size, torch.int32)
        w.lookup(0, qt, v4, key_type=0)
        g = host(v4).view(np.uint32)
        assert np.array_equal(g[hit], (value_of(want["lower"][hit]) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        assert np.all(g[~hit] == 0x55555555)
        only = torch.zeros(q.size, dtype=torch.bool, device="cuda")
        w.lookup(0, qt, found=only, key_type=0)
        assert np.array_equal(host(only), hit)
        assert np.array_equal(host(qt).view(np.uint64), q)
        # m == 0
        w.lookup(0, qt[:0], vals[:0], key_type=0)
        assert np.array_equal(host(vals).view(np.uint64), v)


# ------------------------------------------------- 12. every key form at the kernels
def form_bits(name):
    kt, dt = KEYS[name]
    width = 8 * np.dtype(dt).itemsize
    mask, sign = (1 << width) - 1, 1 << (width - 1)
    draws = np.random.default_rng(300 + kt).integers(0, 256, (600, 8), dtype=np.uint8).view(np.uint64).ravel()
    if name in ("f32", "f64"):
        inf, quiet = (0x7f800000, 0x00400000) if width == 32 else (0x7ff0000000000000, 0x0008000000000000)
        special = [0, sign, inf, sign | inf, inf | quiet | 1, inf | 2, sign | inf | quiet | 1, sign | inf | 2,
                   1, sign | 1, inf - 1, sign | (inf - 1)]
    else:
        special = [sign, mask, 0, 1, sign - 1, sign + 1, mask - 1]
    return np.unique(np.concatenate([draws & np.uint64(mask), np.array(special, dtype=np.uint64)])), special


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("name", list(KEYS))
@torch_first
def test_every_key_form(lsb_built, name, descending):
    """k_lookup and k_join_count encode the queries on the device from (key
    type, flags): all 12 forms, the types' extremes and the floats' zeros,
    infinities and NaNs (both signs, two payloads) among keys and queries."""
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    n = 2 * TILE + 5
    wide = np.dtype(dt).itemsize == 8
    mask = U64_MAX if wide else np.uint64(0xFFFFFFFF)
    one = np.uint64(1)
    rng = np.random.default_rng(310 + kt)
    pool, special = form_bits(name)
    special = np.array(special, dtype=np.uint64)
    bits = np.concatenate([pool, rng.choice(pool, n - pool.size)])
    keys = np.sort(model_encode(bits, kt, descending))
    qbits = np.concatenate([special, pool, (pool + one) & mask, (pool - one) & mask])
    rng.shuffle(qbits[special.size:])
    want = model(keys, model_encode(qbits, kt, descending))
    hit = want["count"] > 0
    assert want["count"].max() > 1 and (~hit).sum() > 100 and np.all(hit[:special.size])
    if name in ("f32", "f64"):  # the two zeros and the NaN payloads are keys of their own
        b = list(special)
        for x, y in ((0, 1), (4, 5), (6, 7)):
            assert want["lower"][x] != want["lower"][y], (hex(int(b[x])), hex(int(b[y])))
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)
    dq = torch.from_numpy(qbits.astype(np.uint64 if wide else np.uint32).view(key_np).copy()).cuda()
    kw = dict(key_type=kt, descending=descending)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(keys))
        vals, found = sentinels(dq.numel()), torch.zeros(dq.numel(), dtype=torch.uint8, device="cuda")
        w.lookup(0, dq, vals, found, **kw)
        v = host(vals).view(np.uint64)
        assert np.array_equal(host(found) == 1, hit), (name, descending)
        assert np.array_equal(v[hit], value_of(want["lower"][hit])) and np.all(v[~hit] == np.uint64(SENT))
        counts = sentinels(dq.numel())
        assert w.join_count(0, dq, counts, **kw) == want["total"]
        assert np.array_equal(host(counts), want["count"]), (name, descending)
        check_pairs(store(w, 0, want["total"]), want, what=(name, descending))
    assert np.array_equal(bits_of(host(dq)), qbits)


# ------------------------------------------------- 13. refusals that need a device
@torch_first
def test_refusals(lsb_built):
    import torch
    L = lsb_built
    ct = ctypes
    lib = L._lib()
    n, m = TILE + 3, 300
    keys = short_run_keys(n, 14)
    q = np.resize(query_pool(keys, 14), m)
    want = model(keys, q)
    total = want["total"]
    assert total > 50
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, records(keys))
        qt = column(q)
        assert w.join_count(0, qt, key_type=0) == total
        cap = total + 8
        v, c, le, ri, po = (sentinels(cap + m) for _ in range(5))
        f = torch.full((m + 8,), 0x55, dtype=torch.uint8, device="cuda")
        both = sentinels(2 * (cap + m))
        bp = both.data_ptr()
        host_col = np.full(cap + m, SENT, dtype=np.int64)
        hp = host_col.ctypes.data
        big = torch.zeros(1 << 22, dtype=torch.int32, device="cuda")  # 16 MiB: an allocation of its own
        bigp, bigm = big.data_ptr(), 1 << 22
        qp = qt.data_ptr()
        cnt = ct.c_int64(-1)

        def lookup(ctx=h, rank=0, m=m, queries=qp, kt=0, flags=0, vals=v.data_ptr(), vb=8, found=f.data_ptr()):
            torch.cuda.synchronize()
            return lib.lsb_lookup(ctx, rank, m, queries, kt, flags, vals, vb, found)

        def count(ctx=h, rank=0, m=m, queries=qp, kt=0, flags=0, counts=c.data_ptr()):
            torch.cuda.synchronize()
            return lib.lsb_join_count(ctx, rank, m, queries, kt, flags, counts, ct.byref(cnt))

        def stor(ctx=h, rank=0, cap=cap, base=0, left=le.data_ptr(), right=ri.data_ptr(), vb=8, pos=po.data_ptr()):
            torch.cuda.synchronize()
            return lib.lsb_store_join(ctx, rank, cap, base, left, right, vb, pos, None)

        def untouched():
            torch.cuda.synchronize()
            return (all(bool((t == SENT).all()) for t in (v, c, le, ri, po, both)) and bool((f == 0x55).all())
                    and bool(np.all(host_col == SENT)) and np.array_equal(host(qt).view(np.uint64), q))

        refusals = [
            ("lookup: null context", lambda: lookup(ctx=None)),
            ("lookup: rank 1 of 1", lambda: lookup(rank=1)),
            ("lookup: m < 0", lambda: lookup(m=-1)),
            ("lookup: key type 6", lambda: lookup(kt=6)),
            ("lookup: flags 2", lambda: lookup(flags=2)),
            ("lookup: val_bytes 2", lambda: lookup(vb=2)),
            ("lookup: val_bytes 16", lambda: lookup(vb=16)),
            ("lookup: values without val_bytes", lambda: lookup(vb=0)),
            ("lookup: val_bytes without values", lambda: lookup(vals=None)),
            ("lookup: no output", lambda: lookup(vals=None, vb=0, found=None)),
            ("lookup: null queries", lambda: lookup(queries=None)),
            ("lookup: host queries", lambda: lookup(queries=hp)),
            ("lookup: host values", lambda: lookup(vals=hp)),
            ("lookup: host found", lambda: lookup(found=hp)),
            ("lookup: queries off by 4 bytes", lambda: lookup(queries=qp + 4, m=m - 1)),
            ("lookup: 8-byte values off by 4 bytes", lambda: lookup(vals=v.data_ptr() + 4)),
            ("lookup: 4-byte values off by 2 bytes", lambda: lookup(vals=v.data_ptr() + 2, vb=4)),
            ("lookup: values leave their allocation", lambda: lookup(m=bigm, queries=bigp, kt=3)),
            ("lookup: queries leave their allocation", lambda: lookup(m=1 << 40)),
            ("lookup: values are the queries", lambda: lookup(queries=bp, vals=bp)),
            ("lookup: values start on the last query", lambda: lookup(queries=bp, vals=bp + 8 * (m - 1))),
            ("lookup: found inside the values", lambda: lookup(vals=bp, found=bp + 8 * m - 1)),
            ("lookup: found inside the queries", lambda: lookup(queries=bp, vals=bp + 8 * m, found=bp + 5)),
            ("count: null context", lambda: count(ctx=None)),
            ("count: rank -1", lambda: count(rank=-1)),
            ("count: m < 0", lambda: count(m=-1)),
            ("count: key type -1", lambda: count(kt=-1)),
            ("count: flags 4", lambda: count(flags=4)),
            ("count: null queries", lambda: count(queries=None)),
            ("count: host queries", lambda: count(queries=hp)),
            ("count: host counts", lambda: count(counts=hp)),
            ("count: counts off by 4 bytes", lambda: count(counts=c.data_ptr() + 4)),
            ("count: 4-byte queries off by 2 bytes", lambda: count(queries=qp + 2, kt=3)),
            ("count: counts leave their allocation", lambda: count(m=bigm, queries=bigp, kt=3)),
            ("count: counts are the queries", lambda: count(queries=bp, counts=bp)),
            ("count: the queries start on the last count", lambda: count(queries=bp + 8 * (m - 1), counts=bp)),
            ("store: null context", lambda: stor(ctx=None)),
            ("store: rank 1 of 1", lambda: stor(rank=1)),
            ("store: cap < 0", lambda: stor(cap=-1)),
            ("store: val_bytes 3", lambda: stor(vb=3)),
            ("store: right without val_bytes", lambda: stor(vb=0)),
            ("store: val_bytes without right", lambda: stor(right=None)),
            ("store: no output", lambda: stor(left=None, right=None, vb=0, pos=None)),
            ("store: host left", lambda: stor(left=hp)),
            ("store: host right", lambda: stor(right=hp)),
            ("store: host pos", lambda: stor(pos=hp)),
            ("store: left off by 4 bytes", lambda: stor(left=le.data_ptr() + 4)),
            ("store: 4-byte right off by 2 bytes", lambda: stor(right=ri.data_ptr() + 2, vb=4)),
            ("store: pos leaves its allocation", lambda: stor(cap=bigm, left=None, right=bigp, vb=4)),
            ("store: left is right", lambda: stor(left=bp, right=bp)),
            ("store: pos starts on left's last element", lambda: stor(left=bp, pos=bp + 8 * (cap - 1))),
            ("store: 4-byte right ends inside pos", lambda: stor(right=bp + 8 * cap - 4 * cap + 4, vb=4, pos=bp + 8 * cap)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
        # the refused counts left the plan alone; columns that touch without sharing a byte are fine
        assert stor(left=bp, right=bp + 8 * cap, pos=None) == OK
        got = host(both)
        assert np.array_equal(got[:total], want["left"]) and np.all(got[total:cap] == SENT)
        assert np.array_equal(got[cap:cap + total].view(np.uint64), value_of(want["p"]))
        both.fill_(SENT)
        # m == 0: nothing is looked at, nothing is written, and the plan is one of no pairs
        assert lookup(m=0) == OK and lookup(m=0, queries=None) == OK and untouched()
        assert count(m=0, queries=None, counts=None) == OK and cnt.value == 0 and untouched()
        assert stor() == OK and untouched()
        for bad in (lambda: w.lookup(0, qt), lambda: w.lookup(0, qt, v[:m - 1]), lambda: w.lookup(0, qt.cpu(), v[:m]),
                    lambda: w.lookup(0, qt, v[:m], found=v[:m]), lambda: w.join_count(0, qt, c[:m].to(torch.int32)),
                    lambda: w.join_count(0, qt, c[:m + 1]), lambda: w.store_join(0),
                    lambda: w.store_join(0, left=le.to(torch.int32)), lambda: w.store_join(0, pos=po.cpu())):
            with pytest.raises(ValueError):
                bad()


# ------------------------------------------------- 14. the front ends
def front_end_oracle(left, right):
    """(left index, right index) of every pair of equal keys, by left index,
    then by right index; and the left indices without a match."""
    order = np.argsort(right, kind="stable")
    want = model(right[order], left)
    return want["left"], order[want["p"]].astype(np.int64), np.flatnonzero(want["count"] == 0)


@pytest.mark.parametrize("ranks", [1, 3])
@torch_first
def test_join_front_end(lsb_built, ranks):
    import torch
    L = lsb_built
    rng = np.random.default_rng(15)
    n, m = 10_000, 3_000
    right = rng.integers(-2000, 2000, n).astype(np.int64)
    left = rng.integers(-3000, 3000, m).astype(np.int64)
    li, ri, lone = front_end_oracle(model_encode(left.view(np.uint64), 1, False), model_encode(right.view(np.uint64), 1, False))
    assert li.size > m and lone.size > 100
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    gl, gr = L.join(dl, dr, ranks=ranks)
    assert gl.dtype == gr.dtype == torch.int64 and gl.device == dl.device
    gl, gr = host(gl), host(gr)
    if ranks > 1:
        order = np.lexsort((gr, gl))
        gl, gr = gl[order], gr[order]
    assert np.array_equal(gl, li) and np.array_equal(gr, ri)
    assert np.array_equal(left[gl], right[gr])
    # how="left": the matched pairs, then the left keys without a match, in left order
    hl, hr = (host(t) for t in L.join(dl, dr, how="left", ranks=ranks))
    assert np.array_equal(hl[li.size:], lone) and np.all(hr[li.size:] == -1) and hl.size == li.size + lone.size
    head = np.lexsort((hr[:li.size], hl[:li.size])) if ranks > 1 else np.arange(li.size)
    assert np.array_equal(hl[:li.size][head], li) and np.array_equal(hr[:li.size][head], ri)
    # descending, and keys that are sorted already
    sr = np.sort(right)[::-1].copy()
    sl, srr, _ = front_end_oracle(model_encode(left.view(np.uint64), 1, True), model_encode(sr.view(np.uint64), 1, True))
    al, ar = (host(t) for t in L.join(dl, torch.from_numpy(sr).cuda(), descending=True, assume_sorted=True, ranks=ranks))
    order = np.lexsort((ar, al))
    assert np.array_equal(al[order], sl) and np.array_equal(ar[order], srr)
    # empty sides
    for a, b in ((dl[:0], dr), (dl, dr[:0]), (dl[:0], dr[:0])):
        el, er = L.join(a, b, ranks=ranks)
        assert el.numel() == 0 and er.numel() == 0 and el.dtype == er.dtype == torch.int64
        el, er = L.join(a, b, how="left", ranks=ranks)
        assert np.array_equal(host(el), np.arange(a.numel())) and bool((er == -1).all())
    assert np.array_equal(host(dl), left) and np.array_equal(host(dr), right)
    with pytest.raises(ValueError, match="how"):
        L.join(dl, dr, how="outer")
    with pytest.raises(ValueError):
        L.join(dl.to(torch.int32), dr)
    with pytest.raises(ValueError):
        L.join(dl.cpu(), dr)


@torch_first
def test_join_front_end_floats(lsb_built):
    """float32 with NaNs and both zeros: pairs are equal bits, not equal values."""
    import torch
    L = lsb_built
    rng = np.random.default_rng(16)
    specials = np.array([0x00000000, 0x80000000, 0x7fc00001, 0xffc00001, 0x7f800002, 0x7f800000, 0xff800000], dtype=np.uint32)
    right = np.concatenate([rng.integers(1, 50, 500).astype(np.float32).view(np.uint32), np.repeat(specials, 3)])
    left = np.concatenate([rng.integers(1, 80, 200).astype(np.float32).view(np.uint32), specials,
                           np.array([0x7fc00002, 0xffc00002], dtype=np.uint32)])
    rng.shuffle(right)
    rng.shuffle(left)
    li, ri, lone = front_end_oracle(model_encode(left.astype(np.uint64), 5, False), model_encode(right.astype(np.uint64), 5, False))
    dl = torch.from_numpy(left.view(np.float32).copy()).cuda()
    dr = torch.from_numpy(right.view(np.float32).copy()).cuda()
    gl, gr = (host(t) for t in L.join(dl, dr))
    assert np.array_equal(gl, li) and np.array_equal(gr, ri)
    assert np.array_equal(left[gl], right[gr])  # bit for bit
    for s in specials:  # each special of the left side pairs with its three bit-equal records only
        at = int(np.flatnonzero(left == s)[0])
        assert (gl == at).sum() == 3, hex(int(s))
    for s in (0x7fc00002, 0xffc00002):
        assert int(np.flatnonzero(left == np.uint32(s))[0]) in lone


@pytest.mark.parametrize("ranks", [1, 3])
@torch_first
def test_lookup_front_end(lsb_built, ranks):
    import torch
    L = lsb_built
    rng = np.random.default_rng(17)
    n, m = 10_000, 3_000
    keys = rng.integers(-2000, 2000, n).astype(np.int64)
    vals = rng.integers(-1 << 30, 1 << 30, n).astype(np.int32)
    q = rng.integers(-3000, 3000, m).astype(np.int64)
    ek, eq = model_encode(keys.view(np.uint64), 1, False), model_encode(q.view(np.uint64), 1, False)
    order = np.argsort(ek, kind="stable")
    want = model(ek[order], eq)
    hit = want["count"] > 0
    first = order[np.minimum(want["lower"], n - 1)]  # the lowest input index of the key
    assert hit.sum() > 1000 and (~hit).sum() > 500 and want["count"].max() > 2
    dk, dv, dq = torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda(), torch.from_numpy(q).cuda()
    out, found = L.lookup(dk, dv, dq, default=-7, ranks=ranks)
    assert out.dtype == torch.int32 and found.dtype == torch.bool and out.shape == found.shape == dq.shape
    assert np.array_equal(host(found), hit)
    assert np.array_equal(host(out), np.where(hit, vals[first], -7))
    idx, found = L.lookup(dk, None, dq, default=-1, ranks=ranks)
    assert idx.dtype == torch.int64 and np.array_equal(host(found), hit)
    assert np.array_equal(host(idx), np.where(hit, first, -1))
    out, found = L.lookup(dk, dv, dq, ranks=ranks)
    assert np.array_equal(host(out), np.where(hit, vals[first], 0))
    # no keys, no queries
    out, found = L.lookup(dk[:0], dv[:0], dq, default=3, ranks=ranks)
    assert bool((out == 3).all()) and not bool(found.any()) and out.shape == dq.shape
    out, found = L.lookup(dk, dv, dq[:0], ranks=ranks)
    assert out.numel() == 0 and found.numel() == 0 and found.dtype == torch.bool
    for bad in (lambda: L.lookup(dk, dv[:5], dq), lambda: L.lookup(dk, dv, dq.to(torch.int32)),
                lambda: L.lookup(dk, dv.cpu(), dq), lambda: L.lookup(dk, dv, dq, ranks=0)):
        with pytest.raises(ValueError):
            bad()
