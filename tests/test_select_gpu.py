"""The k-th key and the first k + 1 records on the device, without a sort
(lsb_select / lsb_store_select, lsbsort.kth / lsbsort.topk; include/lsb.h "the
k-th key and the first k + 1 records").

The oracle is numpy on the host: the stable argsort of the mapped keys, the
mapping written out below from the header's table (tests/test_runs_gpu.py's
model).  Records are loaded with copy_in, their value the global index, so a
rank's part of the selection, in slot order, is a sorted list of indices.
What every round reads, and who compacts, is tests/select_model.py's rule of
the rounds (held against the same argsort in tests/test_select_host.py):
last_select() must equal it exactly.

The outputs are torch CUDA tensors, so (as tests/test_runs_gpu.py) the tests
run in one child pytest process over this same file that imports torch before
the library is loaded (LSB_SELECT_CHILD=1), once per session; here each test
reports what its namesake did there.  The tests with real rank processes start
their own processes and run from the pytest process itself.
"""
import ctypes
import functools
import inspect
import multiprocessing
import os
import re
import socket
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import select_model as M

IN_CHILD = os.environ.get("LSB_SELECT_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
INVALID, STATE = 1, 7
SENT = 0x5555555555555555
ELEM = np.dtype([("key", "<u8"), ("val", "<u8")])
# name -> (LSB_KEY_*, numpy dtype)
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("select") / "child.xml"
    env = dict(os.environ, LSB_SELECT_CHILD="1")
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


class Oracle:
    """The stable sort of the mapped keys, once per key set."""

    def __init__(self, keys):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.order = np.argsort(self.keys, kind="stable")
        self.sorted = self.keys[self.order]

    def at(self, k):
        """-> (pivot, below, equal) of position k."""
        pivot = self.sorted[k]
        lo = int(np.searchsorted(self.sorted, pivot, "left"))
        hi = int(np.searchsorted(self.sorted, pivot, "right"))
        return int(pivot), lo, hi - lo

    def selection(self, k):
        """The input indices of the first k + 1 records, ascending: the ranks'
        parts in slot order, laid end to end."""
        return np.sort(self.order[:k + 1])

    def per_rank(self, k, P):
        """-> (below[P], equal[P]) of the block partition."""
        n = self.keys.size
        per = -(-n // P)
        pivot = self.sorted[k]
        rank_of = np.arange(n) // per
        return (np.bincount(rank_of[self.keys < pivot], minlength=P)[:P].astype(np.int64),
                np.bincount(rank_of[self.keys == pivot], minlength=P)[:P].astype(np.int64))

    def tie_edges(self):
        """Both edges, as positions of the sort, of every group of two or
        more equal keys (at most 8 groups, spread over the order)."""
        heads = np.flatnonzero(np.concatenate([[True], self.sorted[1:] != self.sorted[:-1]]))
        tails = np.concatenate([heads[1:], [self.sorted.size]]) - 1
        ties = np.flatnonzero(tails > heads)
        if ties.size > 8:
            ties = ties[np.linspace(0, ties.size - 1, 8).astype(np.int64)]
        return sorted(set(heads[ties].tolist()) | set(tails[ties].tolist()))


def store(w, rank, m, outputs=("keys", "values"), val_bytes=8, key_type=0, key_np=np.int64, descending=False,
          shift=2):
    """store_select of `rank` into fresh columns of m elements, each with
    `shift` sentinel elements in front and two behind that must survive
    (shift = 1: columns aligned to their element only) -> {name: numpy}."""
    import torch
    dts = {"keys": key_np, "values": np.int64 if val_bytes == 8 else np.int32}
    sent = {k: np.frombuffer(b"\x55" * ((m + shift + 2) * np.dtype(dts[k]).itemsize), dtype=dts[k]).copy()
            for k in outputs}
    full = {k: torch.from_numpy(v.copy()).cuda() for k, v in sent.items()}
    got = w.store_select(rank, **{k: full[k][shift:shift + m] for k in outputs}, key_type=key_type,
                         descending=descending)
    assert got == m
    out = {}
    for k, t in full.items():
        h = host(t)
        assert np.array_equal(bits_of(h[:shift]), bits_of(sent[k][:shift])), k
        assert np.array_equal(bits_of(h[shift + m:]), bits_of(sent[k][shift + m:])), k
        out[k] = h[shift:shift + m]
    return out


def check_select(w, orc, k, what):
    """select(k) against the oracle -> the plan."""
    pivot, below, equal = orc.at(k)
    plan = w.select(k)
    assert (plan["key"], plan["below"], plan["equal"]) == (pivot, below, equal), (what, k)
    P = len(plan["take"])
    want = w_plan(orc, k, P)
    assert plan["take"] == want["take"] and plan["bases"] == want["bases"], (what, k)
    return plan


def w_plan(orc, k, P):
    import lsbsort
    b, e = orc.per_rank(k, P)
    got = lsbsort.plan_select(orc.keys.size, P, k + 1, b, e)
    return {"take": [int(x) for x in got["take"]], "bases": [int(x) for x in got["bases"]]}


def check_rounds(w, keys, k, what):
    """The rounds and the records read of the select just run are the model's."""
    m = M.round_model(keys, w.P, k)
    assert w.last_select() == (m.rounds, sum(m.read)), (what, k, m.rounds, m.read)
    return m


def check_store(w, orc, k, plan, what, **kw):
    """Every rank's store_select, laid end to end, is the selection in index
    order; the keys are those records' keys."""
    parts = [store(w, r, plan["take"][r], **kw) for r in range(len(plan["take"]))]
    want = orc.selection(k)
    for name in parts[0]:
        glob = np.concatenate([p[name] for p in parts])
        if name == "values":
            w_ = want.astype(np.uint64) & np.uint64(0xFFFFFFFF if glob.dtype.itemsize == 4 else ~np.uint64(0))
        else:
            w_ = orc.keys[want]
        assert np.array_equal(bits_of(glob), w_), (what, k, name)


# ------------------------------------------------- 1. tile edges, one rank
def key_patterns(n, seed=5):
    rng = np.random.default_rng(seed + n)
    distinct = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    heavy = distinct.copy()
    heavy[rng.random(n) < 0.6] = np.uint64(0x7A00_0000_0000_1234)   # one top-byte bucket over half: no compaction
    heavy[rng.random(n) < 0.1] = np.uint64(0x7A00_0000_0000_1235)
    heavy[rng.random(n) < 0.05] = np.uint64(0x0300_0000_0000_0000)
    return {
        "distinct": distinct,
        "one value": np.full(n, 0xC0FFEE, dtype=np.uint64),
        "two values in byte 0": np.where(rng.random(n) < 0.5, np.uint64(0x1122334455667701), np.uint64(0x11223344556677F0)),
        "byte 7 only": rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56) | np.uint64(0x00AB_CDEF_0123_4567),
        "heavy among distinct": heavy,
        "below 2^32": rng.integers(0, 1 << 32, n, dtype=np.int64).astype(np.uint64),
    }


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@torch_first
def test_tile_edges_one_rank(lsb_built, n):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        for name, keys in key_patterns(n).items():
            rec = records(keys)
            orc = Oracle(keys)
            w.copy_in(0, rec)
            ks = sorted({0, n - 1, n // 2} | set(orc.tie_edges()))
            for k in ks:
                plan = check_select(w, orc, k, name)
                assert plan["take"] == [k + 1] and plan["bases"] == [0]
                if k in (0, n - 1, n // 2) or k == ks[len(ks) // 2]:
                    check_store(w, orc, k, plan, name)
            k = ks[len(ks) // 2]
            plan = check_select(w, orc, k, name)
            check_store(w, orc, k, plan, (name, "4-byte values"), val_bytes=4)
            check_store(w, orc, k, plan, (name, "element-aligned columns"), shift=1)
            check_store(w, orc, k, plan, (name, "keys alone"), outputs=("keys",))
            check_store(w, orc, k, plan, (name, "values alone"), outputs=("values",))
            check_store(w, orc, k, plan, (name, "32-bit keys"), key_type=3, key_np=np.int32) if name == "below 2^32" \
                else None
            # every A is bit for bit what it was
            assert np.array_equal(w.copy_out(0), rec), name


# ------------------------------------------------- 2. rounds and reads
@torch_first
def test_rounds_and_reads(lsb_built):
    L = lsb_built
    n = 64 * TILE
    rng = np.random.default_rng(2024)
    u64 = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + (rng.integers(0, 2, n).astype(np.uint64))
    u32 = rng.integers(0, 1 << 32, n, dtype=np.int64).astype(np.uint64)
    k = n // 2
    with L.World(n, ranks=1) as w:
        def run(keys):
            orc = Oracle(keys)
            w.copy_in(0, records(keys))
            check_select(w, orc, k, "rounds")
            check_rounds(w, keys, k, "rounds")
            return w.last_select()

        assert run(np.full(n, 77, dtype=np.uint64)) == (1, n)
        assert run(np.where(rng.random(n) < 0.5, np.uint64(0xAA00), np.uint64(0xAA01))) == (2, 2 * n)
        # the n / 16 is a condition on the input, checked here, not a measurement
        top = u64 >> np.uint64(56)
        assert np.count_nonzero(top == np.sort(u64)[k] >> np.uint64(56)) < n // 16
        rounds, read = run(u64)
        print("u64: rounds", rounds, "records_read", read, "bound", 2 * n + n // 16)
        assert read <= 2 * n + n // 16
        byte3 = u32 >> np.uint64(24)
        assert np.count_nonzero(byte3 == np.sort(u32)[k] >> np.uint64(24)) < n // 16
        rounds, read = run(u32)
        print("u32: rounds", rounds, "records_read", read, "bound", 3 * n + n // 16)
        assert rounds <= 5 and read <= 3 * n + n // 16


# ------------------------------------------------- 3. more tiles than workgroups
def grid_cap():
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_select.hip")).read()
    return (int(re.search(r"kSelGridCap = (\d+);", src).group(1)),
            int(re.search(r"kSelScanBlock = (\d+);", src).group(1)))


@torch_first
def test_more_tiles_than_workgroups(lsb_built):
    """The first two workgroups of k_sel_hist (with the span, with the
    compaction and plain), of k_sel_count and of k_sel_write take a second
    tile, and every thread of k_sel_scan several: n = (grid cap) tiles + one
    tile + 1.  (Two tiles for every workgroup: test_dense_two_tiles_each.)"""
    L = lsb_built
    cap, scan_block = grid_cap()
    n = cap * TILE + TILE + 1
    assert n // TILE > cap and n // TILE > scan_block
    rng = np.random.default_rng(99)
    k = n // 2 + 17
    with L.World(n, ranks=1) as w:
        # round one with the span, round two with the compaction, both over all of A
        keys = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64)
        keys[rng.random(n) < 0.001] = np.sort(keys)[k]  # a pivot group spread over the tiles
        orc = Oracle(keys)
        w.copy_in(0, records(keys))
        plan = check_select(w, orc, k, "u64")
        rounds, read = w.last_select()
        assert 2 * n < read < 2 * n + n // 16
        check_rounds(w, keys, k, "u64")
        check_store(w, orc, k, plan, "u64")
        # keys below 2^32: round two reads all of A without a compaction
        keys = rng.integers(0, 1 << 32, n, dtype=np.int64).astype(np.uint64)
        orc = Oracle(keys)
        w.copy_in(0, records(keys))
        check_select(w, orc, k, "below 2^32")
        rounds, read = w.last_select()
        assert rounds <= 5 and 3 * n < read < 3 * n + n // 16
        check_rounds(w, keys, k, "below 2^32")
        # three top-byte values: a third of the records match, and the waves of the two workgroups that
        # take a second tile flush inside the loop
        keys = M.top3_keys(n)
        orc = Oracle(keys)
        w.copy_in(0, records(keys))
        for k3 in M.dense_ks(n):
            plan = check_select(w, orc, k3, "top3")
            check_rounds(w, keys, k3, "top3")
            if k3 < k:  # the smallest of the three only: a store's outputs and its check grow with k
                check_store(w, orc, k3, plan, "top3")


# ------------------------------------------------- 4. loopback ranks
def rank_cases(P):
    """(name, mapped keys, ks): per = 4099 (odd: ranks 1.. hold blocks aligned
    to their element only), n = P * per - 1."""
    per = 4099
    n = P * per - 1
    rng = np.random.default_rng(40 + P)
    base = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(np.uint64)
    pivot = np.uint64(1 << 61)  # about the median of the others
    cases = []
    astride = base.copy()
    astride[per - 3:per + 4] = pivot                  # the pivot group lies across the first boundary
    cases.append(("astride", astride))
    if P >= 3:
        middle = base.copy()
        middle[per - 5:2 * per + 7] = pivot           # ... and over the whole of rank 1
        cases.append(("whole middle rank", middle))
    few = rng.integers(0, 3, n).astype(np.uint64) << np.uint64(40)  # three values: every rank holds part of the group
    cases.append(("three values", few))
    out = []
    for name, keys in cases:
        orc = Oracle(keys)
        lo = int(np.searchsorted(orc.sorted, pivot if name != "three values" else np.uint64(1 << 40), "left"))
        hi = int(np.searchsorted(orc.sorted, pivot if name != "three values" else np.uint64(1 << 40), "right")) - 1
        out.append((name, orc, sorted({0, n - 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi})))
    return out


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_loopback_ranks(lsb_built, P):
    L = lsb_built
    for name, orc, ks in rank_cases(P):
        n = orc.keys.size
        rec = records(orc.keys)
        with L.World(n, ranks=P) as w:
            w.scatter_global(rec)
            for k in ks:
                plan = check_select(w, orc, k, name)
                assert sum(plan["take"]) == k + 1
                check_store(w, orc, k, plan, name)
                if name == "whole middle rank" and k == ks[3]:
                    b, e = orc.per_rank(k, P)
                    assert e[1] == w.per and 0 < plan["take"][1] - b[1] < w.per  # cut inside the middle rank
            check_store(w, orc, ks[-1], plan, (name, "element-aligned, 4-byte"), shift=1, val_bytes=4)
            assert np.array_equal(w.gather_global(), rec), name
    # trailing empty ranks
    n = 6 if P == 5 else P - 1
    keys = np.array([3, 1, 3, 3, 0, 3][:n], dtype=np.uint64)
    orc = Oracle(keys)
    with L.World(n, ranks=P) as w:
        assert w.here(P - 1) == 0
        w.scatter_global(records(keys))
        for k in range(n):
            plan = check_select(w, orc, k, "empty ranks")
            assert plan["take"][P - 1] == 0
            check_store(w, orc, k, plan, "empty ranks")


# ------------------------------------------------- 5. typed keys through the front ends
N = 100_003


@functools.lru_cache(maxsize=None)
def typed_keys(name, n=N):
    """n keys of at most 2^12 distinct values spread over every byte of the
    type, negative ones included; f32 without NaN and -0.0; f64 with both
    zeros, both infinities and NaNs of both signs."""
    kt, dt = KEYS[name]
    v = np.random.default_rng(20 + kt).integers(0, 4096, n).astype(np.int64)
    if name == "i64":
        a = (v - 2048) * np.int64(0x0002_0008_0200_0801)
    elif name == "u32":
        a = (v * 0x00100401 % (1 << 32)).astype(np.uint32)
    elif name == "u64":  # v >= 2048: bit 63 set
        a = v.astype(np.uint64) * np.uint64(0x0010_0400_8020_0401)
        assert np.any(a >> np.uint64(63) == 1) and np.any(a >> np.uint64(63) == 0)
    elif name == "i32":
        a = ((v - 2048) * 0x00080401).astype(np.int32)
        assert a.min() < 0 < a.max()
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


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("name,descending", [("i64", False), ("f32", True), ("u32", False), ("f64", False),
                                             ("u64", False), ("i32", True)])
@torch_first
def test_typed_front_ends(lsb_built, name, descending, ranks):
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    keys = typed_keys(name)
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)  # uint columns travel as tensors of the same width
    dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
    key_type = kt if name in ("u64", "u32") else None
    bits = bits_of(keys)
    for desc in (descending, not descending):
        orc = Oracle(model_encode(bits, kt, desc))
        for k in (0, N // 3, N - 1) + tuple(orc.tie_edges()[2:4]):
            value, below, equal = L.kth(dk, k, descending=desc, ranks=ranks, key_type=key_type)
            assert value.dtype == dk.dtype and value.device == dk.device and value.numel() == 1
            _, lo, cnt = orc.at(k)
            assert int(bits_of(host(value))[0]) == int(bits[orc.order[k]]) and (below, equal) == (lo, cnt), (desc, k)
    if name == "f64":  # the specials sit where the header's order puts them
        asc = Oracle(model_encode(bits, kt, False))
        first, last = bits[asc.order[0]], bits[asc.order[-1]]
        assert first == 0xfff8000000000002 and last == 0x7ff8000000000001
    for largest in (True, False):
        orc = Oracle(model_encode(bits, kt, largest))
        for k in (1, 1000, 4099):
            idx = orc.order[:k]
            values, indices = L.topk(dk, k, largest=largest, ranks=ranks, key_type=key_type)
            assert values.dtype == dk.dtype and indices.dtype == torch.int64 and values.device == dk.device
            assert np.array_equal(host(indices), idx), (largest, k)
            assert np.array_equal(bits_of(host(values)), bits[idx]), (largest, k)
            values, indices = L.topk(dk, k, largest=largest, sorted=False, ranks=ranks, key_type=key_type)
            assert np.array_equal(host(indices), np.sort(idx)), (largest, k, "unsorted")
            assert np.array_equal(bits_of(host(values)), bits[np.sort(idx)]), (largest, k, "unsorted")
            if name in ("i64", "f32", "i32"):  # NaN-free: torch's values are the same
                tv = torch.topk(torch.from_numpy(keys.copy()), k, largest=largest, sorted=True).values
                assert np.array_equal(bits_of(host(L.topk(dk, k, largest=largest, ranks=ranks)[0])), bits_of(tv.numpy()))
    assert np.array_equal(bits_of(host(dk)), bits)  # the input is untouched
    v, i = L.topk(dk, 0, ranks=ranks, key_type=key_type)
    assert v.numel() == 0 and i.numel() == 0 and v.dtype == dk.dtype and i.dtype == torch.int64
    v, i = L.topk(dk[:0], 0, ranks=ranks, key_type=key_type)
    assert v.numel() == 0 and i.numel() == 0
    v, i = L.topk(dk, N, ranks=ranks, key_type=key_type)  # everything: the stable descending argsort
    assert np.array_equal(host(i), Oracle(model_encode(bits, kt, True)).order)
    for bad in (lambda: L.topk(dk, N + 1, key_type=key_type), lambda: L.topk(dk, -1, key_type=key_type),
                lambda: L.kth(dk, N, key_type=key_type), lambda: L.kth(dk, -1, key_type=key_type),
                lambda: L.kth(dk[:0], 0, key_type=key_type),
                lambda: L.kth(torch.zeros((4, 4), dtype=torch.float32, device="cuda"), 0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------- 6. state and refusals
@torch_first
def test_state_and_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = (1 << 18) + 77
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(30)
    orc = Oracle(keys)
    rec = records(keys)
    k = n // 3
    m = k + 1
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, rec)
        cols = {c: torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda") for c in "kv"}
        kp, vp = (cols[c].data_ptr() for c in "kv")
        small = torch.zeros(16, dtype=torch.int64, device="cuda")
        host_arr = np.full(m, SENT, dtype=np.uint64)
        torch.cuda.synchronize()
        count = ctypes.c_int64(-1)

        def call(cap=m, keys=kp, kt=0, flags=0, vals=vp, vb=8):
            count.value = -1
            return lib.lsb_store_select(h, 0, cap, keys, kt, flags, vals, vb, ctypes.byref(count))

        def untouched():
            torch.cuda.synchronize()
            return all(bool((t == SENT).all()) for t in cols.values()) and bool(np.all(host_arr == SENT))

        # no plan yet, and none after anything that can change A
        assert call() == STATE and untouched()
        changes = [("my_sort", w.my_sort), ("copy_in", lambda: w.copy_in(0, rec[:5], off=3)),
                   ("load_columns", lambda: w.load_columns(0, small, key_type=0)), ("generate", w.generate),
                   ("global_shuffle", lambda: w.global_shuffle(0)),
                   ("label_runs", lambda: (w.count_runs(), w.label_runs(L.LABEL_KEEP)))]
        for what, change in changes:
            w.select(5)
            change()
            assert call() == STATE and untouched(), what
            with pytest.raises(L.LsbError) as e:
                w.store_select(0, values=cols["v"])
            assert e.value.code == STATE, what
        # k out of range: refused, and an earlier plan stays
        w.copy_in(0, rec)
        check_select(w, orc, k, "state")
        key = ctypes.c_uint64(5)
        for bad_k in (-1, n, n + 1, 1 << 62):
            assert lib.lsb_select(h, bad_k, ctypes.byref(key), None, None, None, None) == INVALID and key.value == 5
        with L.World(0, ranks=2) as empty:
            assert lib.lsb_select(empty._h, 0, None, None, None, None, None) == INVALID
            assert empty.last_select() == (0, 0)
        refusals = [
            ("cap one short", lambda: call(cap=m - 1)),
            ("negative cap", lambda: call(cap=-1)),
            ("rank", lambda: lib.lsb_store_select(h, 1, m, kp, 0, 0, vp, 8, None)),
            ("no output", lambda: call(keys=None, vals=None, vb=0)),
            ("key type 6", lambda: call(kt=6)),
            ("flags 2", lambda: call(flags=2)),
            ("val_bytes 3", lambda: call(vb=3)),
            ("val_bytes 8, no values", lambda: call(vals=None)),
            ("val_bytes 0 with values", lambda: call(vb=0)),
            ("host keys", lambda: call(keys=host_arr.ctypes.data)),
            ("host values", lambda: call(vals=host_arr.ctypes.data)),
            ("keys off by 4 bytes", lambda: call(keys=kp + 4)),
            ("32-bit keys off by 2 bytes", lambda: call(keys=kp + 2, kt=4)),
            ("4-byte values off by 2 bytes", lambda: call(vals=vp + 2, vb=4)),
            ("keys leave their allocation", lambda: call(cap=1 << 40, vals=None, vb=0)),
            ("values leave their allocation", lambda: call(cap=1 << 40, keys=None)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
            if what == "cap one short":
                assert count.value == m
        with pytest.raises(ValueError):
            w.store_select(0)
        # the plan survived every refusal
        plan = {"take": [m], "bases": [0]}
        check_store(w, orc, k, plan, "after the refusals")
        # select leaves a run plan usable, and the run calls leave the select plan
        runs = w.count_runs()
        starts = torch.empty(runs["total"], dtype=torch.int64, device="cuda")
        check_select(w, orc, k + 9, "beside a run plan")
        assert w.store_runs(0, starts=starts) == runs["total"]
        w.plan_reduce(L.REDUCE_SUM, L.KEY_U64)
        out = torch.empty(runs["total"], dtype=torch.int64, device="cuda")
        assert w.store_reduce(0, out) == runs["total"]
        w.count_runs()
        check_store(w, orc, k + 9, {"take": [k + 10], "bases": [0]}, "after the run calls")
        assert np.array_equal(w.copy_out(0), rec)
        # and the context sorts and verifies afterwards
        w.generate()
        w.select(n // 2)
        w.my_sort()
        assert w.verify() == (True, -1)
        srt = w.copy_out(0)
        plan = w.select(n // 2)
        assert plan["key"] == int(srt["key"][n // 2]) and plan["take"] == [n // 2 + 1]
        assert np.array_equal(w.copy_out(0), srt)


# ------------------------------------------------- 7. the compaction
# The inputs of tests/select_model.py, whose conditions (which rounds compact,
# the fills at the flushes inside the tile loop) tests/test_select_host.py
# asserts.  A candidate the compaction loses, doubles or replaces moves the
# pivot of the ks beyond it, or the next round's counts no longer add up.
def run_compaction(L, keys, P, ks, what):
    """Every k of ks: the plan against the stable sort, the rounds and reads
    against the model; the store at the first, middle and last k; A bit for
    bit afterwards.  No LsbError: a STATE error from the compaction's own
    checks is a failure like a wrong answer."""
    rec = records(keys)
    orc = Oracle(keys)
    first, mid, last = ks[0], ks[len(ks) // 2], ks[-1]
    with L.World(keys.size, ranks=P) as w:
        w.scatter_global(rec)
        for k in ks:
            plan = check_select(w, orc, k, what)
            check_rounds(w, keys, k, what)
            if k in (first, mid, last):
                check_store(w, orc, k, plan, what)
            if k == mid:
                check_store(w, orc, k, plan, (what, "element-aligned, 4-byte"), shift=1, val_bytes=4)
        assert np.array_equal(w.gather_global(), rec), what


@pytest.mark.parametrize("layout", ["sorted", "shuffled", "one_over"])
@torch_first
def test_halving_chain(lsb_built, layout):
    """Eight rounds, each bucket half of its source: rounds two to eight
    compact at 2 cand == held, out of A and then out of B into B, until B
    holds n - n / 128 records.  sorted: tiles that match whole, every flush
    inside the loop of a full stage.  one_over: 2 cand == held + 2 in the first
    record's bucket, where round two must filter A again."""
    run_compaction(lsb_built, M.chain_keys(layout), 1, M.chain_ks(), layout)


@torch_first
def test_three_quarter_blocks(lsb_built):
    """Three tiles that match at 3/4 in a rank that matches under 1/2: flushes
    inside the loop with a stage filled to 449..511."""
    keys = M.blocks_keys()
    run_compaction(lsb_built, keys, 1, M.bucket_ks(keys, M.BLOCKS_TOP), "blocks")


@torch_first
def test_dense_two_tiles_each(lsb_built):
    """A third of the records match and every workgroup takes two tiles: nearly
    every wave flushes inside the loop, across the tile boundary, with a
    partial stage, and reserves twice."""
    n = M.dense_n()
    run_compaction(lsb_built, M.top3_keys(n), 1, M.dense_ks(n), "top3")


@torch_first
def test_mixed_ranks(lsb_built):
    """Ranks that decide differently in one round: one filters A, one
    compacts, one has no candidate and launches nothing."""
    keys = M.mixed_keys()
    run_compaction(lsb_built, keys, M.MIXED_P, M.mixed_ks(keys)[0], "mixed")


# ------------------------------------------------- 8. real processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_process(rank, world, transport, port, n, k, result_dir, q_uid, q_out):
    """One rank of a one-rank-per-process world: select, then store its part
    into its own torch tensors."""
    try:
        for p in (ROOT, os.path.join(ROOT, "distributed-lsb_amd")):
            sys.path.insert(0, p)
        if transport == "rccl":  # one "host" per rank: RCCL's socket transport between them
            os.environ["NCCL_HOSTID"] = f"lsb-rank-{rank}"
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
            os.environ.setdefault("NCCL_IB_DISABLE", "1")
        import torch
        import lsbsort
        if transport == "gloo":
            import torch.distributed as dist
            from bench import GlooComm
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            dist.init_process_group("gloo", rank=rank, world_size=world)
            w = lsbsort.World.rank_ops(n, world, rank, 0, GlooComm(dist, world, rank))
        else:
            if rank == 0:
                uid = lsbsort.get_unique_id()
                for _ in range(world - 1):
                    q_uid.put(uid)
            else:
                uid = q_uid.get(timeout=60)
            w = lsbsort.World.rank(n, world, rank, 0, uid)
        rec = np.load(os.path.join(result_dir, "input.npy"))
        mine = rec[rank * w.per: rank * w.per + w.here(rank)]
        w.copy_in(rank, mine)
        w.barrier()
        plan = w.select(k)
        last = w.last_select()
        m = plan["take"][rank]
        cols = {c: torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda") for c in ("keys", "values")}
        got = w.store_select(rank, **{c: t[1:1 + m] for c, t in cols.items()}, key_type=0)
        out = {c: t.cpu().numpy() for c, t in cols.items()}
        ok = got == m and all(o[0] == SENT and o[-1] == SENT for o in out.values())
        ok = ok and np.array_equal(w.copy_out(rank), mine)
        np.savez(os.path.join(result_dir, f"rank{rank}.npz"), **{c: o[1:1 + m] for c, o in out.items()})
        w.barrier()
        w.close()
        if transport == "gloo":
            dist.destroy_process_group()
        q_out.put((rank, "ok" if ok else "sentinels, count or A", plan, last))
    except Exception as e:  # report, never hang the parent
        q_out.put((rank, repr(e), None, None))


def process_case(world):
    """-> (mapped keys, k): the pivot group lies across the ranks' boundaries."""
    per = 4099
    n = world * per - 1
    rng = np.random.default_rng(70 + world)
    keys = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(np.uint64)
    keys[per - 6:(2 * per + 11 if world >= 3 else per + 9)] = np.uint64(1 << 61)  # the pivot group across the boundaries
    lo = int(np.searchsorted(np.sort(keys), np.uint64(1 << 61), "left"))
    return keys, lo + (per // 2 + 20 if world >= 3 else 8)  # inside the group: the cut falls inside rank 1


def run_processes(tmp_path, world, transport, keys, k):
    """One process per rank selects k of these keys and stores its part ->
    (the plan, the model of its rounds); every rank's last_select() is the
    model's."""
    n = keys.size
    orc = Oracle(keys)
    np.save(tmp_path / "input.npy", records(keys))
    ctx = multiprocessing.get_context("spawn")
    q_uid, q_out = ctx.Queue(), ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_process, args=(r, world, transport, port, n, k, str(tmp_path), q_uid, q_out))
             for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q_out.get(timeout=240)
            res[r[0]] = r
        for p in procs:
            p.join(timeout=60)
    finally:  # a rank that died or hangs leaves its peers in a collective: none outlives the test
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    assert all(v[1] == "ok" for v in res.values()), {r: v[1] for r, v in res.items()}
    plan = res[0][2]
    assert all(res[r][2] == plan for r in range(world))  # every rank holds the same plan
    pivot, below, equal = orc.at(k)
    assert (plan["key"], plan["below"], plan["equal"]) == (pivot, below, equal)
    assert plan == dict(plan, **w_plan(orc, k, world))
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    want = orc.selection(k)
    assert np.array_equal(np.concatenate([p["values"] for p in parts]).astype(np.uint64), want.astype(np.uint64))
    assert np.array_equal(bits_of(np.concatenate([p["keys"] for p in parts])), keys[want])
    # a rank reads its own records only, in the rounds every rank counts alike
    m = M.round_model(keys, world, k)
    lasts = [res[r][3] for r in range(world)]
    assert lasts == [(m.rounds, m.read[r]) for r in range(world)], (lasts, m.rounds, m.read)
    return plan, m


if not IN_CHILD:
    def test_three_gloo_ranks(lsb_built, tmp_path):
        plan, _ = run_processes(tmp_path, 3, "gloo", *process_case(3))
        assert 0 < plan["take"][1] < 4099  # the cut falls inside rank 1, which lies inside the pivot group

    def test_two_rccl_ranks(lsb_built, tmp_path):
        run_processes(tmp_path, 2, "rccl", *process_case(2))

    def test_three_gloo_ranks_decide_differently(lsb_built, tmp_path):
        """The mixed ranks, one per process: in round two rank 0 filters A,
        rank 1 compacts and rank 2 launches nothing and gives zeros to the
        gather; later rounds have ranks 0 and 1 compact together."""
        keys = M.mixed_keys()
        ks, _ = M.mixed_ks(keys)
        k = ks[len(ks) // 2]
        plan, m = run_processes(tmp_path, 3, "gloo", keys, k)
        assert m.trace[1].packed == (False, True, False) and m.trace[1].cand[2] == 0
        assert any(r.packed[0] and r.packed[1] for r in m.trace[2:])
        assert m.read[2] == M.MIXED_PER - 1 and plan["take"][2] == 0 and plan["take"][0] > 0 and plan["take"][1] > 0
