"""Scans within the runs on the device (lsb_plan_scan / lsb_store_scan /
lsb_scan_runs, lsbsort.group_scan, cumcount, rank; include/lsb.h "a scan
within the runs").

Inputs are built from run lengths, as in tests/test_labels_gpu.py, so every
answer is known by construction; where no sort is needed they are loaded with
copy_in.  The model is numpy on the CPU: per run np.cumsum (uint64 wraps),
np.minimum.accumulate and np.maximum.accumulate over the encoded values,
decoded again; positions for COUNT and START.

One case of the issue is not here: no entry point changes A and keeps the run
plan (every call that writes records ends it), and neither
tests/test_reduce_gpu.py nor tests/test_labels_gpu.py has a way around that,
so the recount guard of the scan's kernels cannot be made to fire from a test.
What the guard's refusal leaves behind is the code path of a dropped plan,
which test_state_and_refusals covers.

As tests/test_labels_gpu.py, the tests run in one child pytest process over
this same file that imports torch before the library is loaded
(LSB_SCAN_CHILD=1), once per session; here each test reports what its namesake
did there.  The test with real rank processes starts its own processes and runs
from the pytest process itself.
"""
import ctypes
import functools
import inspect
import multiprocessing
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_SCAN_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

from test_labels_gpu import KEYS, _free_port, bits_of, cut, cycle, host, model_encode  # noqa: E402
from test_reduce_host import splitmix64  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
INVALID, STATE = 1, 7
KEEP, BY_VALUE = 0, 1
SENT = 0x5555555555555555
SUM, MIN, MAX, COUNT, START = 0, 1, 2, 3, 4
U64, I64, F64, U32 = 0, 1, 2, 3
REC = np.dtype([("key", "<u8"), ("val", "<u8")])
SIGN = np.uint64(1 << 63)
# lane, item, wave and tile edges; runs that span whole tiles
EDGE_CYCLE = [1, 2, 3, 64, 65, 1023, 1025, 4096, 4097, 9000]


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("scan") / "child.xml"
    env = dict(os.environ, LSB_SCAN_CHILD="1")
    for name in ("LSB_REGION_MIN", "LSB_PACK_VALUES", "LSB_REGION_FIRST", "LSB_LABELS_CHILD"):
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
def values_for(n, kind):
    """The value bits (uint64) of positions 0..n-1, a hash of the position:
      hash      the hash itself (integer sums, integer min and max)
      exact     integer-valued doubles in [0, 2^38), so below 2^40: a run of
                up to 32767 of them sums exactly in every order (below 2^53)
      ordered   doubles of both signs and many exponents, with both zeros,
                both infinities and a NaN of either sign
      wide      finite doubles of both signs over 40 binades"""
    h = splitmix64(np.arange(n))
    if kind == "hash":
        return h
    if kind == "exact":
        return (h >> np.uint64(26)).astype(np.float64).view(np.uint64)
    mant = 1.0 + (h >> np.uint64(12)).astype(np.float64) * 2.0 ** -52
    d = np.ldexp(mant, ((h >> np.uint64(1)) % np.uint64(41)).astype(np.int64) - 20) * \
        np.where(h & np.uint64(1), -1.0, 1.0)
    b = d.view(np.uint64).copy()
    if kind == "ordered":
        pick = (h >> np.uint64(7)) % np.uint64(23)
        for k, bits in enumerate((0, 0x8000000000000000, 0x7ff8000000000001, 0xfff8000000000001,
                                  0x7ff0000000000000, 0xfff0000000000000)):
            b[pick == k] = bits
    return b


# (op, value type, the values' kind)
PAIRS = [(SUM, U64, "hash"), (SUM, I64, "hash"), (MIN, U64, "hash"), (MAX, U64, "hash"), (MIN, I64, "hash"),
         (MAX, I64, "hash"), (SUM, F64, "exact"), (MIN, F64, "ordered"), (MAX, F64, "ordered"),
         (COUNT, U64, "hash"), (START, U64, "hash")]


def model_decode(k, vt):
    if vt == I64:
        return k ^ SIGN
    if vt == F64:
        return np.where((k & SIGN) != 0, k ^ SIGN, ~k)
    return k


def model(vals, lengths, op, vt):
    """The inclusive scan of op over vals (uint64 bits) inside every run ->
    uint64 bits, one per record."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    first = np.repeat(starts, lengths)
    if op == COUNT:
        return (np.arange(n, dtype=np.int64) - first).astype(np.uint64)
    if op == START:
        return first.astype(np.uint64)
    out = vals.copy()
    work = vals if op == SUM else model_encode(vals, vt, False)
    if op == SUM and vt != F64:
        with np.errstate(over="ignore"):
            c = np.cumsum(vals, dtype=np.uint64)
            before = np.where(first > 0, c[np.maximum(first - 1, 0)], np.uint64(0))
            return c - before
    for lo, cnt in zip(starts[lengths > 1], lengths[lengths > 1]):
        seg = work[lo:lo + cnt]
        if op == SUM:
            out[lo:lo + cnt] = np.cumsum(seg.view(np.float64)).view(np.uint64)
        else:
            acc = (np.minimum if op == MIN else np.maximum).accumulate(seg)
            out[lo:lo + cnt] = model_decode(acc, vt)
    return out


def records(lengths, vals):
    """Records whose runs have these lengths (run j's key is j times an odd
    constant: adjacent keys differ, the keys are not sorted) with these value
    bits."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ukeys = (np.arange(lengths.size, dtype=np.uint64) + np.uint64(11)) * np.uint64(0x9E3779B97F4A7C15)
    rec = np.zeros(int(lengths.sum()), dtype=REC)
    rec["key"] = np.repeat(ukeys, lengths)
    rec["val"] = vals
    return rec


def stored(w, rank, shift=2):
    """store_scan of `rank` into a fresh column with `shift` sentinel elements
    in front and two behind that must survive -> the results' bits."""
    import torch
    h = w.here(rank)
    full = torch.full((h + shift + 2,), SENT, dtype=torch.int64, device="cuda")
    assert w.store_scan(rank, full[shift:shift + h]) == h
    got = host(full).view(np.uint64)
    assert np.all(got[:shift] == SENT) and np.all(got[shift + h:] == SENT)
    return got[shift:shift + h].copy()


def stored_all(w, P, shift=2):
    return np.concatenate([stored(w, r, shift) for r in range(P)])


def check_all_pairs(w, P, lengths, vals, what, pairs=PAIRS):
    """Every (op, type) from one count_runs: the plans stay through the stores."""
    for op, vt, kind in pairs:
        w.plan_scan(op, vt)
        got = stored_all(w, P)
        want = model(vals[kind], lengths, op, vt)
        assert np.array_equal(got, want), (what, op, vt, np.flatnonzero(got != want)[:4])


def load(w, P, rec):
    if P == 1:
        w.copy_in(0, rec)
    else:
        w.scatter_global(rec)


# ------------------------------------------------- 1. boundaries of every level, one rank
def edge_patterns(n):
    return {"one run": [n], "all distinct": np.ones(n, dtype=np.int64), "cycle": cycle(EDGE_CYCLE, n)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
@torch_first
def test_boundaries_one_rank(lsb_built, n):
    L = lsb_built
    kinds = {k: values_for(n, k) for k in ("hash", "exact", "ordered")}
    with L.World(n, ranks=1) as w:
        for name, lengths in edge_patterns(n).items():
            runs = len(lengths)
            for kind in ("hash", "ordered"):
                rec = records(lengths, kinds[kind])
                assert rec.size == n
                w.copy_in(0, rec)
                assert w.count_runs()["total"] == runs, name
                check_all_pairs(w, 1, lengths, kinds, (name, n), [p for p in PAIRS if p[2] == kind])
            rec = records(lengths, kinds["exact"])
            w.copy_in(0, rec)
            w.count_runs()
            check_all_pairs(w, 1, lengths, kinds, (name, n), [p for p in PAIRS if p[2] == "exact"])
            # the records form, both modes, a value op and a counting one; A is rec again before each
            for mode, (op, vt) in ((KEEP, (SUM, F64)), (BY_VALUE, (COUNT, U64)), (KEEP, (START, U64)),
                                   (BY_VALUE, (SUM, F64))):
                w.copy_in(0, rec)
                w.count_runs()
                w.plan_scan(op, vt)
                w.scan_runs(mode)
                got = w.copy_out(0)
                assert np.array_equal(got["key"], rec["key"] if mode == KEEP else rec["val"]), (name, n, mode)
                assert np.array_equal(got["val"], model(kinds["exact"], lengths, op, vt)), (name, n, mode, op)


@torch_first
def test_heads_around_tile_edges(lsb_built):
    """Heads at positions 4096 t - 1, 4096 t and 4096 t + 1: a run that ends
    with its tile, one that starts with it, and one record on either side."""
    L = lsb_built
    n = 5 * TILE
    heads = sorted({0} | {TILE * t + d for t in range(1, 5) for d in (-1, 0, 1)})
    lengths = np.diff(np.array(heads + [n], dtype=np.int64))
    kinds = {k: values_for(n, k) for k in ("hash", "exact", "ordered")}
    with L.World(n, ranks=1) as w:
        for kind in kinds:
            rec = records(lengths, kinds[kind])
            w.copy_in(0, rec)
            assert w.count_runs()["total"] == len(heads)
            check_all_pairs(w, 1, lengths, kinds, "tile edges", [p for p in PAIRS if p[2] == kind])
        for mode in (KEEP, BY_VALUE):
            w.copy_in(0, rec)
            w.count_runs()
            w.plan_scan(MAX, F64)
            w.scan_runs(mode)
            got = w.copy_out(0)
            assert np.array_equal(got["key"], rec["key"] if mode == KEEP else rec["val"])
            assert np.array_equal(got["val"], model(kinds["ordered"], lengths, MAX, F64))


# ------------------------------------------------- 2. the chain kernel's chunks
@torch_first
def test_more_tiles_than_chain_threads(lsb_built):
    """1025 tiles and 5 records: every thread of k_run_scan_chain that has
    tiles has two.  One run of the whole array (every tile hands on what all
    the tiles before it hold), then runs of 3 tiles and 1 record."""
    L = lsb_built
    n = 1025 * TILE + 5
    vals = {"hash": values_for(n, "hash")}
    with L.World(n, ranks=1) as w:
        for name, lengths in (("one run", [n]), ("three tiles and one", cycle([3 * TILE + 1], n))):
            rec = records(lengths, vals["hash"])
            w.copy_in(0, rec)
            assert w.count_runs()["total"] == len(lengths)
            check_all_pairs(w, 1, lengths, vals, name, [(SUM, U64, "hash"), (COUNT, U64, "hash")])


# ------------------------------------------------- 3. ranks, loopback
def rank_cases(P):
    """(name, lengths); per = ceil(n / P)."""
    cases = [
        ("three records", [2, 1]),  # P = 5: per = 1, ranks 3 and 4 are empty
        # P = 5: per = 1000; the run of 3300 begins in rank 0, holds ranks 1 and 2 whole and ends inside rank 3
        ("whole middle ranks", [400, 3300, 1, 1299]),
        ("cycle", cycle(EDGE_CYCLE, 5 * 4097)),
    ]
    per = 1001
    n = P * per
    # a run ends at every rank's last slot, and the next starts at the first slot
    cases.append(("ends at the boundary", cut([5, per - 5] * P, n)))
    return cases


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_ranks_loopback(lsb_built, P):
    L = lsb_built
    for name, lengths in rank_cases(P):
        lengths = np.asarray(lengths, dtype=np.int64)
        n = int(lengths.sum())
        kinds = {k: values_for(n, k) for k in ("hash", "exact", "ordered")}
        with L.World(n, ranks=P) as w:
            if name == "three records" and P == 5:
                assert w.here(2) == 1 and w.here(3) == 0
            for kind in kinds:
                rec = records(lengths, kinds[kind])
                w.scatter_global(rec)
                plan = w.count_runs()
                assert plan["total"] == lengths.size, name
                if name == "whole middle ranks" and P == 5:
                    assert plan["runs"][1] == 0 and plan["runs"][2] == 0
                check_all_pairs(w, P, lengths, kinds, (name, P), [p for p in PAIRS if p[2] == kind])
            # START and COUNT by construction, through the records form
            starts = np.repeat(np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths).astype(np.uint64)
            for mode, op, want in ((KEEP, START, starts), (BY_VALUE, COUNT, np.arange(n, dtype=np.uint64) - starts)):
                w.scatter_global(rec)
                w.count_runs()
                w.plan_scan(op, U64)
                w.scan_runs(mode)
                got = w.gather_global()
                assert np.array_equal(got["key"], rec["key"] if mode == KEEP else rec["val"]), (name, P)
                assert np.array_equal(got["val"], want), (name, P, op)


# ------------------------------------------------- 4. floats
@pytest.mark.parametrize("P", [1, 3])
@torch_first
def test_f64_sum_of_arbitrary_doubles(lsb_built, P):
    """Two calls give the same bits.  Against np.cumsum per run, at the run's
    m-th record |got - want| <= 2 (m - 1) 2^-53 sum |v| over its first m
    values: (m - 1) u sum |v| bounds the error of recursive summation in any
    order (Higham, Accuracy and Stability of Numerical Algorithms, §4.2, to
    first order), taken once for each side.  Adding the identity -0.0 is exact
    and adds no term."""
    L = lsb_built
    n = 3 * TILE + 17
    lengths = cycle(EDGE_CYCLE, n)
    vals = values_for(n, "wide")
    rec = records(lengths, vals)
    with L.World(n, ranks=P) as w:
        load(w, P, rec)
        w.count_runs()
        w.plan_scan(SUM, F64)
        first = stored_all(w, P)
        w.count_runs()
        w.plan_scan(SUM, F64)
        again = stored_all(w, P, shift=3)
    assert np.array_equal(first, again)
    x = vals.view(np.float64)
    got = first.view(np.float64)
    lo = 0
    for cnt in lengths:
        seg = x[lo:lo + cnt]
        bound = 2.0 * np.arange(cnt) * 2.0 ** -53 * np.cumsum(np.abs(seg))
        err = np.abs(got[lo:lo + cnt] - np.cumsum(seg))
        assert np.all(err <= bound), (lo, cnt, float(np.max(err - bound)))
        lo += cnt


@torch_first
def test_f64_zeros_and_order(lsb_built):
    """A run of -0.0 scans to -0.0 (the identity is -0.0, not +0.0), and one
    +0.0 turns the rest of its run to +0.0; MIN and MAX return the run's own
    bits in lsb.h's order: a NaN with the sign set below -inf, -0.0 below +0.0,
    a NaN with the sign clear above +inf."""
    L = lsb_built
    nz, pz = 0x8000000000000000, 0
    n = 2 * TILE + 9
    lengths = [TILE + 3, n - TILE - 3]
    vals = np.full(n, nz, dtype=np.uint64)
    vals[TILE + 3 + 70] = pz
    want = vals.copy()
    want[TILE + 3 + 70:] = pz
    order = np.array([0xfff8000000000001, 0xfff0000000000000, np.float64(-1.5).view(np.uint64), nz, pz,
                      np.float64(2.5).view(np.uint64), 0x7ff0000000000000, 0x7ff8000000000001], dtype=np.uint64)
    with L.World(n, ranks=1) as w:
        w.copy_in(0, records(lengths, vals))
        w.count_runs()
        w.plan_scan(SUM, F64)
        assert np.array_equal(stored(w, 0), want)
    m = order.size
    with L.World(2 * m, ranks=1) as w:
        # a run falling through the order, then one rising through it
        both = np.concatenate([order[::-1], order])
        w.copy_in(0, records([m, m], both))
        w.count_runs()
        w.plan_scan(MIN, F64)
        assert np.array_equal(stored(w, 0), np.concatenate([order[::-1], np.full(m, order[0])]))
        w.plan_scan(MAX, F64)
        assert np.array_equal(stored(w, 0), np.concatenate([np.full(m, order[-1]), order]))


# ------------------------------------------------- 5. agreement with the reductions
@pytest.mark.parametrize("P", [1, 3])
@torch_first
def test_last_record_is_the_reduction(lsb_built, P):
    """From one count_runs: the scan's value at every run's last record is
    what store_reduce writes for the run, bit for bit for MIN, MAX and the
    integer SUM, and within the two orders' rounding for the F64 SUM."""
    import torch
    L = lsb_built
    n = 3 * TILE + 17
    lengths = cycle(EDGE_CYCLE, n)
    last = np.cumsum(lengths) - 1
    m = len(lengths)
    kinds = {k: values_for(n, k) for k in ("hash", "ordered", "wide")}
    pairs = [(SUM, U64, "hash"), (SUM, I64, "hash"), (MIN, I64, "hash"), (MAX, U64, "hash"), (MIN, F64, "ordered"),
             (MAX, F64, "ordered"), (SUM, F64, "wide")]
    with L.World(n, ranks=P) as w:
        for kind in kinds:
            rec = records(lengths, kinds[kind])
            load(w, P, rec)
            plan = w.count_runs()
            for op, vt, k in pairs:
                if k != kind:
                    continue
                w.plan_reduce(op, vt)
                w.plan_scan(op, vt)  # both plans live side by side
                red = torch.zeros(m, dtype=torch.int64, device="cuda")
                for r in range(P):
                    lo, cnt = plan["bases"][r], plan["runs"][r]
                    if cnt:
                        assert w.store_reduce(r, red[lo:lo + cnt]) == cnt
                red = host(red).view(np.uint64)
                scan = stored_all(w, P)[last]
                if (op, vt) != (SUM, F64):
                    assert np.array_equal(scan, red), (op, vt)
                    continue
                x = np.abs(kinds[kind].view(np.float64))
                total = np.add.reduceat(x, np.concatenate([[0], last[:-1] + 1]))
                bound = 2.0 * (np.asarray(lengths) - 1) * 2.0 ** -53 * total
                assert np.all(np.abs(scan.view(np.float64) - red.view(np.float64)) <= bound)


# ------------------------------------------------- 6. state and arguments
@torch_first
def test_state_and_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = 3 * TILE + 17
    lengths = cycle(EDGE_CYCLE, n)
    vals = values_for(n, "hash")
    rec = records(lengths, vals)
    want = model(vals, lengths, MIN, I64)
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, rec)
        col = torch.full((n + 3,), SENT, dtype=torch.int64, device="cuda")
        small = torch.zeros(16, dtype=torch.int64, device="cuda")
        host_arr = np.full(n, SENT, dtype=np.uint64)
        torch.cuda.synchronize()
        count = ctypes.c_int64(-1)

        def call(rank=0, cap=n, out=col.data_ptr()):
            count.value = -1
            return lib.lsb_store_scan(h, rank, cap, out, ctypes.byref(count))

        def untouched():
            torch.cuda.synchronize()
            return bool((col == SENT).all()) and bool(np.all(host_arr == SENT))

        # no run plan: no scan plan either
        assert lib.lsb_plan_scan(h, SUM, U64) == STATE
        assert call() == STATE and untouched()
        assert lib.lsb_scan_runs(h, KEEP) == STATE
        # a run plan alone is not a scan plan
        w.count_runs()
        assert call() == STATE and untouched()
        assert lib.lsb_scan_runs(h, KEEP) == STATE and lib.lsb_scan_runs(h, BY_VALUE) == STATE
        assert np.array_equal(w.copy_out(0), rec)
        # none after anything that can change A, or after a new count
        changes = [("my_sort", w.my_sort), ("copy_in", lambda: w.copy_in(0, rec[:5], off=3)),
                   ("load_columns", lambda: w.load_columns(0, small, key_type=0)), ("generate", w.generate),
                   ("count_runs", w.count_runs)]
        for what, change in changes:
            w.count_runs()
            w.plan_scan(SUM, U64)
            change()
            assert call() == STATE and untouched(), what
            assert lib.lsb_scan_runs(h, KEEP) == STATE, what
            with pytest.raises(L.LsbError) as e:
                w.store_scan(0, col)
            assert e.value.code == STATE, what
        w.copy_in(0, rec)
        assert w.count_runs()["total"] == len(lengths)
        w.plan_scan(MIN, I64)
        refusals = [
            ("cap one short", lambda: call(cap=n - 1)),
            ("negative cap", lambda: call(cap=-1)),
            ("rank 1", lambda: call(rank=1)),
            ("rank -1", lambda: call(rank=-1)),
            ("null out", lambda: call(out=None)),
            ("host pointer", lambda: call(out=host_arr.ctypes.data)),
            ("off by 4 bytes", lambda: call(out=col.data_ptr() + 4)),
            ("leaves the allocation", lambda: call(cap=1 << 40)),
            ("op 5", lambda: lib.lsb_plan_scan(h, 5, I64)),
            ("op -1", lambda: lib.lsb_plan_scan(h, -1, I64)),
            ("a 32-bit value type", lambda: lib.lsb_plan_scan(h, MIN, U32)),
            ("value type 6", lambda: lib.lsb_plan_scan(h, MIN, 6)),
            ("COUNT over F64", lambda: lib.lsb_plan_scan(h, COUNT, F64)),
            ("START over I64", lambda: lib.lsb_plan_scan(h, START, I64)),
            ("mode 2", lambda: lib.lsb_scan_runs(h, 2)),
            ("mode -1", lambda: lib.lsb_scan_runs(h, -1)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
            if what == "cap one short":
                assert count.value == n
        for bad in (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int64),
                    torch.zeros((n, 2), dtype=torch.int64, device="cuda")):
            with pytest.raises(ValueError):
                w.store_scan(0, bad)
        # the plan survived every refusal; a column aligned to 8 bytes only gives what one aligned to 16 gives
        assert col.data_ptr() % 16 == 0
        assert np.array_equal(stored(w, 0, shift=2), want)
        assert np.array_equal(stored(w, 0, shift=1), want)
        assert np.array_equal(w.copy_out(0), rec)  # the stores left A alone
        # a successful scan_runs ends the run, reduce, scan and select plans
        w.plan_reduce(L.REDUCE_SUM, L.KEY_U64)
        w.select(n // 2)
        w.scan_runs(KEEP)
        got = w.copy_out(0)
        assert np.array_equal(got["key"], rec["key"]) and np.array_equal(got["val"], want)
        assert call() == STATE and untouched()
        assert lib.lsb_scan_runs(h, KEEP) == STATE and lib.lsb_plan_scan(h, SUM, U64) == STATE
        for refused in (lambda: w.store_runs(0, keys=col, key_type=0), lambda: w.store_reduce(0, col),
                        lambda: w.store_select(0, keys=col, key_type=0)):
            with pytest.raises(L.LsbError) as e:
                refused()
            assert e.value.code == STATE
        assert np.array_equal(w.copy_out(0), got)  # the refused calls left the records alone
        # and the context sorts and verifies afterwards
        w.generate()
        w.my_sort()
        assert w.verify() == (True, -1)
    for P in (2, 3):  # n = 0: nothing to scan, nothing launched
        with L.World(0, ranks=P) as w:
            assert lib.lsb_plan_scan(w._h, SUM, U64) == STATE
            assert w.count_runs()["total"] == 0
            assert lib.lsb_scan_runs(w._h, KEEP) == STATE
            w.plan_scan(COUNT, U64)
            assert lib.lsb_scan_runs(w._h, 2) == INVALID
            assert w.store_scan(0, small) == 0
            w.scan_runs(BY_VALUE)


# ------------------------------------------------- 7. the Python functions
def py_keys(name, n):
    """n keys of at most 40 distinct values of the type, negative ones and
    (f32) both zeros among them."""
    kt, dt = KEYS[name]
    v = np.random.default_rng(70 + kt).integers(0, 40, n).astype(np.int64)
    if name == "u64":
        return v.astype(np.uint64) * np.uint64(0x0640_0100_4001_0011)
    if name == "i32":
        return ((v - 20) * 0x03680201).astype(np.int32)
    a = ((v - 20) * 0.37).astype(np.float32)
    a[v == 7] = np.float32(-0.0)
    return a


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", [0, 1, TILE + 1, 20000])
@torch_first
def test_python_functions(lsb_built, n, descending, ranks):
    """group_scan, cumcount and rank against a stable argsort of the encoded
    keys, the per-run model over the sorted records, and a scatter back."""
    import torch
    L = lsb_built
    for name in ("u64", "i32", "f32"):
        kt, dt = KEYS[name]
        keys = py_keys(name, n)
        enc = model_encode(bits_of(keys), kt, descending)
        order = np.argsort(enc, kind="stable")
        heads = np.flatnonzero(np.concatenate([[True], enc[order][1:] != enc[order][:-1]])) if n else np.zeros(0, int)
        lengths = np.diff(np.append(heads, n))
        key_np = {"u64": np.int64}.get(name, dt)
        dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
        kw = dict(descending=descending, ranks=ranks, key_type=kt)

        def back(sorted_bits):
            out = np.zeros(n, dtype=np.uint64)
            out[order] = sorted_bits
            return out

        cc, rk = L.cumcount(dk, **kw), L.rank(dk, **kw)
        for t in (cc, rk):
            assert t.dtype == torch.int64 and t.device == dk.device and t.shape == dk.shape
        assert np.array_equal(bits_of(host(cc)), back(model(None, lengths, COUNT, U64))), (name, "cumcount")
        assert np.array_equal(bits_of(host(rk)), back(model(None, lengths, START, U64))), (name, "rank")
        for op, opname, vt, kind, vdt in ((SUM, "sum", I64, "hash", np.int64), (MIN, "min", I64, "hash", np.int64),
                                          (MAX, "max", F64, "ordered", np.float64),
                                          (SUM, "sum", F64, "exact", np.float64)):
            vals = values_for(n, kind)
            dv = torch.from_numpy(vals.view(vdt).copy()).cuda()
            got = L.group_scan(dk, dv, opname, **kw)
            assert got.dtype == dv.dtype and got.device == dk.device and got.shape == dk.shape
            assert np.array_equal(bits_of(host(got)), back(model(vals[order], lengths, op, vt))), (name, opname)
            assert np.array_equal(bits_of(host(dv)), vals)  # the inputs are untouched
        assert np.array_equal(bits_of(host(dk)), bits_of(keys))


@torch_first
def test_python_refusals(lsb_built):
    import torch
    L = lsb_built
    dk = torch.arange(8, dtype=torch.int64, device="cuda")
    dv = torch.arange(8, dtype=torch.int64, device="cuda")
    bad = [
        lambda: L.group_scan(dk, dv, "mean"),                               # a bad op
        lambda: L.group_scan(dk, dv[:7]),                                   # a length mismatch
        lambda: L.group_scan(dk, dv.to(torch.int32)),                       # values of a dtype no scan reads
        lambda: L.group_scan(dk.to(torch.int16), dv),                       # keys of a dtype no sort reads
        lambda: L.cumcount(dk.to(torch.int16)),
        lambda: L.rank(dk.cpu()),
        lambda: L.rank(dk, ranks=0),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------- 8. real processes
PROCESS_PAIRS = ((SUM, U64), (MIN, I64), (COUNT, U64), (START, U64))


def _rank_process(rank, world, port, n, result_dir, q_out):
    """One rank of a one-rank-per-process world over the ops transport: count,
    then plan and store each scan of its records into its own torch tensor,
    and the records form of the last."""
    try:
        for p in (ROOT, os.path.join(ROOT, "distributed-lsb_amd")):
            sys.path.insert(0, p)
        import torch
        import torch.distributed as dist
        import lsbsort
        from bench import GlooComm
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        w = lsbsort.World.rank_ops(n, world, rank, 0, GlooComm(dist, world, rank))
        rec = np.load(os.path.join(result_dir, "input.npy"))
        mine = rec[rank * w.per: rank * w.per + w.here(rank)]
        w.copy_in(rank, mine)
        w.barrier()
        w.count_runs()
        h = w.here(rank)
        ok, out = True, {}
        for op, vt in PROCESS_PAIRS:
            w.plan_scan(op, vt)
            col = torch.full((h + 2,), SENT, dtype=torch.int64, device="cuda")
            got = w.store_scan(rank, col[1:1 + h])
            o = col.cpu().numpy()
            ok = ok and got == h and o[0] == SENT and o[-1] == SENT
            out[f"op{op}"] = o[1:1 + h]
        w.scan_runs(lsbsort.LABEL_KEEP)
        w.sync()
        out["records"] = w.copy_out(rank)
        np.savez(os.path.join(result_dir, f"rank{rank}.npz"), **out)
        w.barrier()
        w.close()
        dist.destroy_process_group()
        q_out.put((rank, "ok" if ok else "sentinels or count"))
    except Exception as e:  # report, never hang the parent
        q_out.put((rank, repr(e)))


if not IN_CHILD:
    def test_two_gloo_ranks(lsb_built, tmp_path):
        """Seven records, per = 4: the run of three lies across the boundary."""
        world, lengths = 2, [3, 3, 1]
        n = sum(lengths)
        vals = values_for(n, "hash")
        rec = records(lengths, vals)
        np.save(tmp_path / "input.npy", rec)
        ctx = multiprocessing.get_context("spawn")
        q_out = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_rank_process, args=(r, world, port, n, str(tmp_path), q_out))
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
        finally:  # a rank that died or hangs leaves its peer in a collective: none outlives the test
            for p in procs:
                if p.is_alive():
                    p.kill()
                    p.join(timeout=30)
        assert all(v[1] == "ok" for v in res.values()), {r: v[1] for r, v in res.items()}
        parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
        for op, vt in PROCESS_PAIRS:
            got = np.concatenate([parts[r][f"op{op}"] for r in range(world)])
            assert np.array_equal(bits_of(got), model(vals, lengths, op, vt)), (op, vt)
        got = np.concatenate([parts[r]["records"] for r in range(world)])
        assert np.array_equal(got["key"], rec["key"])
        assert np.array_equal(got["val"], model(vals, lengths, START, U64))
