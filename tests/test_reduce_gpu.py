"""Reductions over the runs' values on the device (lsb_plan_reduce /
lsb_store_reduce, lsbsort.group_reduce; include/lsb.h "runs of equal keys",
DESIGN.md §7.3).

Inputs are built from run lengths, as in tests/test_runs_gpu.py; a record's
value is a hash of its position (splitmix64), so a dropped, doubled or
misplaced record changes the result of every op.  The model is numpy on the
CPU: np.add.reduceat over uint64 (which wraps) or over exactly summable
doubles, np.minimum / np.maximum.reduceat over the encoded values, the
encoding written out in tests/test_runs_gpu.py from the header's table.

The outputs are torch CUDA tensors, so the tests run in one child pytest
process over this same file that imports torch before the library is loaded
(LSB_REDUCE_CHILD=1), once per session; here each test reports what its
namesake did there.  The tests with real rank processes start their own
processes and run from the pytest process itself.
"""
import ctypes
import functools
import inspect
import math
import multiprocessing
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_REDUCE_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

from test_reduce_host import splitmix64  # noqa: E402
from test_runs_gpu import (KEYS, TILE, _free_port, bits_of, cut, cycle, geometric, host,  # noqa: E402
                           launcher_constants, model_encode, rank_cases, tie_keys)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 7
SENT = 0x5555555555555555
SUM, MIN, MAX = 0, 1, 2
U64, I64, F64, U32 = 0, 1, 2, 3
OPS = {"sum": SUM, "min": MIN, "max": MAX}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("reduce") / "child.xml"
    env = dict(os.environ, LSB_REDUCE_CHILD="1")
    for name in ("LSB_REGION_MIN", "LSB_PACK_VALUES", "LSB_REGION_FIRST", "LSB_RUNS_CHILD"):
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
      exact     integer-valued doubles below 2^31 in magnitude: every order of
                addition is exact (a run's sum stays below 2^53)
      ordered   doubles of both signs and many exponents, with both zeros and
                a NaN of either sign
      wide      finite doubles of both signs over 40 binades"""
    h = splitmix64(np.arange(n))
    if kind == "hash":
        return h
    if kind == "exact":
        return ((h >> np.uint64(33)).astype(np.int64) - (1 << 30)).astype(np.float64).view(np.uint64)
    mant = 1.0 + (h >> np.uint64(12)).astype(np.float64) * 2.0 ** -52
    d = np.ldexp(mant, ((h >> np.uint64(1)) % np.uint64(41)).astype(np.int64) - 20) * \
        np.where(h & np.uint64(1), -1.0, 1.0)
    b = d.view(np.uint64).copy()
    if kind == "ordered":
        pick = (h >> np.uint64(7)) % np.uint64(19)
        b[pick == 0] = 0
        b[pick == 1] = 0x8000000000000000
        b[pick == 2] = 0x7ff8000000000001
        b[pick == 3] = 0xfff8000000000001
    return b


# (op, value type, the values' kind)
PAIRS = [(SUM, U64, "hash"), (MIN, U64, "hash"), (MIN, I64, "hash"), (MAX, I64, "hash"),
         (SUM, F64, "exact"), (MIN, F64, "ordered"), (MAX, F64, "ordered")]


def model(vals, starts, op, vt):
    """op over vals (uint64 bits) per segment from starts -> uint64 bits."""
    starts = np.asarray(starts, dtype=np.int64)
    if op == SUM and vt == F64:
        return np.add.reduceat(vals.view(np.float64), starts).view(np.uint64)
    if op == SUM:
        with np.errstate(over="ignore"):
            return np.add.reduceat(vals, starts)
    e = model_encode(vals, vt, False)
    want = (np.minimum if op == MIN else np.maximum).reduceat(e, starts)
    # decode by index: the first record of each segment whose encoding is the extreme
    seg = np.repeat(np.arange(starts.size), np.diff(np.append(starts, vals.size)))
    hit = np.flatnonzero(e == want[seg])
    at = hit[np.concatenate([[True], seg[hit][1:] != seg[hit][:-1]])]
    assert at.size == starts.size and np.array_equal(e[at], want)
    return vals[at]


def records(lengths, vals):
    """Records whose runs have these lengths (run j's key is j times an odd
    constant, as tests/test_runs_gpu.py) with these value bits, and the runs'
    starts."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    ukeys = (np.arange(lengths.size, dtype=np.uint64) + np.uint64(11)) * np.uint64(0x9E3779B97F4A7C15)
    rec = np.zeros(n, dtype=[("key", "<u8"), ("val", "<u8")])
    rec["key"] = np.repeat(ukeys, lengths)
    rec["val"] = vals
    return rec, np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)


def reduced(w, rank, m, extra=0):
    """store_reduce of `rank` into a fresh column of m + extra elements with
    two sentinel elements on either side; the sentinels and the extra
    elements must survive -> the m values' bits."""
    import torch
    full = torch.full((m + extra + 4,), SENT, dtype=torch.int64, device="cuda")
    assert w.store_reduce(rank, full[2:2 + m + extra]) == m
    h = host(full).view(np.uint64)
    assert np.all(h[:2] == SENT) and np.all(h[2 + m:] == SENT)
    return h[2:2 + m].copy()


# ------------------------------------------------- 1. lane, item, wave and tile edges, one rank
def edge_patterns(n):
    pats = {"all equal": [n], "all distinct": np.ones(n, dtype=np.int64),
            "geometric 3": geometric(3, n, 1), "geometric 700": geometric(700, n, 2)}
    for step in (63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1):
        pats[f"heads every {step}"] = cycle([step], n)
    return pats


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@torch_first
def test_edges_one_rank(lsb_built, n):
    L = lsb_built
    vals = {kind: values_for(n, kind) for kind in ("hash", "exact", "ordered")}
    with L.World(n, ranks=1) as w:
        for name, lengths in edge_patterns(n).items():
            for op, vt, kind in PAIRS:
                rec, starts = records(lengths, vals[kind])
                assert rec.size == n
                m = starts.size
                w.copy_in(0, rec)
                assert w.count_runs() == {"total": m, "runs": [m], "bases": [0]}, name
                w.plan_reduce(op, vt)
                want = model(vals[kind], starts, op, vt)
                assert np.array_equal(reduced(w, 0, m), want), (name, op, vt)
            # a column longer than the runs takes them at its start and keeps the rest
            assert np.array_equal(reduced(w, 0, m, extra=7), want), name


# ------------------------------------------------- 2. more tiles than workgroups and carry threads
@torch_first
def test_more_tiles_than_workgroups(lsb_built):
    """Every workgroup of k_run_reduce takes a second tile and every thread of
    k_run_carry several; runs span tiles, the longest several carry chunks."""
    L = lsb_built
    grid_cap, scan_block = launcher_constants()
    n = grid_cap * TILE + TILE + 1
    tiles = -(-n // TILE)
    assert tiles > grid_cap and tiles > scan_block and 300001 > 3 * TILE * -(-tiles // scan_block)
    lengths = cycle([1, 2, TILE - 1, TILE, TILE + 1, 70001, 300001], n)
    with L.World(n, ranks=1) as w:
        for op, vt, kind in ((SUM, U64, "hash"), (MIN, I64, "hash"), (SUM, F64, "exact")):
            vals = values_for(n, kind)
            rec, starts = records(lengths, vals)
            m = starts.size
            w.copy_in(0, rec)
            del rec
            assert w.count_runs()["total"] == m
            w.plan_reduce(op, vt)
            assert np.array_equal(reduced(w, 0, m), model(vals, starts, op, vt)), (op, vt)


# ------------------------------------------------- 3. rank edges, loopback
def check_world(L, P, lengths, name):
    n = int(np.sum(lengths))
    for op, vt, kind in ((SUM, U64, "hash"), (MIN, I64, "hash"), (SUM, F64, "exact"), (MAX, F64, "ordered")):
        vals = values_for(n, kind)
        rec, starts = records(lengths, vals)
        want = model(vals, starts, op, vt)
        with L.World(n, ranks=P) as w:
            w.scatter_global(rec)
            plan = w.count_runs()
            owner = starts // max(w.per, 1)
            runs = [int(np.count_nonzero(owner == r)) for r in range(P)]
            assert plan["total"] == starts.size and plan["runs"] == runs, name
            w.plan_reduce(op, vt)
            # the ranks' outputs, laid end to end by bases, are the global answer
            glob = np.zeros(plan["total"], dtype=np.uint64)
            for r in range(P):
                glob[plan["bases"][r]:plan["bases"][r] + runs[r]] = reduced(w, r, runs[r], extra=3 if runs[r] == 0 else 0)
            assert np.array_equal(glob, want), (name, op, vt)
    return plan


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_rank_edges_loopback(lsb_built, P):
    for name, lengths in rank_cases(P):
        plan = check_world(lsb_built, P, lengths, name)
        if name == "one key":  # ranks 1.. own no run: 0 runs, their sentinel-filled columns untouched (reduced())
            assert plan["runs"] == [1] + [0] * (P - 1)
        if name == "three ranks":
            assert plan["runs"][1] == 0
    # n < P: empty ranks
    for lengths in ([1], [2], [1, 1], [1, 2], [2, 2]):
        if sum(lengths) < P:
            check_world(lsb_built, P, lengths, ("n < P", lengths))
    with lsb_built.World(0, ranks=P) as w:
        assert w.count_runs() == {"total": 0, "runs": [0] * P, "bases": [0] * P}
        w.plan_reduce(SUM, F64)
        for r in range(P):
            assert reduced(w, r, 0, extra=3).size == 0


# ------------------------------------------------- 4. through a sort, typed
N = 300_007


def sort_model(keys, kt, descending, vals, op, vt):
    """A stable argsort of the encoded keys, then reduceat -> (key bits, value bits)."""
    enc = model_encode(bits_of(keys), kt, descending)
    order = np.argsort(enc, kind="stable")
    se = enc[order]
    starts = np.flatnonzero(np.concatenate([[True], se[1:] != se[:-1]]))
    return bits_of(keys[order][starts]), model(vals[order], starts, op, vt)


@pytest.mark.parametrize("radix_bits", [8, 64])
@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("name,descending,vname", [("i64", False, "i64"), ("f32", True, "f64"), ("u32", False, "i64")])
@torch_first
def test_group_reduce_through_a_sort(lsb_built, name, descending, vname, ranks, radix_bits):
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    keys = tie_keys(name)
    assert np.unique(bits_of(keys)).size <= 4096
    vt, vdt, kind = (I64, np.int64, "hash") if vname == "i64" else (F64, np.float64, "exact")
    vals = values_for(N, kind)
    # uint32 columns travel as int32 tensors (key_type= names the type)
    key_np = {"u32": np.int32}.get(name, dt)
    dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
    dv = torch.from_numpy(vals.view(vdt).copy()).cuda()
    for opname, op in OPS.items():
        uk, red = L.group_reduce(dk, dv, op=opname, descending=descending, ranks=ranks, radix_bits=radix_bits,
                                 key_type=kt)
        want_k, want_v = sort_model(keys, kt, descending, vals, op, vt)
        assert uk.dtype == dk.dtype and red.dtype == dv.dtype and uk.device == dk.device and red.device == dk.device
        assert np.array_equal(bits_of(host(uk)), want_k), opname
        assert np.array_equal(bits_of(host(red)), want_v), opname
    # the inputs are untouched
    assert np.array_equal(bits_of(host(dk)), bits_of(keys)) and np.array_equal(bits_of(host(dv)), vals)


@torch_first
def test_group_reduce_interface(lsb_built):
    import torch
    L = lsb_built
    k = torch.empty(0, dtype=torch.float32, device="cuda")
    v = torch.empty(0, dtype=torch.float64, device="cuda")
    for ranks in (1, 3):
        uk, red = L.group_reduce(k, v, op="max", ranks=ranks)
        assert uk.numel() == red.numel() == 0 and uk.dtype == torch.float32 and red.dtype == torch.float64
        assert uk.device == k.device and red.device == k.device
    k = torch.arange(10, dtype=torch.int64, device="cuda")
    uk, red = L.group_reduce(k, k.clone(), op="min")
    assert torch.equal(uk, k) and torch.equal(red, k)
    for bad in (lambda: L.group_reduce(k, torch.zeros(10, dtype=torch.int16, device="cuda")),
                lambda: L.group_reduce(k, torch.zeros(10, dtype=torch.int32, device="cuda")),
                lambda: L.group_reduce(k, torch.zeros(10, dtype=torch.float32, device="cuda")),
                lambda: L.group_reduce(torch.zeros(10, dtype=torch.int16, device="cuda"), k),
                lambda: L.group_reduce(k, k, op="mean"),
                lambda: L.group_reduce(k, k[:9]),
                lambda: L.group_reduce(k, torch.zeros(10, dtype=torch.int64)),
                lambda: L.group_reduce(torch.zeros((2, 5), dtype=torch.int64, device="cuda"), k)):
        with pytest.raises(ValueError):
            bad()
    assert (L.REDUCE_SUM, L.REDUCE_MIN, L.REDUCE_MAX) == (0, 1, 2)


# ------------------------------------------------- 5. F64 sum of arbitrary doubles
@pytest.mark.parametrize("P", [1, 3])
@torch_first
def test_f64_sum_of_arbitrary_doubles(lsb_built, P):
    """Two calls give the same bits; against math.fsum per run of m records
    |got - exact| <= gamma * sum |x| with gamma = (m - 1) u / (1 - (m - 1) u),
    u = 2^-53: the bound of recursive summation in any order (Higham,
    Accuracy and Stability of Numerical Algorithms, §4.2).  Adding the
    identity -0.0 is exact and adds no term."""
    L = lsb_built
    n = 3 * TILE + 5
    lengths = geometric(700, n, 5)
    vals = values_for(n, "wide")
    rec, starts = records(lengths, vals)
    m = starts.size
    with L.World(n, ranks=P) as w:
        w.scatter_global(rec)
        plan = w.count_runs()
        assert plan["total"] == m
        w.plan_reduce(SUM, F64)
        first = np.concatenate([reduced(w, r, plan["runs"][r]) for r in range(P)])
        w.count_runs()
        w.plan_reduce(SUM, F64)
        again = np.concatenate([reduced(w, r, plan["runs"][r]) for r in range(P)])
    assert np.array_equal(first, again)
    x = vals.view(np.float64)
    u = 2.0 ** -53
    for j, (lo, cnt) in enumerate(zip(starts, lengths)):
        seg = x[lo:lo + cnt]
        gamma = (cnt - 1) * u / (1 - (cnt - 1) * u)
        got = float(first[j:j + 1].view(np.float64)[0])
        assert abs(got - math.fsum(seg)) <= gamma * math.fsum(np.abs(seg)), (j, cnt, got)


# ------------------------------------------------- 6. state and refusals
@torch_first
def test_state_and_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = 200_003
    vals = values_for(n, "hash")
    rec, starts = records(geometric(700, n, 9), vals)
    m = starts.size
    want = model(vals, starts, MIN, I64)
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, rec)
        col = torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda")
        small = torch.zeros(16, dtype=torch.int64, device="cuda")
        host_arr = np.full(m, SENT, dtype=np.uint64)
        torch.cuda.synchronize()
        runs = ctypes.c_int64(-1)

        def call(rank=0, cap=m, out=col.data_ptr()):
            runs.value = -1
            return lib.lsb_store_reduce(h, rank, cap, out, ctypes.byref(runs))

        def untouched():
            torch.cuda.synchronize()
            return bool((col == SENT).all()) and bool(np.all(host_arr == SENT))

        # no run plan, no reduce plan
        assert call() == STATE and untouched()
        assert lib.lsb_plan_reduce(h, SUM, U64) == STATE
        w.count_runs()
        assert call() == STATE and untouched()
        # none after anything that can change A, or after a new count
        changes = [("my_sort", w.my_sort), ("copy_in", lambda: w.copy_in(0, rec[:5], off=3)),
                   ("load_columns", lambda: w.load_columns(0, small, key_type=0)), ("generate", w.generate),
                   ("global_shuffle", lambda: w.global_shuffle(0)), ("count_runs", w.count_runs)]
        for what, change in changes:
            w.count_runs()
            w.plan_reduce(SUM, U64)
            change()
            assert call() == STATE and untouched(), what
            with pytest.raises(L.LsbError) as e:
                w.store_reduce(0, col)
            assert e.value.code == STATE, what
        w.copy_in(0, rec)
        assert w.count_runs()["total"] == m
        w.plan_reduce(MIN, I64)
        refusals = [
            ("cap one short", lambda: call(cap=m - 1)),
            ("negative cap", lambda: call(cap=-1)),
            ("rank 1", lambda: call(rank=1)),
            ("rank -1", lambda: call(rank=-1)),
            ("null out", lambda: call(out=None)),
            ("host pointer", lambda: call(out=host_arr.ctypes.data)),
            ("off by 4 bytes", lambda: call(out=col.data_ptr() + 4)),
            ("leaves the allocation", lambda: call(cap=1 << 40)),
            ("op 3", lambda: lib.lsb_plan_reduce(h, 3, I64)),
            ("op -1", lambda: lib.lsb_plan_reduce(h, -1, I64)),
            ("a 32-bit value type", lambda: lib.lsb_plan_reduce(h, MIN, U32)),
            ("value type 6", lambda: lib.lsb_plan_reduce(h, MIN, 6)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
            if what == "cap one short":
                assert runs.value == m
        for bad in (torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int64),
                    torch.zeros((m, 2), dtype=torch.int64, device="cuda")):
            with pytest.raises(ValueError):
                w.store_reduce(0, bad)
        # the plan survived every refusal
        assert np.array_equal(reduced(w, 0, m), want)
        # and the context sorts and verifies afterwards
        w.generate()
        w.my_sort()
        assert w.verify() == (True, -1)


# ------------------------------------------------- 7. real processes
PROCESS_PAIRS = ((SUM, U64), (MIN, I64))


def _rank_process(rank, world, transport, port, n, result_dir, q_uid, q_out):
    """One rank of a one-rank-per-process world: count, then plan and store
    each reduction of its runs into its own torch tensor."""
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
        w.copy_in(rank, rec[rank * w.per: rank * w.per + w.here(rank)])
        w.barrier()
        plan = w.count_runs()
        m = plan["runs"][rank]
        ok, out = True, {}
        for op, vt in PROCESS_PAIRS:
            w.plan_reduce(op, vt)
            col = torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda")
            got = w.store_reduce(rank, col[1:1 + m])
            o = col.cpu().numpy()
            ok = ok and got == m and o[0] == SENT and o[-1] == SENT
            out[f"op{op}"] = o[1:1 + m]
        np.savez(os.path.join(result_dir, f"rank{rank}.npz"), **out)
        w.barrier()
        w.close()
        if transport == "gloo":
            dist.destroy_process_group()
        q_out.put((rank, "ok" if ok else "sentinels or count", plan))
    except Exception as e:  # report, never hang the parent
        q_out.put((rank, repr(e), None))


def run_processes(tmp_path, world, transport):
    per = 4099
    n = world * per - 1
    # one run across both of three ranks' boundaries (across the one of two), runs of 2 astride, small ones
    lengths = cut([per - 6, per + 11] + [2, 3, 1, 700] * (world * 8), n) if world >= 3 else \
        cut([per - 1, 2, 5, per], n)
    vals = values_for(n, "hash")
    rec, starts = records(lengths, vals)
    np.save(tmp_path / "input.npy", rec)
    ctx = multiprocessing.get_context("spawn")
    q_uid, q_out = ctx.Queue(), ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_process, args=(r, world, transport, port, n, str(tmp_path), q_uid, q_out))
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
    assert all(res[r][2] == plan for r in range(world))  # every rank reports the same plan
    assert plan["total"] == starts.size
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    for op, vt in PROCESS_PAIRS:
        glob = np.zeros(plan["total"], dtype=np.int64)
        for r in range(world):
            glob[plan["bases"][r]:plan["bases"][r] + plan["runs"][r]] = parts[r][f"op{op}"]
        assert np.array_equal(bits_of(glob), model(vals, starts, op, vt)), (op, vt)
    return plan


if not IN_CHILD:
    def test_three_gloo_ranks(lsb_built, tmp_path):
        plan = run_processes(tmp_path, 3, "gloo")
        assert plan["runs"][1] == 0  # rank 1 lies wholly inside the run that crosses both boundaries

    def test_two_rccl_ranks(lsb_built, tmp_path):
        run_processes(tmp_path, 2, "rccl")
