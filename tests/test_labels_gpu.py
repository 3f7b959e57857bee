"""A run id per record on the device (lsb_label_runs, lsbsort.unique's
inverse, lsbsort.dense_rank; include/lsb.h "a run id per record", DESIGN.md
§7.4).

Inputs are built from run lengths, so the id of every record is known by
construction (np.repeat(arange(runs), lengths)); where no sort is needed they
are loaded with copy_in.  After a sort the model is numpy on the CPU:
np.unique(return_inverse=True) over the encoded keys, the encoding written out
below from the header's table.

As tests/test_runs_gpu.py, the tests run in one child pytest process over this
same file that imports torch before the library is loaded (LSB_LABELS_CHILD=1),
once per session; here each test reports what its namesake did there.  The
tests with real rank processes start their own processes and run from the
pytest process itself.
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

IN_CHILD = os.environ.get("LSB_LABELS_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
INVALID, STATE = 1, 7
KEEP, BY_VALUE = 0, 1
# name -> (LSB_KEY_*, numpy dtype)
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}
REC = np.dtype([("key", "<u8"), ("val", "<u8")])


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("labels") / "child.xml"
    env = dict(os.environ, LSB_LABELS_CHILD="1")
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


def cut(lengths, n):
    """The run lengths cut to n records in all (n >= 1)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    end = np.cumsum(lengths)
    m = int(np.searchsorted(end, n)) + 1
    assert m <= lengths.size, "not enough lengths"
    out = lengths[:m].copy()
    out[-1] -= end[m - 1] - n
    return out


def cycle(pattern, n):
    reps = n // sum(pattern) + 2
    return cut(np.tile(np.asarray(pattern, dtype=np.int64), reps), n)


def from_lengths(lengths):
    """Records whose runs have these lengths, and the run id of each.  Run j's
    key is j times an odd constant (adjacent keys differ; the keys are not
    sorted, and need not be); the value of the record at position i holds i in
    its upper word and 3 i + 5 in its lower one."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    ukeys = (np.arange(lengths.size, dtype=np.uint64) + np.uint64(11)) * np.uint64(0x9E3779B97F4A7C15)
    rec = np.zeros(n, dtype=REC)
    rec["key"] = np.repeat(ukeys, lengths)
    pos = np.arange(n, dtype=np.uint64)
    rec["val"] = (pos << np.uint64(32)) | ((pos * np.uint64(3) + np.uint64(5)) & np.uint64(0xFFFFFFFF))
    return rec, np.repeat(np.arange(lengths.size, dtype=np.uint64), lengths)


def check_labelled(got, rec, ids, mode, what):
    """KEEP: keys unchanged, val == id.  BY_VALUE: key == old value, val == id."""
    assert got.size == rec.size, what
    assert np.array_equal(got["key"], rec["key"] if mode == KEEP else rec["val"]), what
    assert np.array_equal(got["val"], ids), what


# ------------------------------------------------- 1. tile edges, one rank
EDGE_CYCLE = [1, 63, 64, 65, 1, 1023, 1025, 4095, 4097]


def tile_patterns(n):
    return {
        "all distinct": np.ones(n, dtype=np.int64),
        "one value": [n],
        # heads on lane 0 and lane 63, on item, wave and tile edges; runs that span whole tiles
        "cycle": cycle(EDGE_CYCLE, n),
    }


@pytest.mark.parametrize("mode", [KEEP, BY_VALUE])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@torch_first
def test_tile_edges_one_rank(lsb_built, n, mode):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        for name, lengths in tile_patterns(n).items():
            rec, ids = from_lengths(lengths)
            assert rec.size == n
            w.copy_in(0, rec)
            m = int(ids[-1]) + 1
            assert w.count_runs() == {"total": m, "runs": [m], "bases": [0]}, name
            w.label_runs(mode)
            check_labelled(w.copy_out(0), rec, ids, mode, (name, n, mode))


# ------------------------------------------------- 2. more tiles than workgroups
def grid_cap():
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_runs.hip")).read()
    return int(re.search(r"kRunGridCap = (\d+);", src).group(1))


@torch_first
def test_more_tiles_than_workgroups(lsb_built):
    """Every workgroup of k_run_label takes a second tile: n = (grid cap)
    tiles + one tile + 1.  KEEP, then (the keys, so the runs, are the same)
    BY_VALUE over its output: the ids become the keys."""
    L = lsb_built
    cap = grid_cap()
    n = cap * TILE + TILE + 1
    assert n // TILE > cap
    rec, ids = from_lengths(cycle([1, 2, TILE - 1, TILE, TILE + 1, 70001], n))
    m = int(ids[-1]) + 1
    with L.World(n, ranks=1) as w:
        w.copy_in(0, rec)
        assert w.count_runs()["total"] == m
        w.label_runs(KEEP)
        got = w.copy_out(0)
        check_labelled(got, rec, ids, KEEP, "keep")
        assert w.count_runs()["total"] == m
        w.label_runs(BY_VALUE)
        check_labelled(w.copy_out(0), got, ids, BY_VALUE, "by value")


# ------------------------------------------------- 3. rank edges, loopback
def rank_cases(P):
    """(name, lengths) whose sum gives n; per = ceil(n / P)."""
    per = 4099  # odd: ranks 1.. hold blocks aligned to their element only
    n = P * per - 1
    cases = [
        # a run ends at every rank's last slot, the next starts at the first slot: a boundary that is a head
        ("aligned", cut([3, per - 3] * P, n)),
        # one run of 2 astride every boundary
        ("astride", cut([per - 1] + [2, per - 2] * P, n)),
        ("one key", [n]),
        ("cycle", cycle(EDGE_CYCLE, n)),
        ("all distinct", np.ones(n, dtype=np.int64)),
        # n = 7: per = 2 at P = 5 (rank 4 is empty, rank 3 holds one record inside a run that began on rank 2)
        ("seven", [3, 1, 3]),
    ]
    if P >= 3:  # a run over three ranks, the whole middle rank in it; then one ending at a last slot
        cases.append(("three ranks", cut([per - 5, 5 + per + 7, per - 7] + [per] * P, n)))
    return cases


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_rank_edges_loopback(lsb_built, P):
    import torch
    L = lsb_built
    for name, lengths in rank_cases(P):
        rec, ids = from_lengths(lengths)
        n, m = rec.size, int(ids[-1]) + 1
        with L.World(n, ranks=P) as w:
            if name == "seven" and P == 5:
                assert w.here(3) == 1 and w.here(4) == 0
            w.scatter_global(rec)
            plan = w.count_runs()
            assert plan["total"] == m, name
            if name == "three ranks":
                assert plan["runs"][1] == 0 and plan["bases"][1] == plan["bases"][2]
            # where store_runs writes every run's key: the ids index this column
            keys_out = torch.zeros(m, dtype=torch.int64, device="cuda")
            for r in range(P):
                lo, k = plan["bases"][r], plan["runs"][r]
                if k:
                    assert w.store_runs(r, keys=keys_out[lo:lo + k], key_type=0) == k
            keys_out = host(keys_out).view(np.uint64)
            w.label_runs(KEEP)
            got = w.gather_global()
            check_labelled(got, rec, ids, KEEP, (name, P))
            assert np.array_equal(keys_out[got["val"].astype(np.int64)], got["key"]), (name, P)
            # the keys are what they were, so the runs are
            assert w.count_runs() == plan, name
            w.label_runs(BY_VALUE)
            check_labelled(w.gather_global(), got, ids, BY_VALUE, (name, P))


# ------------------------------------------------- 4. through sorts, typed
N = 3 * TILE + 5


@functools.lru_cache(maxsize=None)
def dup_keys(name, n=N):
    """n keys of at most 300 distinct values (about 40 copies each) spread over
    every byte of the type, negative ones included; f64 with both zeros, NaNs
    of both signs and two payloads, and both infinities."""
    kt, dt = KEYS[name]
    v = np.random.default_rng(40 + kt).integers(0, 300, n).astype(np.int64)
    if name == "u64":
        a = v.astype(np.uint64) * np.uint64(0x0040_0100_4001_0011)
    elif name == "i64":
        a = (v - 150) * np.int64(0x0020_0080_2000_8011)
    elif name == "u32":
        a = (v * 0x00D00401 % (1 << 32)).astype(np.uint32)
    elif name == "i32":
        a = ((v - 150) * 0x00680201).astype(np.int32)
    else:
        a = ((v - 150) * 0.37).astype(dt) * np.where(v % 3 == 0, dt(1e20), dt(1.0)).astype(dt)
        if name == "f64":
            b = a.view(np.uint64).copy()
            b[v == 7] = 0x8000000000000000      # -0.0
            b[v == 9] = 0                       # +0.0
            b[v == 11] = 0x7ff8000000000001     # two NaNs that differ in their payload only
            b[v == 13] = 0x7ff8000000000002
            b[v == 15] = 0xfff8000000000001     # a NaN with the sign set
            b[v == 17] = 0x7ff0000000000000     # +inf
            b[v == 19] = 0xfff0000000000000     # -inf
            a = b.view(np.float64)
    a = np.ascontiguousarray(a.astype(dt))
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("radix_bits", [8, 64])
@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("name,descending", [("i64", False), ("f32", True), ("u32", False), ("f64", False)])
@torch_first
def test_through_sorts_typed(lsb_built, name, descending, ranks, radix_bits):
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    keys = dup_keys(name)
    enc = model_encode(bits_of(keys), kt, descending)
    _, idx, inv, cnt = np.unique(enc, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    if name == "f64":  # bit equality: every special value is a key of its own
        special = {0x8000000000000000, 0, 0x7ff8000000000001, 0x7ff8000000000002, 0xfff8000000000001,
                   0x7ff0000000000000, 0xfff0000000000000}
        assert special <= set(bits_of(keys[idx]).tolist())
    # uint32 / uint64 columns travel as tensors of the same width (key_type= names the type)
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)
    dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
    kw = dict(descending=descending, ranks=ranks, radix_bits=radix_bits, key_type=kt)
    uk, ui, uc, ix = L.unique(dk, return_inverse=True, **kw)
    assert ix.dtype == torch.int64 and ix.device == dk.device and ix.shape == dk.shape
    assert np.array_equal(host(ix), inv)
    assert np.array_equal(bits_of(host(uk[ix])), bits_of(keys))  # unique_keys[inverse] is the input, bit for bit
    assert np.array_equal(bits_of(host(dk)), bits_of(keys))      # the input is untouched
    # the first three are what the 3-tuple form returns, which is what it was
    three = L.unique(dk, **kw)
    assert len(three) == 3
    for a, b, want in zip(three, (uk, ui, uc), (keys[idx], idx, cnt)):
        assert np.array_equal(bits_of(host(a)), bits_of(host(b)))
        assert np.array_equal(bits_of(host(a)), bits_of(np.ascontiguousarray(want)))
    dr = L.dense_rank(dk, **kw)
    assert dr.dtype == torch.int64 and dr.device == dk.device
    assert np.array_equal(host(dr), inv)


@pytest.mark.parametrize("ranks", [1, 3])
@torch_first
def test_inverse_against_torch(lsb_built, ranks):
    import torch
    L = lsb_built
    for name in ("i64", "i32"):
        keys = dup_keys(name)
        dk = torch.from_numpy(keys.copy()).cuda()
        uk, _, uc, ix = L.unique(dk, ranks=ranks, return_inverse=True)
        tv, ti, tc = torch.unique(torch.from_numpy(keys.copy()), sorted=True, return_inverse=True, return_counts=True)
        assert np.array_equal(host(uk), tv.numpy()) and np.array_equal(host(uc), tc.numpy()), name
        assert np.array_equal(host(ix), ti.numpy()), name
        assert np.array_equal(host(L.dense_rank(dk, ranks=ranks)), ti.numpy()), name
        # descending: the ranks count from the other end
        assert np.array_equal(host(L.dense_rank(dk, descending=True, ranks=ranks)), tv.numel() - 1 - ti.numpy()), name
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    out = L.unique(e, ranks=ranks, return_inverse=True)
    assert len(out) == 4 and all(t.numel() == 0 for t in out) and out[3].dtype == torch.int64
    assert len(L.unique(e, ranks=ranks)) == 3
    dr = L.dense_rank(e, ranks=ranks)
    assert dr.numel() == 0 and dr.dtype == torch.int64
    with pytest.raises(ValueError):
        L.dense_rank(torch.zeros((4, 4), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("n", [N, 70_001])
@torch_first
def test_second_sort_skips_the_constant_digits(lsb_built, n):
    """The second sort's keys are the indices 0 .. n - 1: at one rank with the
    default options it runs one local pass per byte of n - 1."""
    import torch
    L = lsb_built
    keys = np.random.default_rng(5).integers(-40, 40, n).astype(np.int64)
    dk = torch.from_numpy(keys).cuda()
    inverse = torch.empty(n, dtype=torch.int64, device="cuda")
    with L.World(n, ranks=1) as w:
        w.load_columns(0, dk)
        w.my_sort()
        w.count_runs()
        w.label_runs(BY_VALUE)
        w.my_sort()
        assert w.last_sort()[0] == -(-(n - 1).bit_length() // 8)
        assert np.array_equal(w.copy_out(0)["key"], np.arange(n, dtype=np.uint64))
        w.store_columns(0, None, inverse)
    assert np.array_equal(host(inverse), np.unique(keys, return_inverse=True)[1].reshape(-1))


# ------------------------------------------------- 5. state and refusals
@torch_first
def test_state_and_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = 3 * TILE + 5
    rec, ids = from_lengths(cycle(EDGE_CYCLE, n))
    m = int(ids[-1]) + 1
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, rec)
        col = torch.zeros(m, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def refused(call):
            with pytest.raises(L.LsbError) as e:
                call()
            return e.value.code

        # no plan yet: refused whatever the mode, and nothing has changed
        assert lib.lsb_label_runs(h, KEEP) == STATE and lib.lsb_label_runs(h, BY_VALUE) == STATE
        assert refused(lambda: w.label_runs(KEEP)) == STATE
        assert np.array_equal(w.copy_out(0), rec)
        # an unknown mode: refused before any launch, and the plan is still valid afterwards
        assert w.count_runs()["total"] == m
        for mode in (2, -1, 1 << 20):
            assert lib.lsb_label_runs(h, mode) == INVALID, mode
        assert np.array_equal(w.copy_out(0), rec)
        assert w.store_runs(0, keys=col, key_type=0) == m
        # a label ends both plans
        w.plan_reduce(L.REDUCE_SUM, L.KEY_U64)
        assert w.store_reduce(0, col) == m
        w.label_runs(KEEP)
        labelled = w.copy_out(0)
        check_labelled(labelled, rec, ids, KEEP, "keep")
        assert refused(lambda: w.store_runs(0, keys=col, key_type=0)) == STATE
        assert refused(lambda: w.store_reduce(0, col)) == STATE
        assert refused(lambda: w.plan_reduce(L.REDUCE_SUM, L.KEY_U64)) == STATE
        assert refused(lambda: w.label_runs(KEEP)) == STATE
        assert lib.lsb_label_runs(h, BY_VALUE) == STATE
        assert np.array_equal(w.copy_out(0), labelled)  # the refused calls left the records alone
        # until the runs are counted again: KEEP left the keys, so the total is the same
        assert w.count_runs()["total"] == m
        assert w.store_runs(0, keys=col, key_type=0) == m
        w.label_runs(BY_VALUE)
        check_labelled(w.copy_out(0), labelled, ids, BY_VALUE, "by value")
        assert refused(lambda: w.store_runs(0, keys=col, key_type=0)) == STATE
        # and the context sorts and verifies afterwards
        w.generate()
        w.my_sort()
        assert w.verify() == (True, -1)
    for P in (2, 3):  # n = 0: nothing to label, nothing launched
        with L.World(0, ranks=P) as w:
            assert lib.lsb_label_runs(w._h, KEEP) == STATE
            assert w.count_runs()["total"] == 0
            assert lib.lsb_label_runs(w._h, 2) == INVALID
            w.label_runs(BY_VALUE)


# ------------------------------------------------- 6. real processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_process(rank, world, transport, port, n, result_dir, q_uid, q_out):
    """One rank of a one-rank-per-process world: sort, count, label by value,
    sort again; its block then holds its slice of the inverse."""
    try:
        for p in (ROOT, os.path.join(ROOT, "distributed-lsb_amd")):
            sys.path.insert(0, p)
        if transport == "rccl":  # one "host" per rank: RCCL's socket transport between them
            os.environ["NCCL_HOSTID"] = f"lsb-rank-{rank}"
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
            os.environ.setdefault("NCCL_IB_DISABLE", "1")
        import torch  # noqa: F401  before the library is loaded
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
        w.my_sort()
        plan = w.count_runs()
        w.label_runs(lsbsort.LABEL_BY_VALUE)
        w.my_sort()
        w.sync()
        np.save(os.path.join(result_dir, f"rank{rank}.npy"), w.copy_out(rank))
        w.barrier()
        w.close()
        if transport == "gloo":
            dist.destroy_process_group()
        q_out.put((rank, "ok", plan))
    except Exception as e:  # report, never hang the parent
        q_out.put((rank, repr(e), None))


def run_processes(tmp_path, world, transport):
    """41 records of four keys, shuffled; sorted, a run lies across every rank
    boundary."""
    counts = [9, 12, 11, 9] if world == 3 else [9, 13, 10, 9]
    n = sum(counts)
    per = -(-n // world)
    rng = np.random.default_rng(world)
    rec = np.zeros(n, dtype=REC)
    rec["key"] = rng.permutation(np.repeat(np.array([7, 1 << 40, 3, 1 << 63], dtype=np.uint64), counts))
    rec["val"] = np.arange(n, dtype=np.uint64)
    _, inv, cnt = np.unique(rec["key"], return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert all(r * per not in set(np.cumsum(cnt).tolist()) for r in range(1, world))
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
    assert all(res[r][2] == plan for r in range(world))  # every rank holds the same plan
    assert plan["total"] == len(counts)
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npy")
        lo, hi = r * per, min(n, (r + 1) * per)
        assert np.array_equal(got["key"], np.arange(lo, hi, dtype=np.uint64)), r
        assert np.array_equal(got["val"], inv[lo:hi].astype(np.uint64)), r


if not IN_CHILD:
    def test_three_gloo_ranks(lsb_built, tmp_path):
        run_processes(tmp_path, 3, "gloo")

    def test_two_rccl_ranks(lsb_built, tmp_path):
        run_processes(tmp_path, 2, "rccl")
