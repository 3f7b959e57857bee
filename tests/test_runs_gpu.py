"""Runs of equal keys on the device (lsb_count_runs / lsb_store_runs,
lsbsort.unique; include/lsb.h "runs of equal keys").

Inputs are built from run lengths, so the expected keys, starts, counts and
first values are known by construction; where no sort is needed they are
loaded with copy_in.  After a sort the model is numpy on the CPU: np.unique
over the encoded keys, the encoding written out below from the header's table.

The outputs are torch CUDA tensors, so (as tests/test_columns_gpu.py) the
tests run in one child pytest process over this same file that imports torch
before the library is loaded (LSB_RUNS_CHILD=1), once per session; here each
test reports what its namesake did there.  The tests with real rank processes
start their own processes and run from the pytest process itself.
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

IN_CHILD = os.environ.get("LSB_RUNS_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
INVALID, STATE = 1, 7
SENT = 0x5555555555555555
# name -> (LSB_KEY_*, numpy dtype)
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("runs") / "child.xml"
    env = dict(os.environ, LSB_RUNS_CHILD="1")
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


def geometric(mean, n, seed):
    rng = np.random.default_rng(seed)
    return cut(rng.geometric(1.0 / mean, n // mean * 2 + 64), n)


def from_lengths(lengths):
    """Records whose runs have these lengths, and what the library must say
    about them.  Run j's key is j times an odd constant (adjacent keys differ;
    the keys are not sorted, and need not be); the value of the record at
    position i holds i in its upper word and 3 i + 5 in its lower one."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    ukeys = (np.arange(lengths.size, dtype=np.uint64) + np.uint64(11)) * np.uint64(0x9E3779B97F4A7C15)
    rec = np.zeros(n, dtype=[("key", "<u8"), ("val", "<u8")])
    rec["key"] = np.repeat(ukeys, lengths)
    pos = np.arange(n, dtype=np.uint64)
    rec["val"] = (pos << np.uint64(32)) | ((pos * np.uint64(3) + np.uint64(5)) & np.uint64(0xFFFFFFFF))
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    return rec, {"keys": ukeys, "starts": starts, "counts": lengths, "firsts": rec["val"][starts]}


def store(w, rank, m, outputs=("keys", "starts", "counts", "firsts"), val_bytes=8, key_type=0, key_np=np.int64,
          descending=False):
    """store_runs of `rank` into fresh columns of m elements, each with two
    sentinel elements on either side that must survive -> {name: numpy}."""
    import torch
    dts = {"keys": key_np, "starts": np.int64, "counts": np.int64, "firsts": np.int64 if val_bytes == 8 else np.int32}
    sent = {k: np.frombuffer(b"\x55" * ((m + 4) * np.dtype(dts[k]).itemsize), dtype=dts[k]).copy() for k in outputs}
    full = {k: torch.from_numpy(v.copy()).cuda() for k, v in sent.items()}
    got = w.store_runs(rank, **{k: full[k][2:2 + m] for k in outputs}, key_type=key_type, descending=descending)
    assert got == m
    out = {}
    for k, t in full.items():
        h = host(t)
        assert np.array_equal(bits_of(h[:2]), bits_of(sent[k][:2])), k
        assert np.array_equal(bits_of(h[2 + m:]), bits_of(sent[k][2 + m:])), k
        out[k] = h[2:2 + m]
    return out


def check_outputs(got, want, val_bytes=8, what=None):
    for k, v in got.items():
        w_ = want[k]
        if k == "firsts" and val_bytes == 4:
            w_ = w_ & np.uint64(0xFFFFFFFF)
        assert np.array_equal(bits_of(v), bits_of(np.ascontiguousarray(w_))), (k, what)


# ------------------------------------------------- 1. tile edges, one rank
def tile_patterns(n):
    k = n // TILE + 2
    return {
        "all equal": [n],
        "all distinct": np.ones(n, dtype=np.int64),
        "heads at 4096k": cut([TILE] * k, n),
        "heads at 4096k-1": cut([TILE - 1] + [TILE] * k, n),
        "heads at 4096k+1": cut([TILE + 1] + [TILE] * k, n),
        "geometric 3": geometric(3, n, 1),
        "geometric 700": geometric(700, n, 2),
    }


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@torch_first
def test_tile_edges_one_rank(lsb_built, n):
    L = lsb_built
    with L.World(n, ranks=1) as w:
        for name, lengths in tile_patterns(n).items():
            rec, want = from_lengths(lengths)
            assert rec.size == n
            w.copy_in(0, rec)
            m = want["keys"].size
            assert w.count_runs() == {"total": m, "runs": [m], "bases": [0]}, name
            check_outputs(store(w, 0, m), want, what=(name, "all outputs"))
            check_outputs(store(w, 0, m, val_bytes=4), want, val_bytes=4, what=(name, "4-byte firsts"))
            for outs in (("keys",), ("starts",), ("starts", "counts"), ("firsts",)):
                check_outputs(store(w, 0, m, outputs=outs), want, what=(name, outs))
            # a column longer than the runs takes them at its start
            import torch
            big = torch.full((m + 7,), SENT, dtype=torch.int64, device="cuda")
            assert w.store_runs(0, starts=big, key_type=0) == m
            assert np.array_equal(host(big)[:m], want["starts"]) and np.all(host(big)[m:] == SENT), name


# ------------------------------------------------- 2. more tiles than workgroups and scan threads
def launcher_constants():
    src = open(os.path.join(ROOT, "distributed-lsb_amd", "csrc", "lsb_runs.hip")).read()
    return (int(re.search(r"kRunGridCap = (\d+);", src).group(1)),
            int(re.search(r"kRunScanBlock = (\d+);", src).group(1)))


@torch_first
def test_more_tiles_than_workgroups(lsb_built):
    """Every workgroup of k_run_count and k_run_write takes a second tile, and
    every thread of k_run_scan several: n = (grid cap) tiles + one tile + 1."""
    L = lsb_built
    grid_cap, scan_block = launcher_constants()
    n = grid_cap * TILE + TILE + 1
    assert n // TILE > grid_cap and n // TILE > scan_block
    rec, want = from_lengths(cycle([1, 2, TILE - 1, TILE, TILE + 1, 70001], n))
    m = want["keys"].size
    with L.World(n, ranks=1) as w:
        w.copy_in(0, rec)
        assert w.count_runs() == {"total": m, "runs": [m], "bases": [0]}
        check_outputs(store(w, 0, m), want)


# ------------------------------------------------- 3. rank edges, loopback
def rank_cases(P):
    """(name, lengths) whose sum gives n; per = ceil(n / P)."""
    per = 4099  # odd: ranks 1.. hold blocks aligned to their element only
    n = P * per - 1
    cases = [
        # a run ends at every rank's last slot, the next starts at the first slot
        ("aligned", cut([3, per - 3] * P, n)),
        # records before and after each boundary differ only in value: one run of 2 astride it
        ("astride", cut([per - 1] + [2, per - 2] * P, n)),
        ("one key", [n]),
        ("geometric 700", geometric(700, n, 3 + P)),
        ("all distinct", np.ones(n, dtype=np.int64)),
    ]
    if P >= 3:  # a run over three ranks, the whole middle rank in it; then one ending at a last slot
        cases.append(("three ranks", cut([per - 5, 5 + per + 7, per - 7] + [per] * P, n)))
    return cases


def check_world(L, P, rec, want, name):
    n = rec.size
    with L.World(n, ranks=P) as w:
        w.scatter_global(rec)
        plan = w.count_runs()
        owner = want["starts"] // max(w.per, 1)
        runs = [int(np.count_nonzero(owner == r)) for r in range(P)]
        assert plan["total"] == want["keys"].size and plan["runs"] == runs, name
        assert plan["bases"] == [int(sum(runs[:r])) if w.here(r) else 0 for r in range(P)], name
        parts = [store(w, r, runs[r]) for r in range(P)]
        for k in ("keys", "starts", "counts", "firsts"):
            # the ranks' outputs, laid end to end by bases, are the global answer
            glob = np.zeros(plan["total"], dtype=parts[0][k].dtype)
            for r in range(P):
                glob[plan["bases"][r]:plan["bases"][r] + runs[r]] = parts[r][k]
            assert np.array_equal(bits_of(glob), bits_of(np.ascontiguousarray(want[k]))), (name, k)
    return plan


@pytest.mark.parametrize("P", [2, 3, 5])
@torch_first
def test_rank_edges_loopback(lsb_built, P):
    for name, lengths in rank_cases(P):
        rec, want = from_lengths(lengths)
        assert -(-rec.size // P) % 2 == 1
        plan = check_world(lsb_built, P, rec, want, name)
        if name == "one key":
            assert plan["runs"] == [1] + [0] * (P - 1)
        if name == "three ranks":
            assert plan["runs"][1] == 0
    # n < P: empty ranks
    for lengths in ([1], [2], [1, 1], [1, 2], [2, 2]):
        if sum(lengths) < P:
            rec, want = from_lengths(lengths)
            check_world(lsb_built, P, rec, want, ("n < P", lengths))
    with lsb_built.World(0, ranks=P) as w:
        assert w.count_runs() == {"total": 0, "runs": [0] * P, "bases": [0] * P}


# ------------------------------------------------- 4. through a sort, typed
N = 300_007


@functools.lru_cache(maxsize=None)
def tie_keys(name, n=N):
    """n keys of at most 2^12 distinct values spread over every byte of the
    type, negative ones included; f32 without NaN and -0.0, f64 with both
    zeros and NaNs of two payloads."""
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
        if name == "f64":
            b = a.view(np.uint64).copy()
            b[v == 7] = 0x8000000000000000      # -0.0
            b[v == 9] = 0                       # +0.0
            b[v == 11] = 0x7ff8000000000001     # two NaNs that differ in their payload only
            b[v == 13] = 0x7ff8000000000002
            a = b.view(np.float64)
    a = np.ascontiguousarray(a.astype(dt))
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("radix_bits", [8, 64])
@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("name,descending", [("i64", False), ("f32", True), ("u32", False), ("f64", False)])
@torch_first
def test_through_a_sort_typed(lsb_built, name, descending, ranks, radix_bits):
    import torch
    L = lsb_built
    kt, dt = KEYS[name]
    keys = tie_keys(name)
    enc = model_encode(bits_of(keys), kt, descending)
    _, idx, cnt = np.unique(enc, return_index=True, return_counts=True)
    want = {"keys": keys[idx], "starts": np.concatenate([[0], np.cumsum(cnt)[:-1]]), "counts": cnt, "firsts": idx}
    if name == "f64":  # bit equality: both zeros and both NaNs are keys of their own
        assert {0x8000000000000000, 0, 0x7ff8000000000001, 0x7ff8000000000002} <= set(bits_of(want["keys"]).tolist())
    # uint32 / uint64 columns travel as tensors of the same width (key_type= names the type)
    key_np = {"u64": np.int64, "u32": np.int32}.get(name, dt)
    dk = torch.from_numpy(keys.view(key_np).copy()).cuda()
    with L.World(N, ranks=ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            w.load_columns(r, dk[lo:lo + h], None, descending=descending, key_type=kt)
        w.my_sort()
        plan = w.count_runs()
        assert plan["total"] == idx.size and sum(plan["runs"]) == idx.size
        parts = [store(w, r, plan["runs"][r], key_type=kt, key_np=key_np, descending=descending)
                 for r in range(ranks)]
    for k in ("keys", "starts", "counts", "firsts"):
        glob = np.concatenate([p[k] for p in parts])  # bases are the prefix sums of runs
        assert np.array_equal(bits_of(glob), bits_of(np.ascontiguousarray(want[k]))), k
    assert plan["bases"] == [int(sum(plan["runs"][:r])) for r in range(ranks)]


@pytest.mark.parametrize("ranks", [1, 3])
@torch_first
def test_unique_against_torch(lsb_built, ranks):
    import torch
    L = lsb_built
    for name in ("i64", "i32", "f32"):
        keys = tie_keys(name)[:50_001]
        dk = torch.from_numpy(keys.copy()).cuda()
        uk, ui, uc = L.unique(dk, ranks=ranks)
        tv, tc = torch.unique(torch.from_numpy(keys.copy()), sorted=True, return_counts=True)
        _, idx = np.unique(keys, return_index=True)
        assert uk.dtype == dk.dtype and ui.dtype == torch.int64 and uc.dtype == torch.int64
        assert uk.device == dk.device and ui.device == dk.device and uc.device == dk.device
        assert np.array_equal(bits_of(host(uk)), bits_of(tv.numpy())), name
        assert np.array_equal(host(uc), tc.numpy()) and np.array_equal(host(ui), idx), name
        assert np.array_equal(bits_of(host(dk)), bits_of(keys))  # the input is untouched
        dk_, di_, dc_ = L.unique(dk, descending=True, ranks=ranks)
        assert np.array_equal(bits_of(host(dk_)), bits_of(tv.numpy()[::-1].copy())), name
        assert np.array_equal(host(dc_), tc.numpy()[::-1]) and np.array_equal(host(di_), idx[::-1]), name
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    uk, ui, uc = L.unique(e, ranks=ranks)
    assert uk.numel() == ui.numel() == uc.numel() == 0
    assert uk.dtype == torch.float32 and ui.dtype == torch.int64 and uc.dtype == torch.int64
    with pytest.raises(ValueError):
        L.unique(torch.zeros((4, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        L.unique(torch.zeros(10, dtype=torch.int16, device="cuda"))


# ------------------------------------------------- 5. state and refusals
@torch_first
def test_state_and_refusals(lsb_built):
    import torch
    L = lsb_built
    lib = L._lib()
    n = (1 << 20) + (1 << 18)
    rec, want = from_lengths(geometric(700, n, 9))
    m = want["keys"].size
    with L.World(n, ranks=1) as w:
        h = w._h
        w.copy_in(0, rec)
        cols = {k: torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda") for k in "ksf"}
        kp, sp, fp = (cols[k].data_ptr() for k in "ksf")
        small = torch.zeros(16, dtype=torch.int64, device="cuda")
        host_arr = np.full(m, SENT, dtype=np.uint64)
        torch.cuda.synchronize()
        runs = ctypes.c_int64(-1)

        def call(cap=m, keys=kp, kt=0, flags=0, starts=sp, counts=None, firsts=fp, vb=8):
            runs.value = -1
            return lib.lsb_store_runs(h, 0, cap, keys, kt, flags, starts, counts, firsts, vb, ctypes.byref(runs))

        def untouched():
            torch.cuda.synchronize()
            return all(bool((t == SENT).all()) for t in cols.values()) and bool(np.all(host_arr == SENT))

        # no plan yet, and none after anything that can change A
        assert call() == STATE
        changes = [("my_sort", w.my_sort), ("copy_in", lambda: w.copy_in(0, rec[:5], off=3)),
                   ("load_columns", lambda: w.load_columns(0, small, key_type=0)), ("generate", w.generate),
                   ("global_shuffle", lambda: w.global_shuffle(0))]
        for what, change in changes:
            w.count_runs()
            change()
            assert call() == STATE and untouched(), what
            with pytest.raises(L.LsbError) as e:
                w.store_runs(0, starts=cols["s"], key_type=0)
            assert e.value.code == STATE, what
        w.copy_in(0, rec)
        assert w.count_runs()["total"] == m
        refusals = [
            ("cap one short", lambda: call(cap=m - 1)),
            ("negative cap", lambda: call(cap=-1)),
            ("rank", lambda: lib.lsb_store_runs(h, 1, m, kp, 0, 0, sp, None, fp, 8, None)),
            ("counts without starts", lambda: call(starts=None, counts=sp)),
            ("no output", lambda: call(keys=None, starts=None, firsts=None, vb=0)),
            ("key type 6", lambda: call(kt=6)),
            ("flags 2", lambda: call(flags=2)),
            ("val_bytes 3", lambda: call(vb=3)),
            ("val_bytes 8, no firsts", lambda: call(firsts=None)),
            ("val_bytes 0 with firsts", lambda: call(vb=0)),
            ("host keys", lambda: call(keys=host_arr.ctypes.data)),
            ("host firsts", lambda: call(firsts=host_arr.ctypes.data)),
            ("starts off by 4 bytes", lambda: call(cap=m, starts=sp + 4)),
            ("32-bit keys off by 2 bytes", lambda: call(keys=kp + 2, kt=4)),
            ("4-byte firsts off by 2 bytes", lambda: call(firsts=fp + 2, vb=4)),
            ("counts are starts", lambda: call(counts=sp)),
            ("firsts are keys", lambda: call(firsts=kp)),
            ("starts overlap keys by one element", lambda: call(cap=m, starts=kp + 8 * (m - 1) if m > 1 else kp,
                                                                 keys=kp, firsts=None, vb=0)),
            ("keys leave their allocation", lambda: call(cap=1 << 40, starts=None, firsts=None, vb=0)),
            ("starts leave their allocation", lambda: call(cap=1 << 40, keys=None, counts=kp, firsts=None, vb=0)),
            ("firsts leave their allocation", lambda: call(cap=1 << 40, keys=None, starts=None)),
        ]
        for what, bad in refusals:
            assert bad() == INVALID and untouched(), what
            if what == "cap one short":
                assert runs.value == m
        with pytest.raises(ValueError):
            w.store_runs(0, counts=cols["s"], key_type=0)
        with pytest.raises(ValueError):
            w.store_runs(0)
        # the plan survived every refusal
        check_outputs(store(w, 0, m), want)
        # and the context sorts and verifies afterwards
        w.generate()
        w.my_sort()
        assert w.verify() == (True, -1)
        assert w.count_runs()["total"] == n  # 2^64 keys, 1.3 M draws: all distinct


# ------------------------------------------------- 6. real processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_process(rank, world, transport, port, n, result_dir, q_uid, q_out):
    """One rank of a one-rank-per-process world: count, then store its runs
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
        w.copy_in(rank, rec[rank * w.per: rank * w.per + w.here(rank)])
        w.barrier()
        plan = w.count_runs()
        m = plan["runs"][rank]
        cols = {k: torch.full((m + 2,), SENT, dtype=torch.int64, device="cuda") for k in
                ("keys", "starts", "counts", "firsts")}
        got = w.store_runs(rank, **{k: t[1:1 + m] for k, t in cols.items()}, key_type=0)
        out = {k: t.cpu().numpy() for k, t in cols.items()}
        ok = got == m and all(o[0] == SENT and o[-1] == SENT for o in out.values())
        np.savez(os.path.join(result_dir, f"rank{rank}.npz"), **{k: o[1:1 + m] for k, o in out.items()})
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
    rec, want = from_lengths(lengths)
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
    assert plan["total"] == want["keys"].size
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    for k in ("keys", "starts", "counts", "firsts"):
        glob = np.zeros(plan["total"], dtype=np.int64)
        for r in range(world):
            glob[plan["bases"][r]:plan["bases"][r] + plan["runs"][r]] = parts[r][k]
        assert np.array_equal(bits_of(glob), bits_of(np.ascontiguousarray(want[k]))), k
    return plan


if not IN_CHILD:
    def test_three_gloo_ranks(lsb_built, tmp_path):
        plan = run_processes(tmp_path, 3, "gloo")
        assert plan["runs"][1] == 0  # rank 1 lies inside the run that crosses both boundaries

    def test_two_rccl_ranks(lsb_built, tmp_path):
        run_processes(tmp_path, 2, "rccl")
