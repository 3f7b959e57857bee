"""A run id per record, host side (no GPU needed): the entry point, the
header, the Python surface, and the id rule of include/lsb.h ("a run id per
record") written out in numpy over lsb_plan_runs' outputs, against the run
index of every record taken from the whole array."""
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lsb.h")).read()


def test_library_exports_the_entry_point(lsb_built):
    lib = lsb_built._lib()
    assert hasattr(lib, "lsb_label_runs")
    # a null context is refused before anything else is looked at
    assert lib.lsb_label_runs(None, 0) == INVALID
    assert lib.lsb_label_runs(None, 7) == INVALID


def test_header_declares_the_call_and_its_modes():
    h = header()
    assert re.search(r"^int\s+lsb_label_runs\(lsb_ctx_t\* ctx, int mode\);", h, re.M)
    assert re.search(r"^#define LSB_LABEL_KEEP\s+0\s*$", h, re.M)
    assert re.search(r"^#define LSB_LABEL_BY_VALUE\s+1\s*$", h, re.M)


def test_python_constants_are_the_headers(lsb_built):
    h = header()
    for name in ("KEEP", "BY_VALUE"):
        want = int(re.search(rf"^#define LSB_LABEL_{name}\s+(\d+)", h, re.M).group(1))
        assert getattr(lsb_built, f"LABEL_{name}") == want
    assert callable(lsb_built.World.label_runs)


def test_unique_and_dense_rank_signatures(lsb_built):
    p = inspect.signature(lsb_built.unique).parameters
    assert "return_inverse" in p and p["return_inverse"].default is False
    d = inspect.signature(lsb_built.dense_rank).parameters
    assert list(d) == ["keys", "descending", "ranks", "radix_bits", "key_type"]
    assert d["descending"].default is False and d["ranks"].default == 1 and d["radix_bits"].default == 8


# ------------------------------------------------------------------ the id rule
def summarise(a, n, P):
    """The [P][4] summary words of the block partition of a: first key, last
    key, heads inside the rank, the smallest head or here."""
    per = -(-n // P)
    s = np.zeros((P, 4), dtype=np.uint64)
    for r in range(P):
        blk = a[r * per: min(n, (r + 1) * per)]
        if blk.size == 0:
            continue
        heads = np.flatnonzero(blk[1:] != blk[:-1]) + 1
        s[r] = (blk[0], blk[-1], heads.size, heads[0] if heads.size else blk.size)
    return s


def ids_by_the_rule(L, a, P):
    """For the record at position i of rank r: bases[r] + (heads of rank r at
    or below i, position 0 counted when head0[r]) - 1."""
    n = a.size
    per = -(-n // P)
    plan = L.plan_runs(n, P, summarise(a, n, P))
    out = []
    for r in range(P):
        blk = a[r * per: min(n, (r + 1) * per)]
        if blk.size == 0:
            continue
        head = np.empty(blk.size, dtype=np.int64)
        head[0] = plan["head0"][r]          # never decided from the records
        head[1:] = blk[1:] != blk[:-1]
        out.append(plan["bases"][r] + np.cumsum(head) - 1)
    return (np.concatenate(out) if out else np.zeros(0, dtype=np.int64)), plan


def check_rule(L, lengths, P):
    lengths = np.asarray(lengths, dtype=np.int64)
    # adjacent runs differ; the keys are not sorted, and need not be
    keys = (np.arange(lengths.size, dtype=np.uint64) % np.uint64(3)) + np.uint64(5)
    a = np.repeat(keys, lengths)
    got, plan = ids_by_the_rule(L, a, P)
    want = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
    assert plan["total"] == lengths.size
    assert np.array_equal(got, want), (lengths.tolist(), P)
    return plan


def test_id_rule_random_partitions(lsb_built):
    rng = np.random.default_rng(11)
    for _ in range(1500):
        P = int(rng.integers(1, 6))
        runs = int(rng.integers(1, 9))
        lengths = rng.integers(1, int(rng.integers(2, 14)), runs)
        check_rule(lsb_built, lengths, P)


def test_id_rule_fixed_cases(lsb_built):
    L = lsb_built
    for P in range(1, 6):
        check_rule(L, [23], P)                       # one key everywhere: ranks 1.. inside the run
        check_rule(L, [1] * 29, P)                   # all distinct
        check_rule(L, [1, 2][:max(1, min(2, P - 2))], P)  # n < P: trailing empty ranks
    # per = 4: the middle rank is exactly one run, then wholly inside one that spills over both ends
    assert check_rule(L, [4, 4, 3], 3)["runs"][1] == 1
    plan = check_rule(L, [3, 6, 2], 3)
    assert plan["runs"][1] == 0 and plan["bases"][1] == plan["bases"][2]
    # per = 3, P = 5: two middle ranks inside one run, a boundary that is also a head, a short last rank
    plan = check_rule(L, [2, 8, 2, 1], 5)
    assert list(plan["runs"][1:3]) == [0, 0]
    # n = 7, P = 5: per = 2, rank 4 is empty
    check_rule(L, [3, 1, 3], 5)
    check_rule(L, [7], 5)
