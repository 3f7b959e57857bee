"""Runs of equal keys, host side (no GPU needed): the planner lsb_plan_runs
(include/lsb.h, "runs of equal keys") against a brute-force count over the
whole array, and the argument checks that return before any device call."""
import ctypes

import numpy as np
import pytest

INVALID = 1


def summarise(a, n, P):
    """The [P][4] summary words of the block partition of a, from their
    definition: first key, last key, heads inside the rank, the smallest
    head or here."""
    per = -(-n // P) if P else 0
    s = np.zeros((P, 4), dtype=np.uint64)
    for r in range(P):
        blk = a[r * per: min(n, (r + 1) * per)]
        if blk.size == 0:
            continue
        heads = np.flatnonzero(blk[1:] != blk[:-1]) + 1
        s[r] = (blk[0], blk[-1], heads.size, heads[0] if heads.size else blk.size)
    return s


def brute(a, n, P):
    """Every run of the whole array, given to the rank that holds its first
    record; ends[r]: one past the run that holds r's last record."""
    per = -(-n // P) if P else 0
    starts = [i for i in range(n) if i == 0 or a[i] != a[i - 1]]
    run_end = {s: e for s, e in zip(starts, starts[1:] + [n])}
    runs, bases, ends, head0 = [0] * P, [0] * P, [0] * P, [0] * P
    for s in starts:
        runs[s // per] += 1
    acc = 0
    for r in range(P):
        here = max(0, min(n, (r + 1) * per) - r * per)
        if here == 0:
            continue
        bases[r] = acc
        acc += runs[r]
        head0[r] = int(r * per in run_end)
        last = r * per + here - 1
        ends[r] = run_end[max(s for s in starts if s <= last)]
    return {"runs": runs, "bases": bases, "ends": ends, "head0": head0, "total": len(starts)}


def check(L, a, P):
    a = np.asarray(a, dtype=np.uint64)
    n = a.size
    got = L.plan_runs(n, P, summarise(a, n, P))
    want = brute(a, n, P)
    for k in ("runs", "bases", "ends", "head0"):
        assert list(got[k]) == want[k], (k, a.tolist(), P)
    assert got["total"] == want["total"], (a.tolist(), P)


def test_planner_against_brute_force_random(lsb_built):
    rng = np.random.default_rng(7)
    for _ in range(4000):
        n = int(rng.integers(0, 61))
        P = int(rng.integers(1, 9))
        a = rng.integers(0, int(rng.integers(1, 6)), n).astype(np.uint64)
        if rng.integers(0, 2):
            a.sort()
        check(lsb_built, a, P)


def test_planner_fixed_cases(lsb_built):
    L = lsb_built
    for P in range(1, 9):
        check(L, [], P)                                  # n = 0
        check(L, [5, 5, 9][:min(3, P - 1)], P)           # n < P: trailing empty ranks
        check(L, [3] * 23, P)                            # one key everywhere
        check(L, np.arange(29), P)                       # all distinct
    # per = 4: a run covering exactly the whole middle rank, one spilling over both its ends
    check(L, [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3], 3)
    check(L, [1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3], 3)
    check(L, [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3], 4)
    # a run ending exactly at a rank's last slot, the next starting at the first slot
    check(L, [1, 1, 2, 2, 3, 3, 3, 3, 4], 3)
    # unsorted: the same key on both sides of a run of another
    check(L, [7, 7, 1, 7, 7, 7, 1, 1, 7], 3)
    # the extremes of the key range
    check(L, [0, 0, 2**64 - 1, 2**64 - 1, 2**64 - 1, 0], 2)


def test_planner_refuses_impossible_summaries(lsb_built):
    L = lsb_built
    n, P = 12, 3  # here = 4 on every rank
    good = summarise(np.array([1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 4, 4], dtype=np.uint64), n, P)
    assert L.plan_runs(n, P, good)["total"] == 4

    def bad(r, **words):
        s = good.copy()
        for k, v in words.items():
            s[r, {"first": 0, "last": 1, "inner": 2, "lead": 3}[k]] = v
        with pytest.raises(L.LsbError) as e:
            L.plan_runs(n, P, s)
        assert e.value.code == INVALID, words

    for r in range(P):
        bad(r, lead=0)                       # lead < 1
        bad(r, lead=5)                       # lead > here
        bad(r, lead=2**64 - 1)
        bad(r, inner=4)                      # inner > here - 1
        bad(r, inner=2**63)
    bad(0, inner=0)                          # inner == 0 but lead < here
    bad(0, lead=4)                           # lead == here but inner > 0
    bad(1, first=9)                        # inner == 0 && first != last


def test_planner_refuses_null_and_bad_arguments(lsb_built):
    lib = lsb_built._lib()
    P = 2
    s = np.zeros((P, 4), dtype=np.uint64)
    s[:, 3] = 1
    i32 = np.zeros(P, dtype=np.intc)
    a, b, c = (np.zeros(P, dtype=np.int64) for _ in range(3))
    t = ctypes.c_int64()
    args = [2, P, s.ctypes.data, i32.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, ctypes.byref(t)]
    assert lib.lsb_plan_runs(*args) == 0
    for i in range(2, 8):
        broken = list(args)
        broken[i] = None
        assert lib.lsb_plan_runs(*broken) == INVALID, i
    assert lib.lsb_plan_runs(-1, *args[1:]) == INVALID
    assert lib.lsb_plan_runs(2, 0, *args[2:]) == INVALID
    assert lib.lsb_plan_runs(2, 65, *args[2:]) == INVALID


def test_entry_points_refuse_a_null_context(lsb_built):
    lib = lsb_built._lib()
    t = ctypes.c_int64(-5)
    assert lib.lsb_count_runs(None, ctypes.byref(t), None, None) == INVALID
    assert lib.lsb_count_runs(None, None, None, None) == INVALID
    assert lib.lsb_store_runs(None, 0, 4, None, 0, 0, None, None, None, 0, ctypes.byref(t)) == INVALID
    assert lib.lsb_store_runs(None, -1, -1, None, 6, 2, None, None, None, 3, None) == INVALID
    assert t.value == -5
