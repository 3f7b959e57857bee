"""The select, host side (no GPU needed): the planner lsb_plan_select
(include/lsb.h, "the k-th key and the first k + 1 records") against a numpy
derivation from the stable argsort of the whole array, its refusals, and the
argument checks that return before any device call."""
import ctypes

import numpy as np
import pytest

INVALID = 1


def derive(a, P, k):
    """From the definition: the first k + 1 records of the stable sort of a,
    counted per rank of the block partition -> (below, equal, take, bases)."""
    n = a.size
    per = -(-n // P)
    order = np.argsort(a, kind="stable")
    pivot = a[order[k]]
    rank_of = np.arange(n) // per
    below = np.bincount(rank_of[a < pivot], minlength=P)[:P]
    equal = np.bincount(rank_of[a == pivot], minlength=P)[:P]
    take = np.bincount(rank_of[order[:k + 1]], minlength=P)[:P]
    bases = np.concatenate([[0], np.cumsum(take)[:-1]])
    return below.astype(np.int64), equal.astype(np.int64), take.astype(np.int64), bases.astype(np.int64)


def check(L, a, P, k):
    a = np.asarray(a, dtype=np.uint64)
    below, equal, take, bases = derive(a, P, k)
    got = L.plan_select(a.size, P, k + 1, below, equal)
    assert np.array_equal(got["take"], take), (a.tolist(), P, k)
    assert np.array_equal(got["bases"], bases), (a.tolist(), P, k)
    assert got["take"].sum() == k + 1
    assert np.array_equal(got["bases"], np.concatenate([[0], np.cumsum(got["take"])[:-1]]))


def tie_edges(a):
    """Both edges of every group of equal keys, as positions of the sort."""
    s = np.sort(a)
    heads = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return sorted(set(heads.tolist()) | set((np.concatenate([heads[1:], [s.size]]) - 1).tolist()))


def test_planner_against_numpy_random(lsb_built):
    rng = np.random.default_rng(11)
    for it in range(400):
        n = int(rng.integers(1, 60))
        P = int(rng.integers(1, 9))
        a = rng.integers(0, int(rng.integers(1, 6)), n).astype(np.uint64)
        for k in sorted({0, n - 1, n // 2, int(rng.integers(0, n))} | set(tie_edges(a))):
            check(lsb_built, a, P, k)


@pytest.mark.parametrize("P", [1, 2, 3, 7, 33, 64])
def test_planner_every_rank_count(lsb_built, P):
    rng = np.random.default_rng(P)
    for n in (1, P, 4 * P + 3, 6):  # n = 6 with P = 5 or more: trailing empty ranks
        a = rng.integers(0, 4, n).astype(np.uint64)
        for k in sorted({0, n - 1, n // 2} | set(tie_edges(a))):
            check(lsb_built, a, P, k)


def test_pivot_group_over_whole_middle_ranks(lsb_built):
    L = lsb_built
    P, per = 5, 7
    n = P * per - 2  # the last rank is short
    a = np.full(n, 9, dtype=np.uint64)
    a[:3] = [1, 2, 3]        # below the pivot, on rank 0
    a[-4:] = [20, 21, 5, 9]  # rank 4: two above, one below, one equal
    s = np.sort(a)
    lo, hi = int(np.searchsorted(s, 9, "left")), int(np.searchsorted(s, 9, "right")) - 1
    assert lo == 4 and hi == n - 3
    for k in (lo, lo + 1, lo + per, lo + 2 * per + 3, hi - 1, hi):  # both ends of the bracket and inside it
        check(L, a, P, k)
    below, equal, take, _ = derive(a, P, lo + 2 * per)
    assert list(equal[1:4]) == [per] * 3  # ranks 1 to 3 lie wholly inside the pivot group
    assert take[1] == per and 0 < take[2] < per and take[3] == 0 and take[4] == 1


def test_trailing_empty_ranks(lsb_built):
    a = np.array([3, 1, 3, 3, 0, 3], dtype=np.uint64)  # n = 6, P = 5: per = 2, ranks 3 and 4 are empty
    for k in range(6):
        check(lsb_built, a, 5, k)
    got = lsb_built.plan_select(6, 5, 6, *derive(a, 5, 5)[:2])
    assert list(got["take"]) == [2, 2, 2, 0, 0] and list(got["bases"]) == [0, 2, 4, 6, 6]


def test_planner_refusals(lsb_built):
    L = lsb_built
    lib = L._lib()
    n, P = 10, 3  # here = 4, 4, 2
    below = np.array([1, 2, 0], dtype=np.int64)
    equal = np.array([2, 1, 2], dtype=np.int64)
    take, bases = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)

    def call(n=n, P=P, count=5, b=below, e=equal, t=take, s=bases):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.lsb_plan_select(n, P, count, ptr(b), ptr(e), ptr(t), ptr(s))

    assert call() == 0 and list(take) == [3, 2, 0] and list(bases) == [0, 3, 5]
    # both ends of the bracket: sum(below) = 3 < count <= 3 + 5
    assert call(count=4) == 0 and list(take) == [2, 2, 0]
    assert call(count=8) == 0 and list(take) == [3, 3, 2] and list(bases) == [0, 3, 6]
    assert call(count=3) == INVALID and call(count=9) == INVALID and call(count=0) == INVALID
    for name in "best":
        assert call(**{name: None}) == INVALID, name
    assert call(n=-1) == INVALID and call(P=0) == INVALID and call(P=65) == INVALID
    for arr, r in ((below, 0), (equal, 2)):
        bad = arr.copy()
        bad[r] = -1
        assert call(**({"b": bad} if arr is below else {"e": bad})) == INVALID
    assert call(b=np.array([1, 2, 1], dtype=np.int64)) == INVALID      # rank 2 holds 2 records, not 1 + 2
    assert call(e=np.array([4, 1, 2], dtype=np.int64)) == INVALID      # rank 0 holds 4, not 1 + 4
    assert call(b=np.array([1 << 62, 2, 0], dtype=np.int64)) == INVALID
    with pytest.raises(L.LsbError) as e:
        L.plan_select(n, P, 9, below, equal)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        L.plan_select(n, P, 5, below[:2], equal)


def test_error_codes_without_device(lsb_built):
    lib = lsb_built._lib()
    key, cnt = ctypes.c_uint64(5), ctypes.c_int64(-5)
    assert lib.lsb_select(None, 0, ctypes.byref(key), None, None, None, None) == INVALID and key.value == 5
    col = np.arange(4, dtype=np.uint64)  # host memory: never reaches a device call with a null context
    assert lib.lsb_store_select(None, 0, 4, col.ctypes.data, 0, 0, col.ctypes.data, 8, ctypes.byref(cnt)) == INVALID
    assert cnt.value == -5
    assert lib.lsb_store_select(None, -1, -1, None, 6, 2, None, 3, None) == INVALID
    assert lib.lsb_get_last_select(None, None, None) == INVALID
