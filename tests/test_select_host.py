"""The select, host side (no GPU needed): the planner lsb_plan_select
(include/lsb.h, "the k-th key and the first k + 1 records") against a numpy
derivation from the stable argsort of the whole array, its refusals, and the
argument checks that return before any device call; and the model of the
select's rounds and of its compaction's flushes (tests/select_model.py) against
the same argsort, with the conditions the compaction's inputs must meet."""
import ctypes
import functools

import numpy as np
import pytest

import select_model as M

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


# ------------------------------------------------- the model of the rounds
class Sorted:
    """The stable argsort of an array, once, and derive()'s answers from it
    (one rank: the stable sort itself, every count is the whole array's)."""

    def __init__(self, a, P):
        self.a, self.P = np.ascontiguousarray(a, dtype=np.uint64), P
        if P == 1:
            self.sorted = np.sort(self.a, kind="stable")
            return
        self.order = np.argsort(self.a, kind="stable")
        self.sorted = self.a[self.order]
        self.rank_of = np.arange(self.a.size) // -(-self.a.size // P)

    def at(self, k):
        """-> (pivot, below[P], equal[P], take[P], bases[P])."""
        pivot, P = self.sorted[k], self.P
        lo = int(np.searchsorted(self.sorted, pivot, "left"))
        hi = int(np.searchsorted(self.sorted, pivot, "right"))
        if P == 1:
            return int(pivot), np.array([lo]), np.array([hi - lo]), np.array([k + 1]), np.array([0])
        below = np.bincount(self.rank_of[self.order[:lo]], minlength=P)[:P]
        equal = np.bincount(self.rank_of[self.order[lo:hi]], minlength=P)[:P]
        take = below + np.bincount(self.rank_of[self.order[lo:k + 1]], minlength=P)[:P]
        return int(pivot), below, equal, take, np.concatenate([[0], np.cumsum(take)[:-1]])


def check_model(L, srt, k):
    """round_model(k) against the stable sort -> the model's answer."""
    pivot, below, equal, take, bases = srt.at(k)
    m = M.round_model(srt.a, srt.P, k)
    what = (srt.a.size, srt.P, k)
    assert m.pivot == pivot and sum(m.below) == below.sum() and sum(m.equal) == equal.sum(), what
    got = L.plan_select(srt.a.size, srt.P, k + 1, np.asarray(m.below), np.asarray(m.equal))
    want = L.plan_select(srt.a.size, srt.P, k + 1, below, equal)
    assert np.array_equal(got["take"], want["take"]) and np.array_equal(got["bases"], want["bases"]), what
    assert np.array_equal(got["take"], take) and np.array_equal(got["bases"], bases), what
    assert np.array_equal(m.below, below) and np.array_equal(m.equal, equal), what
    # what the rounds read: every rank at least its own records once, never more than a read per round
    assert m.rounds == len(m.trace) and 1 <= m.rounds <= 8
    assert all(M.here_of(srt.a.size, srt.P, r) <= m.read[r] <= m.rounds * M.here_of(srt.a.size, srt.P, r)
               for r in range(srt.P)), what
    return m


def test_geometry_read_from_the_sources():
    tile, block, stage, cap = M.geometry()
    assert tile % block == 0 and block % 64 == 0 and 64 <= stage <= tile and cap >= 1
    assert tile == 4096  # the inputs below are written in tiles of this size


def test_round_model_against_numpy_random(lsb_built):
    rng = np.random.default_rng(75)
    for it in range(300):
        n = int(rng.integers(1, 301))
        P = int(rng.integers(1, 6))
        kind = it % 3
        if kind == 0:    # heavy ties
            a = rng.integers(0, int(rng.integers(1, 6)), n).astype(np.uint64) << np.uint64(8 * int(rng.integers(0, 8)))
        elif kind == 1:  # constant bytes between varying ones
            a = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(np.uint64)
            a &= np.uint64(int(rng.choice([0xFF00FF00FF00FF00, 0x00FF0000FFFF00FF, 0xFF000000000000FF, 0x0000FFFF00000000])))
            a |= np.uint64(0x0011002200330044)
        else:            # a few values among distinct ones
            a = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64)
            a[rng.random(n) < 0.5] = a[0]
        srt = Sorted(a, P)
        for k in sorted({0, n - 1, n // 2, int(rng.integers(0, n))} | set(tie_edges(a)[:6])):
            check_model(lsb_built, srt, k)


@functools.lru_cache(maxsize=None)
def chain(layout):
    return Sorted(M.chain_keys(layout), 1)


@pytest.mark.parametrize("layout", ["sorted", "shuffled", "one_over"])
def test_chain_model_and_conditions(lsb_built, layout):
    srt = chain(layout)
    n = srt.a.size
    assert n == 8 * 4096
    first = int(srt.a[0]) >> 56
    for k in M.chain_ks():
        m = check_model(lsb_built, srt, k)
        assert m.rounds == 8 and sum(m.equal) in (127, 128, 129)
        packed = [r.packed[0] for r in m.trace]
        if layout != "one_over":
            # every round's bucket is exactly half of its source: rounds 2 to 8 compact at 2 cand == held
            assert packed == [False] + [True] * 7
            assert all(2 * r.cand[0] == r.held[0] for r in m.trace[1:])
            assert sum(r.cand[0] for r in m.trace[1:]) == n - n // 128  # what B holds in the end
            assert m.read == [n + 2 * n - n // 64] and m.equal == [128]
        elif m.pivot >> 56 == first:
            # one candidate too many: round two filters A again
            assert 2 * m.trace[1].cand[0] == m.trace[1].held[0] + 2 and not packed[1] and packed[2]
            assert m.trace[2].held[0] == n
        else:
            assert packed[1] and 2 * m.trace[1].cand[0] == m.trace[1].held[0] - 2
    ks = M.chain_ks()
    assert len(ks) > 180 and {0, n - 1, n // 64 - 1, n // 64, n // 64 + 1, n // 2 - 1, n // 2} <= set(ks)
    if layout != "shuffled":
        # matching tiles match whole: every flush inside the loop is of a full stage (one_over: a k of
        # the bucket that lost a record, whose round two does compact)
        k2 = next(k for k in ks if int(srt.sorted[k]) >> 56 != first) if layout == "one_over" else 0
        r2 = M.round_model(srt.a, 1, k2).trace[1]
        assert r2.packed == (True,)
        f = M.flush_model(srt.a, r2.prefix, r2.mask)
        assert len(f.fills) >= 1 and set(f.fills) == {512} and f.final >= len(f.fills)


def test_blocks_model_and_conditions(lsb_built):
    keys = M.blocks_keys()
    srt = Sorted(keys, 1)
    ks = M.bucket_ks(keys, M.BLOCKS_TOP)
    assert len(ks) == 36 and ks[1] > 0 and ks[-2] < keys.size - 1  # top bytes on both sides of the bucket
    for k in ks:
        m = check_model(lsb_built, srt, k)
        if m.pivot >> 56 == M.BLOCKS_TOP:
            assert m.trace[1].packed == (True,) and 2 * m.trace[1].cand[0] <= keys.size
    r2 = M.round_model(keys, 1, ks[len(ks) // 2]).trace[1]
    assert r2.prefix >> 56 == M.BLOCKS_TOP and r2.packed == (True,)
    f = M.flush_model(keys, r2.prefix, r2.mask)
    assert any(449 <= x <= 511 for x in f.fills), f.fills


def test_dense_model_and_conditions(lsb_built):
    n = M.dense_n()
    tile, block, stage, cap = M.geometry()
    assert -(-n // tile) >= 2 * cap  # every workgroup of the capped grid takes two tiles
    keys = M.top3_keys(n)
    srt = Sorted(keys, 1)
    tops = set()
    for k in M.dense_ks(n):
        m = check_model(lsb_built, srt, k)
        tops.add(m.pivot >> 56)
        r2 = m.trace[1]
        assert r2.packed == (True,)
        f = M.flush_model(keys, r2.prefix, r2.mask)
        assert 2 * f.flushed >= f.waves and any(x % 64 for x in f.fills), (f.flushed, f.waves)
        assert all(stage - 63 <= x <= stage for x in f.fills)
    assert tops == {0, 1, 2}


def test_mixed_model_and_conditions(lsb_built):
    keys = M.mixed_keys()
    P, per = M.MIXED_P, M.MIXED_PER
    assert keys.size == 3 * per - 1 and per == 2 * 4096 + 3
    top = keys >> np.uint64(56)
    assert np.all(top[:per] == M.MIXED_TOP) and not np.any(top[2 * per:] == M.MIXED_TOP)
    assert set(np.unique(keys[:per] >> np.uint64(48) & np.uint64(0xff)).tolist()) == set(M.MIXED_BYTE6)
    in1 = np.count_nonzero(top[per:2 * per] == M.MIXED_TOP)
    assert 0.35 * per < in1 < 0.45 * per and np.all(top[per:2 * per][top[per:2 * per] != M.MIXED_TOP] >= 0x80)
    srt = Sorted(keys, P)
    ks, swap = M.mixed_ks(keys)
    assert len(ks) >= 35 and swap in ks
    both = 0
    for k in ks:
        m = check_model(lsb_built, srt, k)
        if m.pivot >> 56 == M.MIXED_TOP:
            # round two: rank 0 filters A, rank 1 compacts, rank 2 has no candidate and launches nothing
            assert m.trace[1].packed == (False, True, False) and m.trace[1].cand[2] == 0
            assert m.read[2] == M.here_of(keys.size, P, 2)
            both += any(r.packed[0] and r.packed[1] for r in m.trace[2:])
    assert both >= 16  # ... and in a later round both compact
    m = check_model(lsb_built, srt, swap)
    assert m.trace[1].packed == (False, False, True) and m.trace[1].cand[:2] == (0, 0)
    assert m.read[:2] == [per, per]
