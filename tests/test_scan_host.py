"""Scans within the runs, host side (no GPU needed): the planner
lsb_plan_run_carries (include/lsb.h, "a scan within the runs") against a walk
over the whole array, float sums folded left in rank order bit for bit, its
identities, and the argument checks that return before any device call."""
import ctypes

import numpy as np
import pytest

from test_reduce_host import IDENTITY, encode, splitmix64
from test_runs_host import summarise

INVALID = 1
SUM, MIN, MAX, COUNT, START = 0, 1, 2, 3, 4
U64, I64, F64, U32 = 0, 1, 2, 3
PAIRS = [(op, vt) for op in (SUM, MIN, MAX) for vt in (U64, I64, F64)] + [(COUNT, U64), (START, U64)]


def identity(op, vt):
    return 0 if op >= COUNT else IDENTITY[(op, vt)]


def values_for(n, op, vt):
    """The value bits of positions 0..n-1.  For a sum of doubles: finite
    doubles of both signs over 40 binades, so that the order and the
    association of the additions show in the bits."""
    h = splitmix64(np.arange(n))
    if vt == F64:
        mant = 1.0 + (h >> np.uint64(12)).astype(np.float64) * 2.0 ** -52
        d = np.ldexp(mant, ((h >> np.uint64(1)) % np.uint64(41)).astype(np.int64) - 20) * \
            np.where(h & np.uint64(1), -1.0, 1.0)
        return d.view(np.uint64).copy()
    return h


def fold(acc, bits, op, vt):
    """acc (int bits), then op with every value of bits in order -> int bits."""
    for b in np.asarray(bits, dtype=np.uint64):
        if op >= COUNT:
            acc = (acc + 1) % 2**64
        elif op == SUM and vt == F64:
            s = np.array([acc], dtype=np.uint64).view(np.float64)[0] + np.array([b]).view(np.float64)[0]
            acc = int(np.array([s], dtype=np.float64).view(np.uint64)[0])
        elif op == SUM:
            acc = (acc + int(b)) % 2**64
        else:
            ea, eb = int(encode(np.uint64(acc), vt)), int(encode(b, vt))
            if (eb < ea) if op == MIN else (eb > ea):
                acc = int(b)
    return acc


def fold_words(acc, words, op, vt):
    """The planner's fold: trail words combine as values do, each counting
    word adding its count."""
    if op >= COUNT:
        return (acc + sum(int(x) for x in words)) % 2**64
    return fold(acc, words, op, vt)


def blocks(n, P):
    per = -(-n // P) if P else 0
    return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(P)]


def trails_of(a, vals, n, P, op, vt, rng):
    """trail[s] from its definition: op over rank s's records from its last
    head on (slot 0 is one when a run starts there), all of them without one;
    garbage for empty ranks."""
    trail = rng.integers(0, 2**63, P).astype(np.uint64)
    for s, (lo, hi) in enumerate(blocks(n, P)):
        if hi <= lo:
            continue
        p = hi - 1
        while p > lo and a[p] == a[p - 1]:
            p -= 1
        trail[s] = fold(identity(op, vt), vals[p:hi], op, vt)
    return trail


def brute_carries(a, n, P, trail, op, vt):
    """carry[r]: with s the start of the run that holds r's first record, the
    left fold, in rank order from the identity, of the trail words of the
    ranks below r that hold records of [s, r's first slot)."""
    out = []
    for r, (lo, hi) in enumerate(blocks(n, P)):
        acc = identity(op, vt)
        if hi > lo:
            s = lo
            while s > 0 and a[s] == a[s - 1]:
                s -= 1
            words = [trail[q] for q, (qlo, qhi) in enumerate(blocks(n, P)) if q < r and qhi > qlo and qhi > s]
            acc = fold_words(acc, words, op, vt)
        out.append(acc)
    return out


def arrays(rng):
    """Small arrays of few distinct keys at every P of the issue: n < P, runs
    over several whole ranks, runs that end at a rank's last slot."""
    for P in (1, 2, 3, 5, 8):
        for n in range(0, 41):
            a = rng.integers(0, int(rng.integers(1, 4)), n).astype(np.uint64)
            if rng.integers(0, 2):
                a.sort()
            yield a, n, P
    per = 5  # by construction: one run over ranks 1..3 whole, one ending at rank 0's last slot
    a = np.array([1] * 2 + [2] * 3 + [3] * 15 + [4] * 5, dtype=np.uint64)
    yield a, a.size, 5
    assert -(-a.size // 5) == per


@pytest.mark.parametrize("op,vt", PAIRS)
def test_carries_against_a_walk(lsb_built, op, vt):
    L = lsb_built
    rng = np.random.default_rng(23 + 5 * op + vt)
    seen_chain = False
    for a, n, P in arrays(rng):
        vals = values_for(n, op, vt)
        s = summarise(a, n, P)
        trail = trails_of(a, vals, n, P, op, vt, rng)
        got = [int(x) for x in L.plan_run_carries(n, P, s, op, vt, trail)]
        want = brute_carries(a, n, P, trail, op, vt)
        assert got == want, (a.tolist(), P)
        if op >= COUNT:  # the records of the leading run on earlier ranks, by position
            for r, (lo, hi) in enumerate(blocks(n, P)):
                if hi > lo:
                    st = lo
                    while st > 0 and a[st] == a[st - 1]:
                        st -= 1
                    assert got[r] == lo - st, (a.tolist(), P, r)
                    seen_chain = seen_chain or lo - st > -(-n // P)
    assert seen_chain or op < COUNT  # a carry that spans more than one whole rank was among them


def test_float_sums_fold_left_in_rank_order(lsb_built):
    """Three trail words whose sum depends on the association:
    (1 + 2^-53) + 2^-53 = 1 in a left fold from -0.0, 1 + 2^-52 the other way."""
    L = lsb_built
    n, P = 8, 4  # per = 2, one key: rank 3's carry takes ranks 0, 1, 2 in that order
    one = summarise(np.zeros(n, dtype=np.uint64), n, P)
    w = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 7.0], dtype=np.float64)
    got = L.plan_run_carries(n, P, one, SUM, F64, w.view(np.uint64)).view(np.float64)
    assert got[3] == (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0
    assert got[3] != 1.0 + (2.0 ** -53 + 2.0 ** -53)
    assert got.view(np.uint64)[0] == 0x8000000000000000  # rank 0: the identity, -0.0
    assert got[1] == 1.0 and got[2] == 1.0 + 2.0 ** -53


def test_identities_bit_for_bit(lsb_built):
    L = lsb_built
    n, P = 12, 4  # per = 3; one key per rank: every rank's slot 0 starts a run
    a = np.repeat(np.arange(4, dtype=np.uint64), 3)
    s = summarise(a, n, P)
    for op, vt in PAIRS:
        want = identity(op, vt)
        got = L.plan_run_carries(n, P, s, op, vt, np.full(P, 0x1234, dtype=np.uint64))
        assert [int(x) for x in got] == [want] * P, (op, vt)
        assert [int(x) for x in L.plan_run_carries(0, 3, np.zeros((3, 4), np.uint64), op, vt,
                                                   np.zeros(3, np.uint64))] == [want] * 3
        assert int(L.plan_run_carries(1, 3, summarise(a[:1], 1, 3), op, vt, np.zeros(3, np.uint64))[2]) == want


def test_refuses_what_plan_runs_refuses(lsb_built):
    L = lsb_built
    n, P = 12, 3
    good = summarise(np.array([1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 4, 4], dtype=np.uint64), n, P)
    trail = np.zeros(P, dtype=np.uint64)
    L.plan_run_carries(n, P, good, SUM, U64, trail)
    col = {"first": 0, "last": 1, "inner": 2, "lead": 3}
    bad = [(r, w) for r in range(P) for w in ({"lead": 0}, {"lead": 5}, {"lead": 2**64 - 1}, {"inner": 4},
                                              {"inner": 2**63})]
    bad += [(0, {"inner": 0}), (0, {"lead": 4}), (1, {"first": 9})]
    for r, words in bad:
        s = good.copy()
        for k, v in words.items():
            s[r, col[k]] = v
        for plan in (lambda: L.plan_runs(n, P, s), lambda: L.plan_run_carries(n, P, s, COUNT, U64, trail)):
            with pytest.raises(L.LsbError) as e:
                plan()
            assert e.value.code == INVALID, (r, words)


def test_refuses_bad_arguments(lsb_built):
    lib = lsb_built._lib()
    P = 2
    s = np.zeros((P, 4), dtype=np.uint64)
    s[:, 3] = 1
    trail, carry = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.uint64)
    args = [2, P, s.ctypes.data, SUM, U64, trail.ctypes.data, carry.ctypes.data]
    assert lib.lsb_plan_run_carries(*args) == 0

    def but(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.lsb_plan_run_carries(*a)

    for i in (2, 5, 6):
        assert but(**{f"a{i}": None}) == INVALID, i
    assert but(a0=-1) == INVALID
    assert but(a1=0) == INVALID and but(a1=65) == INVALID
    assert but(a3=5) == INVALID and but(a3=-1) == INVALID
    for vt in (U32, 4, 5, 6, -1):
        assert but(a4=vt) == INVALID, vt
    for op in (COUNT, START):
        assert but(a3=op) == 0
        assert but(a3=op, a4=F64) == INVALID and but(a3=op, a4=I64) == INVALID


def test_entry_points_refuse_a_null_context(lsb_built):
    lib = lsb_built._lib()
    t = ctypes.c_int64(-5)
    assert lib.lsb_plan_scan(None, SUM, U64) == INVALID
    assert lib.lsb_plan_scan(None, 9, U32) == INVALID
    assert lib.lsb_store_scan(None, 0, 4, None, ctypes.byref(t)) == INVALID
    assert lib.lsb_store_scan(None, -1, -1, None, None) == INVALID
    assert lib.lsb_scan_runs(None, 0) == INVALID
    assert t.value == -5
