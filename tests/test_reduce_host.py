"""Reductions over the runs' values, host side (no GPU needed): the planner
lsb_plan_run_tails (include/lsb.h, "runs of equal keys") against a walk over
the whole array, its identities bit for bit, and the argument checks that
return before any device call."""
import ctypes

import numpy as np
import pytest

from test_runs_host import summarise

INVALID = 1
SUM, MIN, MAX = 0, 1, 2
U64, I64, F64, U32 = 0, 1, 2, 3
NEG_ZERO = 0x8000000000000000
# (op, value type) -> the identity's bits: 0, -0.0, and the values whose
# encoding is all ones (min) or 0 (max)
IDENTITY = {(SUM, U64): 0, (SUM, I64): 0, (SUM, F64): NEG_ZERO,
            (MIN, U64): 2**64 - 1, (MIN, I64): 2**63 - 1, (MIN, F64): 2**63 - 1,
            (MAX, U64): 0, (MAX, I64): 2**63, (MAX, F64): 2**64 - 1}


def splitmix64(i):
    """splitmix64 of the positions i (uint64, wrapping)."""
    with np.errstate(over="ignore"):
        z = (np.asarray(i, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def encode(bits, vt):
    """lsb_key_encode's order of a 64-bit type, from the header's table."""
    sign = np.uint64(1 << 63)
    bits = np.asarray(bits, dtype=np.uint64)
    if vt == I64:
        return bits ^ sign
    if vt == F64:
        return np.where((bits & sign) != 0, ~bits, bits ^ sign)
    return bits


def values_for(n, op, vt):
    """The value bits of positions 0..n-1: a hash of the position; for a sum
    of doubles integer-valued ones below 2^31 in magnitude, so that every
    order of addition is exact."""
    h = splitmix64(np.arange(n))
    if op == SUM and vt == F64:
        return ((h >> np.uint64(32)).astype(np.int64) - (1 << 31)).astype(np.float64).view(np.uint64)
    return h


def fold(bits, op, vt):
    """op over the value bits, in order, from the identity -> bits (int)."""
    bits = np.asarray(bits, dtype=np.uint64)
    if bits.size == 0:
        return IDENTITY[(op, vt)]
    if op == SUM and vt == F64:
        acc = np.float64(-0.0)
        for x in bits.view(np.float64):
            acc = acc + x
        return int(np.float64(acc).view(np.uint64))
    if op == SUM:
        with np.errstate(over="ignore"):
            return int(np.add.reduce(bits))
    e = encode(bits, vt)
    return int(bits[np.argmin(e) if op == MIN else np.argmax(e)])


def brute_tails(a, vals, n, P, op, vt):
    """tail[r]: op over the values of the records after rank r's last one that
    carry on its run, found by walking the whole array."""
    per = -(-n // P) if P else 0
    out = []
    for r in range(P):
        lo, hi = r * per, min(n, (r + 1) * per)
        if hi <= lo:
            out.append(IDENTITY[(op, vt)])
            continue
        e = hi
        while e < n and a[e] == a[e - 1]:
            e += 1
        out.append(fold(vals[hi:e], op, vt))
    return out


def leads_of(a, vals, n, P, summary, op, vt, rng):
    """lead[s] from its definition; garbage where the planner must not look
    (empty ranks, ranks whose first slot starts a run)."""
    per = -(-n // P) if P else 0
    lead = rng.integers(0, 2**63, P).astype(np.uint64)
    for s in range(P):
        lo, hi = s * per, min(n, (s + 1) * per)
        if hi > lo and lo > 0 and a[lo] == a[lo - 1]:
            lead[s] = fold(vals[lo:lo + int(summary[s, 3])], op, vt)
    return lead


@pytest.mark.parametrize("op,vt", [(SUM, U64), (SUM, F64), (MIN, I64), (MAX, F64)])
def test_tails_against_a_walk(lsb_built, op, vt):
    L = lsb_built
    rng = np.random.default_rng(11 + 3 * op + vt)
    for _ in range(1500):
        n = int(rng.integers(0, 41))
        P = int(rng.integers(1, 9))
        a = rng.integers(0, int(rng.integers(1, 5)), n).astype(np.uint64)
        if rng.integers(0, 2):
            a.sort()
        vals = values_for(n, op, vt)
        s = summarise(a, n, P)
        got = L.plan_run_tails(n, P, s, op, vt, leads_of(a, vals, n, P, s, op, vt, rng))
        assert [int(x) for x in got] == brute_tails(a, vals, n, P, op, vt), (a.tolist(), P)


def test_identities_bit_for_bit(lsb_built):
    L = lsb_built
    n, P = 12, 4  # per = 3; one key per rank: nothing continues
    a = np.repeat(np.arange(4, dtype=np.uint64), 3)
    s = summarise(a, n, P)
    for (op, vt), want in IDENTITY.items():
        got = L.plan_run_tails(n, P, s, op, vt, np.full(P, 0x1234, dtype=np.uint64))
        assert [int(x) for x in got] == [want] * P, (op, vt)
        # n = 0 and n < P: empty ranks get the identity
        assert [int(x) for x in L.plan_run_tails(0, 3, np.zeros((3, 4), np.uint64), op, vt,
                                                 np.zeros(3, np.uint64))] == [want] * 3
        assert int(L.plan_run_tails(1, 3, summarise(a[:1], 1, 3), op, vt, np.zeros(3, np.uint64))[2]) == want
        # the identity's encoding is the order's end
        if op != SUM:
            assert int(encode(np.uint64(want), vt)) == (2**64 - 1 if op == MIN else 0)
    # one key everywhere, every lead -0.0: the chain sums to -0.0, and +0.0 once makes it +0.0
    one = summarise(np.zeros(n, dtype=np.uint64), n, P)
    lead = np.full(P, NEG_ZERO, dtype=np.uint64)
    assert [int(x) for x in L.plan_run_tails(n, P, one, SUM, F64, lead)] == [NEG_ZERO] * P
    lead[2] = 0
    assert [int(x) for x in L.plan_run_tails(n, P, one, SUM, F64, lead)] == [0, 0, NEG_ZERO, NEG_ZERO]
    # min and max give one of the values back, NaNs at the ends by their sign
    nan_pos, nan_neg = 0x7ff8000000000001, 0xfff8000000000001
    lead = np.array([0, np.float64(1.5).view(np.uint64), nan_pos, nan_neg], dtype=np.uint64)
    assert int(L.plan_run_tails(n, P, one, MAX, F64, lead)[0]) == nan_pos
    assert int(L.plan_run_tails(n, P, one, MIN, F64, lead)[0]) == nan_neg
    lead = np.array([0, 0, NEG_ZERO, 0], dtype=np.uint64)
    assert int(L.plan_run_tails(n, P, one, MIN, F64, lead)[0]) == NEG_ZERO  # -0.0 is below +0.0


def test_refuses_what_plan_runs_refuses(lsb_built):
    L = lsb_built
    n, P = 12, 3
    good = summarise(np.array([1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 4, 4], dtype=np.uint64), n, P)
    lead = np.zeros(P, dtype=np.uint64)
    L.plan_run_tails(n, P, good, SUM, U64, lead)
    col = {"first": 0, "last": 1, "inner": 2, "lead": 3}
    bad = [(r, w) for r in range(P) for w in ({"lead": 0}, {"lead": 5}, {"lead": 2**64 - 1}, {"inner": 4},
                                              {"inner": 2**63})]
    bad += [(0, {"inner": 0}), (0, {"lead": 4}), (1, {"first": 9})]
    for r, words in bad:
        s = good.copy()
        for k, v in words.items():
            s[r, col[k]] = v
        for plan in (lambda: L.plan_runs(n, P, s), lambda: L.plan_run_tails(n, P, s, SUM, U64, lead)):
            with pytest.raises(L.LsbError) as e:
                plan()
            assert e.value.code == INVALID, (r, words)


def test_refuses_bad_arguments(lsb_built):
    lib = lsb_built._lib()
    P = 2
    s = np.zeros((P, 4), dtype=np.uint64)
    s[:, 3] = 1
    lead, tail = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.uint64)
    args = [2, P, s.ctypes.data, SUM, U64, lead.ctypes.data, tail.ctypes.data]
    assert lib.lsb_plan_run_tails(*args) == 0

    def but(i, v):
        a = list(args)
        a[i] = v
        return lib.lsb_plan_run_tails(*a)

    for i in (2, 5, 6):
        assert but(i, None) == INVALID, i
    assert but(0, -1) == INVALID
    assert but(1, 0) == INVALID and but(1, 65) == INVALID
    assert but(3, 3) == INVALID and but(3, -1) == INVALID
    for vt in (U32, 4, 5, 6, -1):
        assert but(4, vt) == INVALID, vt


def test_entry_points_refuse_a_null_context(lsb_built):
    lib = lsb_built._lib()
    t = ctypes.c_int64(-5)
    assert lib.lsb_plan_reduce(None, SUM, U64) == INVALID
    assert lib.lsb_plan_reduce(None, 3, U32) == INVALID
    assert lib.lsb_store_reduce(None, 0, 4, None, ctypes.byref(t)) == INVALID
    assert lib.lsb_store_reduce(None, -1, -1, None, None) == INVALID
    assert t.value == -5
