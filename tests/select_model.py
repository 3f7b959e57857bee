"""The select's rounds and its compaction's flushes as plain numpy, written out
from DESIGN.md §7.5 and include/lsb.h, and the inputs that reach the
compaction's dense, clustered, chained and mixed-rank cases (no GPU, no
library call: tests/test_select_host.py holds the model against the stable
sort, tests/test_select_gpu.py holds the library against the model).

round_model   the host rule of lsb_select: which rank reads what in which
              round, who compacts, the pivot and every rank's counts
flush_model   the reservations a compaction out of A makes: every wave's fill
              at each flush inside the tile loop, and the waves that flush at
              the end (the order inside B depends on the atomics and is not
              modelled)
The geometry (tile, workgroup, stage, grid cap) is read out of the sources, so
a change of it moves the model with it.
"""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-lsb_amd", "csrc")
U = np.uint64


@functools.lru_cache(maxsize=None)
def _sources():
    return "\n".join(open(os.path.join(CSRC, f)).read() for f in ("lsb_kernels.h", "lsb_tile.h", "lsb_select.hip"))


@functools.lru_cache(maxsize=None)
def constant(name):
    """An integer constant of the kernels' sources: `constexpr int name = ...;`
    or `#define name ...`, products and quotients of such."""
    m = re.search(r"constexpr int %s = ([^;]+);" % name, _sources()) or \
        re.search(r"#define %s ([^\n]+)" % name, _sources())
    assert m, name
    expr = re.sub(r"[A-Za-z_]\w*", lambda t: str(constant(t.group(0))), m.group(1))
    assert re.fullmatch(r"[\d\s*/()+-]+", expr), (name, expr)
    return int(eval(expr.replace("/", "//")))  # noqa: S307  digits and operators only


def geometry():
    """-> (kTile, kTileBlock, kSelStage, kSelGridCap)."""
    return tuple(constant(n) for n in ("kTile", "kTileBlock", "kSelStage", "kSelGridCap"))


def here_of(n, P, r):
    per = -(-n // P)
    return max(0, min(per, n - r * per))


# ---------------------------------------------------------------- the rounds
Round = collections.namedtuple("Round", "shift held cand packed prefix mask")
Rounds = collections.namedtuple("Rounds", "pivot below equal rounds read trace")


def round_model(keys, P, k):
    """lsb_select(k) over the block partition of `keys` (mapped uint64) on P
    ranks -> Rounds(pivot, below[P], equal[P], rounds, read[P], trace); trace
    holds, per round, what the round started from: (shift, held[P], cand[P],
    packed[P], prefix, mask).  sum(read) is the records read on all ranks."""
    keys = np.ascontiguousarray(keys, dtype=U)
    n = keys.size
    assert 0 <= k < n and P >= 1
    per = -(-n // P)
    left = [keys[min(n, r * per): min(n, r * per) + here_of(n, P, r)] for r in range(P)]  # a rank's candidates
    held = [here_of(n, P, r) for r in range(P)]
    cand = list(held)
    kor = int(np.bitwise_or.reduce(keys))
    knor = int(np.bitwise_or.reduce(~keys))
    varying = kor & knor
    below, read, trace = [0] * P, [0] * P, []
    prefix = mask = 0
    remaining, shift, first = k, 56, True
    while shift >= 0:
        packed = [not first and cand[r] > 0 and 2 * cand[r] <= held[r] for r in range(P)]
        trace.append(Round(shift, tuple(held), tuple(cand), tuple(packed), prefix, mask))
        for r in range(P):
            if cand[r] > 0:
                read[r] += held[r]
            if packed[r]:
                held[r] = cand[r]
        byte = [(a >> U(shift)).astype(np.uint8) for a in left]
        hist = [np.bincount(b, minlength=256) for b in byte]
        total = np.sum(hist, axis=0)
        upto = np.cumsum(total)
        b = int(np.searchsorted(upto, remaining, "right"))  # the first bucket whose end lies past `remaining`
        assert b < 256
        remaining -= int(upto[b] - total[b])
        for r in range(P):
            below[r] += int(hist[r][:b].sum())
            cand[r] = int(hist[r][b])
            left[r] = left[r][byte[r] == b]
        prefix |= b << shift
        mask |= 0xff << shift
        shift -= 8
        while shift >= 0 and (varying >> shift) & 0xff == 0:  # a byte on which all keys agree: from the span
            prefix |= kor & (0xff << shift)
            mask |= 0xff << shift
            shift -= 8
        first = False
    return Rounds(prefix, below, cand, len(trace), read, trace)


# ---------------------------------------------------------------- the flushes
Flushes = collections.namedtuple("Flushes", "fills final waves flushed")


def flush_model(rank_keys, prefix, mask, grid_cap=None):
    """The compacting k_sel_hist over a rank's A with this prefix and mask ->
    Flushes(fills: the fill at every flush inside the tile loop, final: the
    waves that flush at the end, waves: all waves, flushed: those with at
    least one flush inside the loop)."""
    tile, block, stage, cap = geometry()
    cap = grid_cap or cap
    waves, items = block // 64, tile // block
    a = np.ascontiguousarray(rank_keys, dtype=U)
    tiles = -(-a.size // tile)
    G = min(tiles, cap)
    steps = -(-tiles // G)  # tiles of the workgroup that takes the most
    match = np.zeros(steps * G * tile, dtype=bool)
    match[:a.size] = (a & U(mask)) == U(prefix)
    # position = t * tile + i * block + w * 64 + lane, t = step * G + g
    cnt = match.reshape(steps, G, items, waves, 64).sum(axis=4)
    fill = np.zeros((G, waves), dtype=np.int64)
    flushed = np.zeros((G, waves), dtype=bool)
    fills = []
    for s in range(steps):
        for i in range(items):
            c = cnt[s, :, i, :]
            over = fill + c > stage
            fills.extend(fill[over].tolist())
            flushed |= over
            fill = np.where(over, c, fill + c)
    return Flushes(fills, int(np.count_nonzero(fill)), G * waves, int(np.count_nonzero(flushed)))


# ---------------------------------------------------------------- the inputs
def _low(rng, n, bits):
    return rng.integers(0, 1 << bits, n, dtype=np.int64).astype(U)


# a. two values per byte, byte 7 first: distinct within a byte, no pair twice,
#    and not in the same order everywhere
CHAIN_PAIRS = ((0x31, 0xC4), (0xE0, 0x07), (0x5A, 0x5B), (0x02, 0xFD), (0x9C, 0x13), (0x48, 0x80), (0xFF, 0x6E),
               (0x25, 0xB9))
CHAIN_N = 8 * 4096


def chain_keys(layout):
    """The halving chain: n = 8 tiles, P = 1.  The record with code c takes
    byte 7 from bit 14 of c, byte 6 from bit 13, ... byte 0 from bit 7, so
    every round's chosen bucket is half of its source and 128 records share
    each key.  layout: "sorted" (c = position), "shuffled" (a fixed
    permutation), "one_over" (sorted, with the last record, of the other
    top-byte bucket, given the first record's key: 2 cand = held + 2 after
    round one for every k in the first record's bucket)."""
    n = CHAIN_N
    c = np.arange(n, dtype=np.int64)
    if layout == "shuffled":
        c = np.random.default_rng(815).permutation(n)
    keys = np.zeros(n, dtype=U)
    for byte, (v0, v1) in zip(range(7, -1, -1), CHAIN_PAIRS):
        bit = (c >> (byte + 7)) & 1
        keys |= np.where(bit == 1, U(v1), U(v0)) << U(8 * byte)
    if layout == "one_over":
        assert keys[-1] >> U(56) != keys[0] >> U(56)
        keys[-1] = keys[0]
    else:
        assert layout in ("sorted", "shuffled")
    return keys


def chain_ks(n=CHAIN_N):
    """Every multiple of n / 64, each +- 1, with 0 and n - 1."""
    ks = {0, n - 1}
    for m in range(0, n + 1, n // 64):
        ks |= {m - 1, m, m + 1}
    return sorted(k for k in ks if 0 <= k < n)


BLOCKS_N = 6 * 4096 + 5
BLOCKS_TOP = 0x40


def blocks_keys():
    """b. Three-quarter blocks, P = 1: the records of the first three tiles
    take top byte 0x40 with probability 3/4, every other record a top byte
    below or above it; 56 random bits under it.  A wave of a matching tile
    stages about 48 records per item, so its stage fills to 449..511 before
    the item that does not fit."""
    n = BLOCKS_N
    rng = np.random.default_rng(3404)
    top = np.where(rng.random(n) < 0.5, rng.integers(0x00, BLOCKS_TOP, n), rng.integers(BLOCKS_TOP + 1, 0x100, n))
    dense = (np.arange(n) < 3 * 4096) & (rng.random(n) < 0.75)
    top[dense] = BLOCKS_TOP
    keys = top.astype(U) << U(56) | _low(rng, n, 56)
    inside = int(np.count_nonzero(top == BLOCKS_TOP))
    assert 0 < 2 * inside <= n, "the bucket must compact"
    assert np.any(top < BLOCKS_TOP) and np.any(top > BLOCKS_TOP)
    return keys


def top3_keys(n, seed=99):
    """c. Three top-byte values over 56 random bits: a third of the records
    match wherever the pivot lies."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, n).astype(U) << U(56) | _low(rng, n, 56)


def dense_n():
    """Two tiles for every workgroup of the capped grid, a tile and a record."""
    tile, _, _, cap = geometry()
    return 2 * cap * tile + tile + 1


def dense_ks(n):
    """One k in each of the three buckets."""
    return (n // 6, n // 2 + 17, n - n // 6)


MIXED_P = 3
MIXED_PER = 2 * 4096 + 3
MIXED_N = MIXED_P * MIXED_PER - 1
MIXED_TOP = 0x20
MIXED_BYTE6 = (0x11, 0x77, 0xC3)


def mixed_keys():
    """d. Three ranks that decide differently.  Rank 0: every record in
    top-byte bucket 0x20, byte 6 one of three values.  Rank 1: 40 % of the
    records, anywhere, in 0x20, the rest at or above 0x80.  Rank 2: top bytes
    0x30..0x5f, none in 0x20.  Random bits below."""
    per, n = MIXED_PER, MIXED_N
    rng = np.random.default_rng(7103)
    top = np.empty(n, dtype=np.int64)
    top[:per] = MIXED_TOP
    top[per:2 * per] = np.where(rng.random(per) < 0.4, MIXED_TOP, rng.integers(0x80, 0x100, per))
    top[2 * per:] = rng.integers(0x30, 0x60, n - 2 * per)
    keys = top.astype(U) << U(56) | _low(rng, n, 56)
    six = np.asarray(MIXED_BYTE6, dtype=U)[rng.integers(0, 3, per)]
    keys[:per] = (keys[:per] & ~(U(0xff) << U(48))) | six << U(48)
    return keys


def bucket_ks(keys, top, more=()):
    """32 evenly spaced positions of the sort inside top-byte bucket `top`,
    its two edges, 0 and n - 1, and `more`."""
    tops = np.sort(keys >> U(56))
    lo = int(np.searchsorted(tops, U(top), "left"))
    hi = int(np.searchsorted(tops, U(top), "right")) - 1
    assert hi - lo >= 33
    return sorted({0, keys.size - 1, lo, hi, *np.linspace(lo, hi, 34).astype(np.int64)[1:-1].tolist(), *more})


def mixed_ks(keys):
    """Inside bucket 0x20, and one inside rank 2's buckets, where ranks 0 and
    1 hold no candidate after round one and rank 2 compacts."""
    tops = np.sort(keys >> U(56))
    swap = (int(np.searchsorted(tops, U(0x30), "left")) + int(np.searchsorted(tops, U(0x60), "left"))) // 2
    return bucket_ks(keys, MIXED_TOP, more=(swap,)), swap
