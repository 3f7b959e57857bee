"""The hybrid local sort (LSB_OPT_HYBRID) as plain numpy: which route a
one-rank sort takes, how many passes it runs, and its output (no GPU, no
library call: tests/test_hybrid_model.py holds the model against the stable
sort, tests/test_hybrid_limits_gpu.py holds the library against the model).

It restates distributed-lsb_amd/csrc: LocalSort::queue / hybrid_passes /
finish (lsb_passes.cpp), k_onesweep's SEG write-out (seg_pos,
lsb_kernels.hip), k_segfix and k_segsort (lsb_segsort.hip).

  plan           digits, the hybrid's top bytes, and whether it is taken at
                 all (varying bits, hybrid_bytes, the skewed / constant byte)
  fused_pass     the last byte pass with SEG: every record's stage slot from
                 walks cut at kSegMax; error bit 2
  segfix         k_segfix per tile boundary: a, c, nm as the kernel counts
                 them, the form (CAP, QW) launch_segfix picks; error bit 1
  segsort        k_segsort per tile: owned range, tail, its own error rule
  hybrid_sort    the whole sort: (output, route, passes, pass shifts)

The geometry is read out of the sources, so a constant that moves either
moves the inputs below with it or fails an assertion here.

The first part of the file is the model at toy geometry as it was written
for tests/test_hybrid_model.py (per-record loops, T = 32...256); the shipped
geometry uses the vectorised functions after it.
"""
import collections
import functools
import os
import random
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-lsb_amd", "csrc")
DT = np.dtype([("key", "<u8"), ("val", "<u8")])
U = np.uint64


def _byte(keys, b):
    return ((keys >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.int64)


# ------------------------------------------------- the model at toy geometry
def hybrid_model(a, msd, T, cap):
    """Mode 1 of the hybrid on records a (msd: the top bytes, least
    significant first).  Returns (output, ok); ok False = k_segfix's error."""
    x = a
    for b in msd[:-1]:
        x = x[np.argsort(_byte(x["key"], b), kind="stable")]
    last = msd[-1]
    pmask = np.uint64(sum(0xFF << (8 * b) for b in msd))
    rmask = pmask & ~np.uint64(0xFF << (8 * last))
    m = x.size
    d = _byte(x["key"], last)
    # The plain last pass: slot of each input record (stable by digit).
    order = np.argsort(d, kind="stable")
    slot = np.empty(m, dtype=np.int64)
    slot[order] = np.arange(m)
    out = np.empty_like(x)
    # SEG: inside each tile's bucket block, segments ordered by the key.
    for t0 in range(0, m, T):
        idx = np.arange(t0, min(t0 + T, m))
        for dd in np.unique(d[idx]):
            blk = idx[d[idx] == dd]  # input order = the block's slot order
            s = slot[blk]
            seg = x["key"][blk] & pmask
            # stable by (segment, key): segments stay where they are, since
            # the block is already ordered by its segment (run key sorted)
            o = np.lexsort((x["key"][blk], seg))
            out[s] = x[blk[o]]
    # k_segfix
    ok = True
    rk = x["key"] & rmask
    for b in range(T, m, T):
        lo, hi = b - T, min(b + T, m)
        v = rk[b - 1]
        if rk[b] != v:
            continue
        a_ = 0
        while b - 1 - a_ >= lo and rk[b - 1 - a_] == v:
            a_ += 1
        c_ = 0
        while b + c_ < hi and rk[b + c_] == v:
            c_ += 1
        if a_ > cap or c_ > cap or (b - a_ == lo and lo > 0 and rk[lo - 1] == v) or \
                (b + c_ == hi and hi < m and rk[hi] == v):
            ok = False
            continue
        run = np.arange(b - a_, b + c_)
        left = run < b
        for dd in np.unique(d[run]):
            L, R = run[left & (d[run] == dd)], run[~left & (d[run] == dd)]
            if L.size == 0 or R.size == 0:
                continue
            # P: the end of tile t's bucket-dd block = the slot after its last record
            tile_blk = np.arange(lo, b)[d[lo:b] == dd]
            P = slot[tile_blk].max() + 1
            both = np.concatenate([L, R])  # input order: left first
            o = np.argsort(x["key"][both], kind="stable")
            out[P - L.size + np.arange(both.size)] = x[both[o]]
    return out, ok


def _keys(rng, n, run_values=None):
    a = np.zeros(n, dtype=DT)
    k = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    if run_values is not None:  # few values of the two run bytes: long runs
        pool = rng.choice(1 << 16, run_values, replace=False).astype(np.uint64)
        k = (k & ~np.uint64(0xFFFF << 40)) | (pool[rng.integers(0, run_values, n)] << np.uint64(40))
    a["key"] = k
    a["val"] = np.arange(n, dtype=np.uint64)
    return a


def fused_pass_model(x, last, pmask, T, seg_max, stale):
    """k_onesweep SEG on x (stably sorted by the lower top bytes) into a
    buffer holding `stale`: returns (out, bit2)."""
    m = x.size
    d = _byte(x["key"], last)
    counts = np.bincount(d, minlength=256)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    seen = np.zeros(256, dtype=np.int64)  # records of each bucket in earlier tiles
    out = stale.copy()
    bit2 = False
    keys = x["key"]
    for t0 in range(0, m, T):
        idx = np.arange(t0, min(t0 + T, m))
        stage = idx[np.argsort(d[idx], kind="stable")]  # the tile, bucket-ordered
        sk = keys[stage]
        sd = d[stage]
        nvalid = stage.size
        lstart = {dd: int(np.argmax(sd == dd)) for dd in np.unique(sd)}
        for j in range(nvalid):
            v = sk[j]
            pk = v & pmask
            pos = j
            sp = j > 0 and (sk[j - 1] & pmask) == pk
            sn = j + 1 < nvalid and (sk[j + 1] & pmask) == pk
            if sp or sn:
                less = eqb = 0
                k = j - 1
                klo = max(j - seg_max, 0)
                while k >= klo:
                    kk = sk[k]
                    if (kk & pmask) != pk:
                        break
                    less += kk < v
                    eqb += kk == v
                    k -= 1
                sfirst = k + 1
                too_long = k < klo and klo > 0
                khi = min(j + 1 + seg_max, nvalid)
                k = j + 1
                while k < khi:
                    kk = sk[k]
                    if (kk & pmask) != pk:
                        break
                    less += kk < v
                    k += 1
                too_long |= k == khi and khi < nvalid
                bit2 |= too_long
                pos = sfirst + less + eqb
            dd = int(sd[j])
            slot = base[dd] + seen[dd] + (pos - lstart[dd])
            if 0 <= slot < m:  # the kernel clamps into the buffer
                out[slot] = x[stage[j]]
        seen += np.bincount(sd, minlength=256)
    return out, bit2


def segfix_bit1(x, msd, T, cap):
    """k_segfix's verdict only (bit 1): a crossing run too long to merge."""
    last = msd[-1]
    rmask = np.uint64(sum(0xFF << (8 * b) for b in msd)) & ~np.uint64(0xFF << (8 * last))
    rk = x["key"] & rmask
    m = x.size
    for b in range(T, m, T):
        lo, hi = b - T, min(b + T, m)
        v = rk[b - 1]
        if rk[b] != v:
            continue
        a_ = c_ = 0
        while b - 1 - a_ >= lo and rk[b - 1 - a_] == v:
            a_ += 1
        while b + c_ < hi and rk[b + c_] == v:
            c_ += 1
        if a_ > cap or c_ > cap or (b - a_ == lo and lo > 0 and rk[lo - 1] == v) or \
                (b + c_ == hi and hi < m and rk[hi] == v):
            return True
    return False


def segsort_model(y, pmask, seg_max):
    """k_segsort over y (taken as sorted by pmask) in the comment's words, not
    the kernel's: every maximal run of equal pmask ordered by the whole key;
    (out, err) with err for a run over seg_max.  The kernel's own rule is
    `segsort` below."""
    out = y.copy()
    p = y["key"] & pmask
    i = 0
    while i < y.size:
        j = i + 1
        while j < y.size and p[j] == p[i]:
            j += 1
        if j - i > seg_max:
            return y, True
        out[i:j] = y[i:j][np.argsort(y["key"][i:j], kind="stable")]
        i = j
    return out, False


def hybrid_mode1(a, msd, T, seg_max, cap, stale, dispatch):
    """The hybrid's mode 1 end to end on a (one rank): passes on msd[:-1], the
    fused SEG pass, k_segfix, then the error dispatch ("shipped": bit 2 goes
    to the LSD passes; "pre_d4f7b64": every error takes k_segsort)."""
    x = a
    for b in msd[:-1]:
        x = x[np.argsort(_byte(x["key"], b), kind="stable")]
    pmask = np.uint64(sum(0xFF << (8 * b) for b in msd))
    fused, bit2 = fused_pass_model(x, msd[-1], pmask, T, seg_max, stale)
    if not bit2:  # k_segfix as the first model does it (the fused output is then exact in-tile)
        fused, ok = hybrid_model(a, msd, T, cap)
        bit1 = not ok
    else:
        bit1 = segfix_bit1(x, msd, T, cap)
    err = (1 if bit1 else 0) | (2 if bit2 else 0)
    if err == 0:
        return fused, "fused"
    lsd = a[np.argsort(a["key"], kind="stable")]  # the LSD passes over the kept input
    if dispatch == "shipped" and err & 2:
        return lsd, "lsd"
    out, serr = segsort_model(fused, pmask, seg_max)
    return (lsd, "lsd") if serr else (out, "segsort")


def _seed19_like(rng, n, v4=64):
    """Stress seed 19's shape: bytes 3 and 5 constant, bytes 6
    and 7 two values each, so the hybrid's top bytes are 4, 6, 7; byte 4 takes
    v4 values here, so a segment (records equal on them) holds ~n / (4 v4)
    records: several times the walk's cut, as ~340 records were against
    kSegMax = 64 in the stress input."""
    k = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    k = (k & ~np.uint64(0xFF << 24)) | np.uint64(0x5A << 24)
    k = (k & ~np.uint64(0xFF << 40)) | np.uint64(0x11 << 40)
    k = (k & ~np.uint64(0xFF << 32)) | (rng.integers(0, v4, n, dtype=np.uint64) << np.uint64(32))
    b6 = rng.choice(np.array([0x20, 0x9C], dtype=np.uint64), n)
    b7 = rng.choice(np.array([0x03, 0xE1], dtype=np.uint64), n)
    k = (k & ~np.uint64(0xFFFF << 48)) | (b6 << np.uint64(48)) | (b7 << np.uint64(56))
    a = np.zeros(n, dtype=DT)
    a["key"] = k
    a["val"] = np.arange(n, dtype=np.uint64)
    return a


# ------------------------------------------------------ the shipped geometry
@functools.lru_cache(maxsize=None)
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _sources():
    return "\n".join(_source(f) for f in ("lsb_kernels.h", "lsb_tile.h", "lsb_ostile.h", "lsb_segsort.hip"))


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


Geometry = collections.namedtuple("Geometry", "tile seg_max seg_cap subs seg_tile skew_shift rlen_max forms")


@functools.lru_cache(maxsize=None)
def geometry():
    """kTile, kSegMax, kSegCap, kOnesweepSubs, kSegTile; the skew rule's shift
    (a bucket over m >> 5 records, onesweep_halves_for); launch_segfix's rule
    (rlen <= 64) and its two forms as (CAP, QW)."""
    halves = re.search(r"int onesweep_halves_for\(.*?\n}\n", _source("lsb_kernels.hip"), re.S)
    assert halves, "onesweep_halves_for"
    skew = re.search(r"tot > \(uint64_t\)\(m >> (\d+)\) && tot < \(uint64_t\)m\) return 2;", halves.group(0))
    assert skew, "the 1/32 rule of onesweep_halves_for"
    launch = re.search(r"hipError_t launch_segfix\(.*?\n}\n", _source("lsb_segsort.hip"), re.S)
    assert launch, "launch_segfix"
    rule = re.search(r"rlen = rbits >= 62 \? 0 : m >> rbits;\s*if \(rlen <= (\d+)\)", launch.group(0))
    forms = re.findall(r"k_segfix<((?:\d+ \* )?)kSegCap, \d+, (\d+)>", launch.group(0))
    assert rule and len(forms) == 2, "launch_segfix's two forms"
    cap = constant("kSegCap")
    forms = tuple((int(f.split()[0]) * cap if f else cap, int(q)) for f, q in forms)
    g = Geometry(constant("kTile"), constant("kSegMax"), cap, constant("kOnesweepSubs"), constant("kSegTile"),
                 int(skew.group(1)), int(rule.group(1)), forms)
    assert g.seg_max % 64 == 0 and g.seg_max <= g.seg_tile
    return g


def sub_of_tile(t, TT, subs=None):
    """lsb_ostile.h os_sub_of_tile: the sub-array of tile t of TT."""
    subs = subs or geometry().subs
    return sum(1 for k in range(1, subs) if k * TT <= subs * t + subs - 1)


# ---- lsb_passes.cpp: which bytes, and whether the hybrid is taken
def varying_mask(keys):
    """The key bits that differ somewhere (the span read: OR of the keys and
    OR of their complements)."""
    keys = np.ascontiguousarray(keys, dtype=U)
    return int(np.bitwise_or.reduce(keys)) & int(np.bitwise_or.reduce(~keys))


def varying_bytes(varying):
    return [b for b in range(8) if (varying >> (8 * b)) & 0xFF]


def hybrid_bytes(varying, m):
    """The fewest top varying bytes whose varying bits reach ceil(log2 m)."""
    need = 0
    while (1 << need) < m:
        need += 1
    top, bits = [], 0
    for b in range(7, -1, -1):
        if bits >= need:
            break
        v = (varying >> (8 * b)) & 0xFF
        if not v:
            continue
        top.insert(0, b)
        bits += bin(v).count("1")
    return top


Plan = collections.namedtuple("Plan", "varying digits msd hybrid skewed constant")


def plan(keys, skip=True, geo=None):
    """LocalSort::queue for one rank whose first pass is not regional (fewer
    than 3 guessed top bytes, i.e. at most 2^16 records, or the option off):
    the LSD digits, the hybrid's bytes, and whether the hybrid is taken
    (fewer bytes than digits, first byte neither skewed nor constant)."""
    geo = geo or geometry()
    m = keys.size
    varying = varying_mask(keys) if skip else (1 << 64) - 1
    digits = varying_bytes(varying)
    msd = hybrid_bytes(varying, m)
    hybrid = len(msd) < len(digits)
    skewed = constant_ = False
    if hybrid and msd:
        tot = np.bincount(_byte(keys, msd[0]), minlength=256)
        skewed = bool(np.any((tot > (m >> geo.skew_shift)) & (tot < m)))
        constant_ = bool(np.any(tot == m))
        if skewed or constant_:
            hybrid = False
    return Plan(varying, digits, msd, hybrid, skewed, constant_)


def _masks(msd):
    pmask = U(sum(0xFF << (8 * b) for b in msd))
    return pmask, pmask & ~U(0xFF << (8 * msd[-1]))


# ---- k_onesweep SEG (seg_pos)
def fused_pass(x, last, pmask, T, seg_max, stale=None, cut_slots=True):
    """k_onesweep SEG on x (stably sorted by the lower top bytes), tile by
    tile -> (out, bit2, segs).  A record of the bucket-ordered stage walks its
    segment at most seg_max records each way: [max(s, klo), j) back and
    (j, min(e, khi)) on, klo = max(j - seg_max, 0), khi = min(j + 1 + seg_max,
    nvalid), [s, e) its segment's stage slots.  Bit 2: a back walk that
    reaches klo > 0 inside the segment (s <= klo), or a forward walk that
    reaches khi < nvalid inside it (e >= khi); so a walk that ends at the
    stage's first or last slot is complete and reports nothing.  A segment of
    seg_max + 1 records reports from one of its two end records wherever it
    lies in a stage longer than itself.  segs: (tile, first stage slot,
    records) of every segment of 2 or more.  Records whose walks are cut take
    the cut walks' slots (they may collide; the later stage record wins here,
    any of them on the device); cut_slots=False leaves them out of `out`,
    for a caller that drops the output of a pass with bit 2 anyway."""
    m = x.size
    keys = x["key"]
    d = _byte(keys, last)
    pm = keys & pmask
    counts = np.bincount(d, minlength=256)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    seen = np.zeros(256, dtype=np.int64)
    out = stale.copy() if stale is not None else np.zeros(m, dtype=x.dtype)
    bit2 = False
    segs = []
    for ti, t0 in enumerate(range(0, m, T)):
        idx = np.arange(t0, min(t0 + T, m))
        st = idx[np.argsort(d[idx], kind="stable")]
        sk, sp, sd = keys[st], pm[st], d[st]
        nv = st.size
        j = np.arange(nv)
        brk = np.ones(nv, dtype=bool)
        brk[1:] = sp[1:] != sp[:-1]
        starts = np.flatnonzero(brk)
        sid = np.cumsum(brk) - 1
        s = starts[sid]
        e = np.append(starts[1:], nv)[sid]
        klo = np.maximum(j - seg_max, 0)
        khi = np.minimum(j + 1 + seg_max, nv)
        walks = e - s > 1
        bit2 |= bool(np.any(walks & (((s <= klo) & (klo > 0)) | ((e >= khi) & (khi < nv)))))
        pos = np.empty(nv, dtype=np.int64)
        pos[np.lexsort((sk, sid))] = j  # the segment's first slot + stable rank, where no walk is cut
        cut = walks & ((s < klo) | (e > khi))
        for jj in np.flatnonzero(cut) if cut_slots else ():
            lo_, hi_ = max(s[jj], klo[jj]), min(e[jj], khi[jj])
            v = sk[jj]
            w = sk[lo_:jj]
            pos[jj] = lo_ + int((w < v).sum()) + int((sk[jj + 1:hi_] < v).sum()) + int((w == v).sum())
        lstart = np.searchsorted(sd, sd, "left")
        slot = base[sd] + seen[sd] + (pos - lstart)
        ok = (slot >= 0) & (slot < m) & (cut_slots | ~cut)
        out[slot[ok]] = x[st[ok]]
        seen += np.bincount(sd, minlength=256)
        ln = np.diff(np.append(starts, nv))
        segs.extend((ti, int(a_), int(n_)) for a_, n_ in zip(starts[ln > 1], ln[ln > 1]))
    return out, bit2, segs


# ---- k_segfix
def segfix_form(m, k, geo=None):
    """launch_segfix: (CAP, QW) from the records per run value, m over the
    2^(8 (k - 1)) values of the run bytes."""
    geo = geo or geometry()
    rbits = 8 * (k - 1)
    rlen = 0 if rbits >= 62 else m >> rbits
    return geo.forms[0] if rlen <= geo.rlen_max else geo.forms[1]


def segfix(x, out, msd, T, cap, subs=8):
    """k_segfix over the fused pass's input x and output `out` -> (out, bit1,
    rows); one row per boundary whose two records share a run: t, b, a, c (the
    run's records before / from b inside the two tiles), nm (records of the
    buckets present on both sides), cause (None, or "a", "c", "span", "nm":
    the first test of the kernel's that reports), and the sub-arrays of the
    two tiles.  The kernel counts a and c on past CAP only until they exceed
    it; they are exact here."""
    out = out.copy()
    m = x.size
    pmask, rmask = _masks(msd)
    keys = x["key"]
    rk = keys & rmask
    d = _byte(keys, msd[-1])
    counts = np.bincount(d, minlength=256)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    brk = np.ones(m, dtype=bool)
    brk[1:] = rk[1:] != rk[:-1]
    starts = np.flatnonzero(brk)
    rid = np.cumsum(brk) - 1
    rs, re_ = starts[rid], np.append(starts[1:], m)[rid]
    TT = -(-m // T)
    upto = np.cumsum(np.bincount(np.arange(m) // T * 256 + d, minlength=TT * 256).reshape(TT, 256), axis=0)
    rows, bit1 = [], False
    for t in range(TT - 1):
        b = (t + 1) * T
        lo, hi = t * T, min(b + T, m)
        if rk[b] != rk[b - 1]:
            continue
        a_ = b - max(rs[b], lo)
        c_ = min(re_[b], hi) - b
        cl = np.bincount(d[b - a_:b], minlength=256)
        cr = np.bincount(d[b:b + c_], minlength=256)
        both = (cl > 0) & (cr > 0)
        nm = int((cl + cr)[both].sum())
        cause = None
        if a_ > cap:
            cause = "a"
        elif c_ > cap:
            cause = "c"
        elif (b - a_ == lo and lo > 0 and rk[lo - 1] == rk[b]) or (b + c_ == hi and hi < m and rk[hi] == rk[b]):
            cause = "span"
        elif nm > cap:
            cause = "nm"
        rows.append(dict(t=t, b=b, a=int(a_), c=int(c_), nm=nm, cause=cause, two_sided=int(both.sum()),
                         one_sided=int(((cl > 0) ^ (cr > 0)).sum()),
                         subs=(sub_of_tile(t, TT, subs), sub_of_tile(t + 1, TT, subs))))
        if cause:
            bit1 = True
            continue
        run = np.arange(b - a_, b + c_)
        for dd in np.flatnonzero(both):
            rec = run[d[run] == dd]  # input order: tile t's records first
            P = base[dd] + int(upto[t, dd])  # the end of tile t's bucket-dd block
            o = np.argsort(keys[rec], kind="stable")
            out[P - cl[dd] + np.arange(rec.size)] = x[rec[o]]
    return out, bit1, rows


# ---- k_segsort
def segsort(y, pmask, T, seg_max):
    """k_segsort over y (stably sorted by pmask; its segments in any order)
    -> (out, err, rows), one row per tile of T records: w0 (the tile's first
    segment start, nvalid without one), w1 (the end of its last segment, past
    the tile by the tail), tail, and which of the kernel's tests report:
      tail   wave 0 reads the records after the tile 64 at a time, seg_max at
             the most, and reports when none of them starts a segment: a tail
             of seg_max records or more (also for a tile that owns nothing);
      back   an owned record li with li - seg_max > w0 whose seg_max
             predecessors all share its segment (go && jlo > w0);
      fwd    one with li + 1 + seg_max < w1 whose seg_max successors all do
             (go && jhi < w1).
    This is laxer than "a segment over seg_max records" (segsort_model, and
    the comment at the head of lsb_segsort.hip) in exactly one kind of input:
    a segment of seg_max + 1 records that is the whole owned range, starting
    at w0 and ending at w1 (alone in the last tile, or from a tile's only
    start to the end of its tail).  Its last record's walk back ends at
    jlo = w0 and its first record's walk on at jhi = w1, so neither reports;
    with one record more, or a start after w0, or an end before w1, one of
    the two end records reports.  Every walk is then complete
    and the output exact.  out: every segment stably sorted by key (valid
    when err is False: then every walk was complete)."""
    m = y.size
    p = y["key"] & pmask
    brk = np.ones(m, dtype=bool)
    brk[1:] = p[1:] != p[:-1]
    starts = np.flatnonzero(brk)
    sid = np.cumsum(brk) - 1
    gs, ge = starts[sid], np.append(starts[1:], m)[sid]
    KB = T + seg_max
    rows, err = [], False
    for ti, tb in enumerate(range(0, m, T)):
        nv = min(T, m - tb)
        last = tb + T >= m
        st = np.flatnonzero(brk[tb:tb + nv])
        w0 = int(st[0]) if st.size else nv
        bad_tail = False
        tail = 0
        if last:
            w1 = nv
        else:
            tail = int(ge[tb + T - 1]) - (tb + T)  # records after the tile in its last record's segment
            if tail < seg_max:
                w1 = T + tail
            else:
                bad_tail = True
                w1 = T + seg_max
        w1 = min(w1, KB)
        bad_back = bad_fwd = False
        if w0 < nv:
            li = np.arange(w0, w1)
            g = tb + li
            s = gs[g] - tb
            e = np.minimum(ge[g] - tb, w1)
            bad_back = bool(np.any((li - seg_max > w0) & (li - s >= seg_max)))
            bad_fwd = bool(np.any((li + 1 + seg_max < w1) & (e >= li + 1 + seg_max)))
        rows.append(dict(tile=ti, w0=w0, w1=w1, tail=tail, bad_tail=bad_tail, bad_back=bad_back, bad_fwd=bad_fwd))
        err |= bad_tail or bad_back or bad_fwd
    out = y[np.lexsort((y["key"], sid))]
    return out, err, rows


# ---- the whole sort
Sorted = collections.namedtuple("Sorted", "out route passes shifts plan detail")


def hybrid_sort(a, mode, skip=True, geo=None):
    """One rank's sort with LSB_OPT_HYBRID = mode (1 or 2), stage split 0 ->
    Sorted(out, route, passes, shifts, plan, detail).  route: "direct" (the
    hybrid is not taken: the LSD passes at once), "fused" (mode 1, no error
    bit), "segsort" (k_segsort finished it) or "lsd" (the LSD passes over the
    kept input after an error).  passes is lsb_get_last_sort's count, shifts
    the per-pass shifts of lsb_get_pass_stats (64: a k_segsort pass)."""
    geo = geo or geometry()
    pl = plan(a["key"], skip, geo)
    want = a[np.argsort(a["key"], kind="stable")]
    lsd = [8 * b for b in pl.digits]
    if not pl.hybrid:
        return Sorted(want, "direct", len(pl.digits), lsd, pl, {})
    msd = pl.msd
    k = len(msd)
    shifts = [8 * b for b in msd]
    pmask, _ = _masks(msd)
    x = a
    for b in msd[:-1]:
        x = x[np.argsort(_byte(x["key"], b), kind="stable")]
    detail = {"x": x}
    if mode == 1:
        cap, qw = segfix_form(a.size, k, geo)
        y, bit2, segs = fused_pass(x, msd[-1], pmask, geo.tile, geo.seg_max, cut_slots=False)
        y, bit1, rows = segfix(x, y, msd, geo.tile, cap, geo.subs)
        detail.update(cap=cap, qw=qw, bit1=bit1, bit2=bit2, segfix=rows, stage_segs=segs)
        if not bit1 and not bit2:
            return Sorted(y, "fused", k, shifts, pl, detail)
        if bit2:  # no permutation: the LSD passes over the kept input
            return Sorted(want, "lsd", k + len(lsd), shifts + lsd, pl, detail)
    else:
        y = x[np.argsort(_byte(x["key"], msd[-1]), kind="stable")]
    detail["y"] = y
    out, err, rows = segsort(y, pmask, geo.seg_tile, geo.seg_max)
    detail.update(segsort=rows, segsort_err=err)
    if not err:
        return Sorted(out, "segsort", k + 1, shifts + [64], pl, detail)
    return Sorted(want, "lsd", k + 1 + len(lsd), shifts + [64] + lsd, pl, detail)


def longest_segment(y, pmask, T):
    """(tile, position in the tile, records) of the longest segment of y, a
    block sorted by pmask, by the tile its first record lies in."""
    p = y["key"] & pmask
    brk = np.ones(y.size, dtype=bool)
    brk[1:] = p[1:] != p[:-1]
    starts = np.flatnonzero(brk)
    ln = np.diff(np.append(starts, y.size))
    i = int(np.argmax(ln))
    return int(starts[i] // T), int(starts[i] % T), int(ln[i])


# ------------------------------------------------------------ the inputs
# The last pass's input is the block stably sorted by the run byte (k = 2:
# byte 6), so the records per run value fix every run's position in it.  An
# input is a list of "case" runs, each at a chosen position with chosen
# last-pass bytes and low bits per record, padded by short runs of the other
# run values with random bytes below.
Case = collections.namedtuple("Case", "name a expect")

RUN_BYTE, LAST_BYTE = 6, 7
DUP_POOL = 9  # distinct low parts a case run draws from: duplicate whole keys


def build(m, runs, seed, zeros=None):
    """m records whose last-pass input holds, for every (v, pos, recs) of
    `runs`, run value v at positions [pos, pos + len(recs)), recs a list of
    (last-pass byte, low 48 bits); every other run value pads the gaps evenly
    with random records.  zeros = (v, q): the pad runs below run value v hold
    exactly q records of last-pass byte 0x00 between them and every other pad
    record a non-zero one, so that the records (v, 0x00) start at position q
    of the block sorted by both bytes.  The records come in a random
    interleaving of the runs that keeps each run's order; val = the input
    position."""
    rng = np.random.default_rng(seed)
    runs = sorted(runs)
    limit = m >> geometry().skew_shift
    count = np.zeros(256, dtype=np.int64)
    edges = [(-1, 0)] + [(v, pos) for v, pos, _ in runs] + [(256, m)]
    ends = [0] + [pos + len(recs) for _, pos, recs in runs]
    for (v0, _), (v1, p1), p0 in zip(edges[:-1], edges[1:], ends):
        vals = np.arange(v0 + 1, v1)
        gap = p1 - p0
        assert gap >= 0 and (gap == 0 or vals.size), (v0, v1, gap)
        if vals.size:
            count[vals] = gap // vals.size
            count[vals[:gap % vals.size]] += 1
    for v, _, recs in runs:
        count[v] = len(recs)
    assert count.sum() == m and count[0] > 0 and count[255] > 0 and count.max() <= limit, (count.max(), limit)
    case = {v: recs for v, _, recs in runs}
    b6 = np.repeat(np.arange(256), count)
    b7 = rng.integers(0, 256, m)
    low = rng.integers(0, 1 << 48, m, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    if zeros:
        zv, q = zeros
        pads = [u for u in range(zv) if u not in case]
        z = np.zeros(256, dtype=np.int64)
        z[pads] = q // len(pads)
        z[pads[:q % len(pads)]] += 1
        assert np.all(z <= count) and z.max() <= geometry().seg_max
        b7 = rng.integers(1, 256, m)
        for u in pads:
            b7[first[u]:first[u] + z[u]] = 0
    for v, recs in case.items():
        b7[first[v]:first[v] + len(recs)] = [r[0] for r in recs]
        low[first[v]:first[v] + len(recs)] = [r[1] for r in recs]
    x = np.zeros(m, dtype=DT)
    x["key"] = (b7.astype(U) << U(56)) | (b6.astype(U) << U(48)) | low.astype(U)
    a = np.zeros(m, dtype=DT)
    a[np.argsort(rng.permutation(b6), kind="stable")] = x  # a random interleaving of the runs
    a["val"] = np.arange(m, dtype=U)
    return a


def _lows(rng, n):
    pool = rng.integers(0, 1 << 48, DUP_POOL, dtype=np.int64)
    return pool[rng.integers(0, DUP_POOL, n)].tolist()


def _run_value(pos, m):
    return int(min(254, max(1, round(255 * pos / m))))


BUCKETS = [0x00, 0xFF, 0x3C, 0x81, 0x17, 0xE2, 0x5A, 0xA5, 0x08, 0xF7, 0x66, 0x99, 0x2D, 0xD2, 0x4B, 0xB4,
           0x01, 0xFE, 0x3D, 0x80, 0x16, 0xE3, 0x5B, 0xA4, 0x09, 0xF6, 0x67, 0x98, 0x2C, 0xD3, 0x4A, 0xB5, 0x70, 0x8F]


def crossing_recs(a, c, seed, nb=None, shift=1):
    """A run of a + c records: the a before the boundary cycle through nb
    last-pass bytes, the c after it through nb bytes `shift` further on, so
    (with both sides of nb records or more) `shift` bytes are left-only,
    `shift` right-only and the others on both sides; low parts from a pool of
    DUP_POOL, so whole keys repeat on both sides and within a side.  nb keeps
    a tile's part of a segment at 33 records or fewer."""
    rng = np.random.default_rng(seed)
    nb = nb or max(4, -(-max(a, c) // 32))
    assert nb + shift <= len(BUCKETS)
    b7 = [BUCKETS[(i + 1) % nb] for i in range(a)] + [BUCKETS[shift + (i + 1 - shift) % nb] for i in range(c)]
    low = _lows(rng, a + c)
    assert b7[0] == b7[a]
    low[a] = low[0]  # a whole key on both sides of the boundary, whatever the pool gave
    return list(zip(b7, low))


def segment_recs(n, byte, seed, extra=(0x33, 0xC4, 0x33, 0x52, 0xC4, 0x6B)):
    """n records of one last-pass byte (a segment) with a few of other bytes
    spread through them; low parts from a pool of DUP_POOL."""
    rng = np.random.default_rng(seed)
    b7 = [byte] * n
    for i, e in enumerate(extra):
        b7.insert((i + 1) * n // (len(extra) + 1) + i, e)
    return list(zip(b7, _lows(rng, len(b7))))


def m_small():
    """3 tiles and 1000 records: k = 2, and launch_segfix's 256-record form."""
    T = geometry().tile
    return 3 * T + 1000


def m_large():
    """16 tiles: k = 2 still, runs of 256 records on average: the 1024-record form."""
    return 16 * geometry().tile


def crossing_case(name, m, t, a, c, seed, **kw):
    """A run with a records before and c from the boundary of tiles t, t + 1."""
    T = geometry().tile
    b = (t + 1) * T
    recs = crossing_recs(a, c, seed, **kw)
    v = 255 if b + c == m else _run_value(b - a, m)
    return Case(name, build(m, [(v, b - a, recs)], seed), dict(t=t, a=a, c=c))


CROSS_256 = [(1, 1), (63, 1), (64, 1), (65, 1), (1, 64), (1, 65), (64, 64), (256, 1), (257, 1), (1, 256), (1, 257)]
NM_CASES = [(128, 128), (128, 129), (160, 160)]  # over 8 bytes, all on both sides: nm = a + c
LARGE_A = [255, 256, 257, 1024, 1025]
IN_TILE = [63, 64, 65, 129]
SPLITS = [(64, 64), (64, 1), (1, 64)]
SEGSORT_STARTS = [1, 63, 64]  # the segment starts at tile position T - this
SEGSORT_TAILS = [63, 64, 65]


@functools.lru_cache(maxsize=None)
def cases():
    """Every constructed input, as Case(name, records, expect); expect holds
    what the input was built to be, which tests/test_hybrid_model.py asserts
    from the model's own account of it."""
    g = geometry()
    T, out = g.tile, []
    ms, ml = m_small(), m_large()
    assert g.forms[0][0] == g.seg_cap and segfix_form(ms, 2) == g.forms[0] and segfix_form(ml, 2) == g.forms[1]
    for i, (a, c) in enumerate(CROSS_256):
        out.append(crossing_case("cross256_%d_%d" % (a, c), ms, 1, a, c, 100 + i))
    for i, (a, c) in enumerate(NM_CASES):
        cs = crossing_case("nm_%d_%d" % (a, c), ms, 1, a, c, 200 + i, nb=8, shift=0)
        out.append(cs._replace(expect=dict(cs.expect, nm=a + c)))
    for i, a in enumerate(LARGE_A):
        out.append(crossing_case("cross1024_%d_3" % a, ml, 4, a, 3, 300 + i))  # tiles 4 | 5: one sub-array
    # where the boundary lies.  (A crossing run whose left part starts at its
    # tile's first record, k_segfix's `b - a == lo` test, would hold a = kTile
    # records of one run value: over CAP in both forms, and over the skew
    # rule's m / 32 at every size up to 16 tiles, where the hybrid is not
    # taken.  The model keeps the test, which nothing reaches while CAP < kTile.)
    cs = crossing_case("place_sub_boundary", ml, 1, 40, 40, 400)  # tiles 1 | 2: sub-arrays 0 | 1
    out.append(cs._replace(expect=dict(cs.expect, subs_differ=True)))
    mp = 3 * T + 37
    cs = crossing_case("place_last_partial", mp, 2, 20, 37, 401)  # c reaches m
    out.append(cs._replace(expect=dict(cs.expect, c_reaches_m=True)))
    # segments inside one tile (tile 1), three stage placements
    for i, n in enumerate(IN_TILE):
        recs = segment_recs(n, 0x00, 500 + i)
        out.append(Case("intile_first_%d" % n, build(ms, [(_run_value(T, ms), T, recs)], 500 + i),
                        dict(stage=(1, 0, n))))
        recs = segment_recs(n, 0x81, 510 + i)
        out.append(Case("intile_middle_%d" % n, build(ms, [(_run_value(T + 2000, ms), T + 2000, recs)], 510 + i),
                        dict(stage=(1, None, n))))
        recs = segment_recs(n, 0xFF, 520 + i)
        pos = 2 * T - len(recs)
        out.append(Case("intile_last_%d" % n, build(ms, [(_run_value(pos, ms), pos, recs)], 520 + i),
                        dict(stage=(1, T - n, n))))
    # a segment split by the boundary of tiles 1 | 2
    for i, (l, r) in enumerate(SPLITS):
        b7 = [x[0] for x in segment_recs(l, 0x81, 0, extra=(0x33, 0xC4, 0x33)) +
              segment_recs(r, 0x81, 0, extra=(0xC4, 0x52, 0x52))]
        recs = list(zip(b7, _lows(np.random.default_rng(600 + i), len(b7))))  # one pool for both sides
        a = l + 3
        left = [j for j in range(a) if b7[j] == 0x81]
        right = [j for j in range(a, len(b7)) if b7[j] == 0x81]
        recs[right[0]] = (0x81, recs[left[0]][1])  # a whole key of the segment on both sides
        out.append(Case("split_%d_%d" % (l, r), build(ms, [(_run_value(2 * T - a, ms), 2 * T - a, recs)], 600 + i),
                        dict(t=1, a=a, c=r + 3, split=(l, r))))
    # k_segsort's tiles: the segment (run v, byte 0x00) at position T - back of
    # the block sorted by both bytes, with `tail` records past the tile
    for i, back in enumerate(SEGSORT_STARTS):
        for j, tail in enumerate(SEGSORT_TAILS):
            n = back + tail
            recs = segment_recs(n, 0x00, 700 + 3 * i + j, extra=(0x33, 0xC4))
            v = 160
            out.append(Case("segsort_back%d_tail%d" % (back, tail),
                            build(ms, [(v, 2 * T + 300, recs)], 700 + 3 * i + j, zeros=(v, T - back)),
                            dict(ysegment=(0, T - back, n), tail=tail)))
    n = g.seg_max + 1
    recs = list(zip([0xFF] * n, _lows(np.random.default_rng(800), n)))
    out.append(Case("segsort_whole_last_tile", build(3 * T + n, [(255, 3 * T, recs)], 800),
                    dict(ysegment=(3, 0, n), stage=(3, 0, n), whole_last_tile=True)))
    recs = list(zip([0xFF] * 10, _lows(np.random.default_rng(801), 10)))
    recs[9] = recs[0]  # the last tile's one record repeats a key of the tile before
    out.append(Case("segsort_tile_without_start", build(3 * T + 1, [(255, 3 * T - 9, recs)], 801),
                    dict(t=2, a=9, c=1, c_reaches_m=True, ysegment=(2, T - 9, 10), tail=1, no_start_tile=3)))
    return tuple(out)


# Thinned and crowded keys of tools/stress_mix.py (imported, not restated):
# (kind, seed, n), chosen on the CPU by the model's routes.  Mode 1 takes the
# fused route, or the LSD passes after bit 2; mode 2 k_segsort, or the LSD
# passes after its error; some skip the hybrid (a skewed first byte).  Mode
# 1's third route, k_segsort after bit 1 alone, needs a crossing run over CAP
# whose segments all stay within kSegMax: none of 4000 thinned draws at these
# sizes had one (a byte thinned to a few values makes long segments too, and
# those set bit 2); the constructed inputs above take it.
THINNED = (("thinned", 61, 20011), ("thinned", 65, 24576), ("thinned", 73, 33333), ("thinned", 80, 12289),
           ("thinned", 104, 40000), ("thinned", 107, 28673), ("thinned", 128, 36864), ("thinned", 3346, 24576),
           ("thinned", 3625, 13000), ("thinned", 1, 20011), ("thinned", 2, 16384), ("crowded", 1, 12289),
           ("crowded", 2, 40000))


def stress_keys(kind, seed, n):
    tools = os.path.join(ROOT, "tools")
    pkg = os.path.join(ROOT, "distributed-lsb_amd")
    for p in (pkg, tools):
        if p not in sys.path:
            sys.path.insert(0, p)
    import stress_mix
    rng = random.Random(seed)
    return stress_mix.crowded_keys(rng, n) if kind == "crowded" else stress_mix.thinned_keys(rng, n)


@functools.lru_cache(maxsize=None)
def thinned_cases():
    return tuple(Case("%s_seed%d_n%d" % t, stress_keys(*t), {}) for t in THINNED)


@functools.lru_cache(maxsize=None)
def predicted(name):
    """{mode: Sorted} of the input of that name, computed once per process."""
    cs = {c.name: c for c in cases() + thinned_cases()}[name]
    return {mode: hybrid_sort(cs.a, mode) for mode in (1, 2)}
