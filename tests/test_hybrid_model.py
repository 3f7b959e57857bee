"""CPU model of the hybrid local sort's mode 1 (LSB_OPT_HYBRID = 1), at small
tile sizes so that every boundary case shows up in a few thousand records.

It restates the data flow of distributed-lsb_amd/csrc (k_onesweep with SEG,
then k_segfix) with numpy and checks it against the stable sort by key, the
reference's output (mpi/mpi_lsbsort.cpp:580-585, verified at :722-737):

  1. stable passes on the k top bytes but the last;
  2. the last pass, tile by tile: each tile's bucket-d block goes to the
     bucket's next slots (the look-back), and inside the block every segment
     (records equal on the k bytes) is ordered by the whole key;
  3. k_segfix, per tile boundary b: the run of records equal on the k - 1
     run bytes that crosses b is found in the last pass's input as
     [b - a, b + c); for every bucket present on both sides, its records are
     re-placed, stably, at P - (left count) + rank, where P is the end of
     tile t's bucket block (look-back value + bucket base);
  4. a run longer than the cap on one side, or one spanning a whole tile,
     is reported (the runtime then runs k_segsort).

The GPU tests (tests/test_hybrid_gpu.py) check the kernels; this checks the
algorithm they implement, including the cases the GPU sizes rarely reach.

The model itself, and the inputs built for the kernels' limits at the shipped
geometry, are in tests/hybrid_model.py; the second half of this file holds
them to their stated conditions and to the stable sort.
"""
import numpy as np
import pytest

import hybrid_model as hm
from hybrid_model import (DT, _keys, _seed19_like, fused_pass_model, hybrid_mode1, hybrid_model,  # noqa: F401
                          segfix_bit1, segsort_model)


@pytest.mark.parametrize("n,T,run_values", [(3000, 64, 150), (5000, 128, 100), (4096, 64, None),
                                            (2047, 32, 400), (6000, 256, 60)])
def test_model_matches_stable_sort(n, T, run_values):
    """Runs of ~10-100 records (a few to ~half a tile) and uniform keys; most
    draws stay under the cap, and every one that does is exact."""
    done = 0
    for seed in range(6):
        rng = np.random.default_rng(seed * 1000 + n)
        a = _keys(rng, n, run_values)
        want = a[np.argsort(a["key"], kind="stable")]
        out, ok = hybrid_model(a, [5, 6, 7], T, cap=T // 2)
        if ok:
            assert np.array_equal(out, want), seed
            done += 1
    assert done >= 4


def test_model_duplicates_across_tiles():
    """Equal keys split between tiles: the left tile's records come first."""
    rng = np.random.default_rng(3)
    n = 4000
    a = np.zeros(n, dtype=DT)
    pool = rng.integers(0, 2**64 - 1, 300, dtype=np.uint64)
    a["key"] = pool[rng.integers(0, pool.size, n)]
    a["val"] = np.arange(n, dtype=np.uint64)
    out, ok = hybrid_model(a, [5, 6, 7], 128, cap=64)
    assert ok
    assert np.array_equal(out, a[np.argsort(a["key"], kind="stable")])


def test_model_reports_runs_past_the_cap():
    """A run of one run-key value over the cap on a side is reported, never
    silently mis-sorted."""
    rng = np.random.default_rng(4)
    a = _keys(rng, 4096, run_values=2)  # ~2048-record runs
    _, ok = hybrid_model(a, [5, 6, 7], 64, cap=32)
    assert not ok


# ---- the fused pass's segment walk and the error dispatch
# The model above orders every in-tile segment exactly.  The kernel does not:
# each record walks its segment in the stage at most kSegMax records each way
# (k_onesweep SEG, csrc/lsb_kernels.hip, the write-out's walk), and a segment
# longer than that inside a tile gets slots from cut walks, which can collide:
# the pass then sets error bit 2 and its output is no permutation (duplicates,
# and holes keeping whatever the buffer held).  k_segfix sets bit 1 for a
# crossing run it leaves alone, whose output IS a permutation.  The runtime's
# dispatch (LocalSort::finish, csrc/lsb_passes.cpp): no bit -> done; bit 1
# alone -> k_segsort over the pass's output; bit 2 -> the LSD passes over the
# kept input.  Before d4f7b64 every error took k_segsort, which is how stress
# seed 19 kept a wrong sort.


def test_pre_fix_dispatch_keeps_a_wrong_sort_shipped_does_not():
    """Segments of ~250 records, ~128 of them inside a 256-record tile, with
    the walk cut at 16: the fused pass's slots collide (bit 2).  The
    pre-d4f7b64 dispatch hands that output to k_segsort, whose runs the stale
    records in the holes cut short, and keeps a wrong sort for some inputs;
    the shipped dispatch re-sorts the kept input exactly every time."""
    msd = [4, 6, 7]
    wrong_pre = 0
    for seed in range(6):
        rng = np.random.default_rng(1900 + seed)
        a = _seed19_like(rng, 8000, v4=8)
        want = a[np.argsort(a["key"], kind="stable")]
        stale = _keys(np.random.default_rng(seed), a.size)  # what the pass's buffer held
        stale["val"] += np.uint64(10**9)
        out, route = hybrid_mode1(a, msd, 256, 16, 128, stale, "shipped")
        assert route == "lsd" and np.array_equal(out, want), seed
        out, route = hybrid_mode1(a, msd, 256, 16, 128, stale, "pre_d4f7b64")
        if not np.array_equal(out, want):
            assert route == "segsort"  # the wrong answer came through k_segsort
            assert np.unique(out["val"]).size < out.size or out["val"].max() >= 10**9  # no permutation
            wrong_pre += 1
    assert wrong_pre >= 2  # the round-5 bug, reproduced by the model (3 of these 6 inputs)


def test_dispatch_exact_across_the_cap():
    """Small tiles (32-256 records) and segments on both sides of the walk's
    cut (16): bytes 5 and 6 from a pool (runs of ~seg_len records), byte 7
    from two values (a segment holds ~seg_len / 2 records) or uniform (short
    segments, long crossing runs for k_segfix).  Every route of
    the shipped dispatch -- the fused output, k_segsort after bit 1, the LSD
    passes after bit 2 -- ends in the stable sort, bit for bit, and the grid
    reaches all three."""
    msd = [5, 6, 7]
    routes = {}
    for T in (32, 64, 128, 256):
        for seg_len in (8, 24, 48, 96, 192):
            for seed, two in ((0, True), (1, False)):
                rng = np.random.default_rng(seed * 7919 + T + seg_len)
                n = 3000 + seed * 333
                a = _keys(rng, n, run_values=max(1, n // seg_len))
                if two:
                    a["key"] = (a["key"] & ~np.uint64(0xFF << 56)) | \
                        (rng.choice(np.array([0x11, 0xEE], dtype=np.uint64), n) << np.uint64(56))
                want = a[np.argsort(a["key"], kind="stable")]
                stale = _keys(np.random.default_rng(seed + 99), n)
                out, route = hybrid_mode1(a, msd, T, 16, T // 2, stale, "shipped")
                routes.setdefault(route, []).append((T, seg_len))
                assert np.array_equal(out, want), (T, seg_len, seed, route)
    assert set(routes) == {"fused", "segsort", "lsd"}, {k: len(v) for k, v in routes.items()}


# ---- the model at the shipped geometry (tests/hybrid_model.py) ----------------
# The vectorised functions against the per-record loops above at toy geometry,
# then every constructed input against what it was built to be.


def _stable(a):
    return a[np.argsort(a["key"], kind="stable")]


@pytest.mark.parametrize("T,seg_len,two", [(32, 8, False), (64, 24, True), (64, 48, True), (128, 96, True),
                                           (256, 192, False), (256, 48, True)])
def test_vectorised_kernels_equal_the_loops(T, seg_len, two):
    """fused_pass (slots of cut walks, collisions and stale holes included),
    segfix and the routes of the vectorised model equal the per-record loops
    on inputs with segments on both sides of the walk's cut."""
    msd, seg_max, cap = [5, 6, 7], 16, T // 2
    pmask, _ = hm._masks(msd)
    for seed in range(3):
        rng = np.random.default_rng(seed * 131 + T + seg_len)
        n = 3000 + 77 * seed
        a = _keys(rng, n, run_values=max(1, n // seg_len))
        if two:
            a["key"] = (a["key"] & ~np.uint64(0xFF << 56)) | \
                (rng.choice(np.array([0x11, 0xEE], dtype=np.uint64), n) << np.uint64(56))
        stale = _keys(np.random.default_rng(seed + 99), n)
        x = a
        for b in msd[:-1]:
            x = x[np.argsort(hm._byte(x["key"], b), kind="stable")]
        slow, bit2_slow = fused_pass_model(x, 7, pmask, T, seg_max, stale)
        fast, bit2, _ = hm.fused_pass(x, 7, pmask, T, seg_max, stale)
        assert bit2 == bit2_slow and np.array_equal(fast, slow)
        fixed, bit1, rows = hm.segfix(x, fast, msd, T, cap)
        # (the loops lack the kernel's third cause, over CAP records to re-place)
        assert bit1 == any(r["cause"] for r in rows)
        assert segfix_bit1(x, msd, T, cap) == any(r["cause"] in ("a", "c", "span") for r in rows)
        if not bit2 and not any(r["cause"] == "nm" for r in rows):
            want, ok = hybrid_model(a, msd, T, cap)
            assert ok == (not bit1) and np.array_equal(fixed, want)


def test_geometry_comes_from_the_sources():
    g = hm.geometry()
    assert g.forms[0] == (g.seg_cap, 1) and g.forms[1][0] > g.seg_cap and g.forms[1][1] * 64 <= g.forms[1][0]
    assert g.tile % 64 == 0 and g.seg_tile % 64 == 0 and g.seg_max % 64 == 0 and g.subs == 8
    assert [hm.sub_of_tile(t, 16) for t in range(16)] == [t // 2 for t in range(16)]
    assert [hm.sub_of_tile(t, 4) for t in range(4)] == [1, 3, 5, 7]
    # lsb_passes.cpp hybrid_bytes: uniform keys take 2 top bytes up to 2^16 records, 3 beyond
    full = (1 << 64) - 1
    assert hm.hybrid_bytes(full, 1 << 16) == [6, 7] and hm.hybrid_bytes(full, (1 << 16) + 1) == [5, 6, 7]
    assert hm.hybrid_bytes(full, 256) == [7] and hm.hybrid_bytes(full & ~(0xFF << 48), 1000) == [5, 7]


F, S, L1, L2 = ("fused", 2), ("segsort", 3), ("lsd", 10), ("lsd", 11)
# (route, passes) of modes 1 and 2, per input; every input not named: (F, S),
# the fused route in k = 2 passes and k_segsort as the third.
ROUTES = {
    "cross256_257_1": (S, S), "cross256_1_257": (S, S),  # a, c over the 256-record form's CAP: bit 1
    "nm_128_129": (S, S), "nm_160_160": (S, S),          # 257 and 320 records to re-place: bit 1
    "cross1024_1025_3": (S, S),                          # a over the 1024-record form's CAP
    # 64 + 64, 64 + 1, 1 + 64: k_segfix merges what each tile ordered; k_segsort meets 128 or 65 records
    "split_64_64": (F, L2), "split_64_1": (F, L2), "split_1_64": (F, L2),
}
for _n in (65, 129):  # a segment over kSegMax inside a tile: bit 2 in mode 1, k_segsort's error in mode 2
    for _w in ("first", "middle", "last"):
        ROUTES["intile_%s_%d" % (_w, _n)] = (L1, L2)
for _b in hm.SEGSORT_STARTS:  # all but the 64-record segment (1 + 63) are over kSegMax
    for _t in hm.SEGSORT_TAILS:
        if _b + _t > 64:
            ROUTES["segsort_back%d_tail%d" % (_b, _t)] = (L1, L2)

CASE_NAMES = [c.name for c in hm.cases()]


def test_every_listed_case_is_there():
    g = hm.geometry()
    assert (g.tile, g.seg_max, g.seg_cap, g.forms[1][0]) == (4096, 64, 256, 1024), \
        "the limits moved: the (a, c), nm and segment lists of tests/hybrid_model.py name the old ones"
    assert set(ROUTES) <= set(CASE_NAMES) and len(set(CASE_NAMES)) == len(CASE_NAMES)
    for a, c in [(1, 1), (63, 1), (64, 1), (65, 1), (1, 64), (1, 65), (64, 64), (256, 1), (257, 1), (1, 256), (1, 257)]:
        assert "cross256_%d_%d" % (a, c) in CASE_NAMES
    for a in (255, 256, 257, 1024, 1025):
        assert "cross1024_%d_3" % a in CASE_NAMES
    for n in (63, 64, 65, 129):
        for w in ("first", "middle", "last"):
            assert "intile_%s_%d" % (w, n) in CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_constructed_input(name):
    """The input is what it was built to be (every condition from the model's
    own account of the kernels' counts), takes the stated route in the stated
    passes in both modes, and the model's output is the stable sort."""
    g = hm.geometry()
    T = g.tile
    cs = {c.name: c for c in hm.cases()}[name]
    a, ex = cs.a, cs.expect
    m = a.size
    keys = a["key"]
    r1, r2 = hm.predicted(name)[1], hm.predicted(name)[2]
    # the hybrid is taken, with k = 2 of 8 digits; the run byte is not skewed
    assert 3 * T < m <= 16 * T
    assert r1.plan.hybrid and r1.plan.msd == [6, 7] and r1.plan.digits == list(range(8))
    assert r1.plan.varying == (1 << 64) - 1
    for b in (6, 7):
        assert {0x00, 0xFF} <= set(np.unique(hm._byte(keys, b)).tolist())
    assert np.bincount(hm._byte(keys, 6), minlength=256).max() <= m >> g.skew_shift
    assert np.array_equal(a["val"], np.arange(m, dtype=np.uint64))
    want = _stable(a)
    assert np.array_equal(r1.out, want) and np.array_equal(r2.out, want)
    assert ((r1.route, r1.passes), (r2.route, r2.passes)) == ROUTES.get(name, (F, S))
    k, nd = 2, 8
    assert r1.shifts == {"fused": [48, 56], "segsort": [48, 56, 64],
                         "lsd": [48, 56] + [8 * i for i in range(nd)]}[r1.route]
    assert r2.shifts == ([48, 56, 64] if r2.route == "segsort" else [48, 56, 64] + [8 * i for i in range(nd)])
    assert r1.passes == len(r1.shifts) and r2.passes == len(r2.shifts) and k == len(r1.plan.msd)
    d = r1.detail
    x = d["x"]
    pmask, _ = hm._masks([6, 7])
    cap = d["cap"]
    assert (cap, d["qw"]) == (g.forms[0] if (m >> 8) <= g.rlen_max else g.forms[1])
    assert cap == (1024 if name.startswith(("cross1024", "place_sub")) else 256)
    longest = max(n for _, _, n in d["stage_segs"])
    rows = {r["t"]: r for r in d["segfix"]}
    if "t" in ex:
        row = rows[ex["t"]]
        b = row["b"]
        assert (row["a"], row["c"]) == (ex["a"], ex["c"]) and b == (ex["t"] + 1) * T
        if "nm" in ex:
            assert row["nm"] == ex["nm"] and row["one_sided"] == 0
        cause = "a" if ex["a"] > cap else "c" if ex["c"] > cap else "nm" if row["nm"] > cap else None
        assert row["cause"] == cause and d["bit1"] == (cause is not None)
        assert all(r["cause"] is None for t, r in rows.items() if t != ex["t"])  # the only boundary that reports
        assert row["two_sided"] >= 1
        if name.startswith("cross") and max(ex["a"], ex["c"]) >= 63:
            assert row["one_sided"] >= 1  # some buckets on one side only
        # a whole key on both sides of the boundary: the left tile's copies must come first
        left, right = x["key"][b - row["a"]:b], x["key"][b:b + row["c"]]
        assert np.intersect1d(left, right).size >= 1
        assert row["subs"] == (hm.sub_of_tile(ex["t"], -(-m // T)), hm.sub_of_tile(ex["t"] + 1, -(-m // T)))
        if name.startswith("cross1024"):
            assert row["subs"][0] == row["subs"][1]
        if ex.get("subs_differ") or cap == 256:
            assert row["subs"][0] != row["subs"][1]
        if ex.get("c_reaches_m"):
            assert b + row["c"] == m and m % T != 0
        if "stage" not in ex and "ysegment" not in ex:
            assert longest <= g.seg_max and not d["bit2"]
    else:
        assert not d["bit1"]
    if "split" in ex:
        l, r = ex["split"]
        segs = d["stage_segs"]
        assert (ex["t"], l) in {(t, n) for t, _, n in segs} or l == 1
        assert (ex["t"] + 1, r) in {(t, n) for t, _, n in segs} or r == 1
        assert hm.longest_segment(r2.detail["y"], pmask, g.seg_tile)[2] == l + r
        assert rows[ex["t"]]["nm"] >= l + r
    if "stage" in ex:
        tile, first, n = ex["stage"]
        hit = [s for s in d["stage_segs"] if s[2] == longest]
        assert longest == n and len(hit) == 1 and hit[0][0] == tile
        nvalid = min(T, m - tile * T)
        if first is None:
            assert 0 < hit[0][1] and hit[0][1] + n < nvalid
        else:
            assert hit[0][1] == first and (first == 0 or first + n == nvalid)
        assert d["bit2"] == (n > g.seg_max and n < nvalid)
    if "ysegment" in ex:
        y = r2.detail["y"]
        assert hm.longest_segment(y, pmask, g.seg_tile) == ex["ysegment"]
        tile, start, n = ex["ysegment"]
        srow = r2.detail["segsort"][tile]
        if "tail" in ex:
            assert srow["tail"] == ex["tail"] == start + n - g.seg_tile
            assert srow["bad_tail"] == (ex["tail"] >= g.seg_max)
            assert srow["w0"] == 0 or tile > 0
        if ex.get("whole_last_tile"):
            # laxer than "longer than kSegMax": the 65 records are the owned range, every walk ends at its end
            assert n == g.seg_max + 1 and (srow["w0"], srow["w1"]) == (0, n) and tile == len(r2.detail["segsort"]) - 1
            assert not r2.detail["segsort_err"] and segsort_model(y, pmask, g.seg_max)[1]
        if "no_start_tile" in ex:
            nrow = r2.detail["segsort"][ex["no_start_tile"]]
            assert nrow["w0"] == m - ex["no_start_tile"] * g.seg_tile == 1 and not r2.detail["segsort_err"]
    # a segment's keys repeat (the pool of low parts): ties are ranked by input position
    assert np.unique(keys).size < m


def test_split_segment_is_fused_in_mode_1_and_redone_in_mode_2():
    """64 + 64 records of one segment around a tile boundary: each tile's part
    is within kSegMax, so the fused pass orders both and k_segfix merges them
    (no limit but CAP on the merged records); k_segsort sees 128 records of
    one segment and reports them, and mode 2 runs the LSD passes."""
    r = hm.predicted("split_64_64")
    assert (r[1].route, r[1].passes) == ("fused", 2) and (r[2].route, r[2].passes) == ("lsd", 2 + 1 + 8)
    assert not r[1].detail["bit1"] and not r[1].detail["bit2"] and r[2].detail["segsort_err"]


THINNED_NAMES = [c.name for c in hm.thinned_cases()]


def test_thinned_and_crowded_keys_cover_the_routes():
    """tools/stress_mix.py's host-made keys at the listed seeds: the model's
    output is the stable sort on every route, and every route a mode can take
    on them is taken by at least two seeds (mode 1: fused, the LSD passes
    after bit 2; mode 2: k_segsort, the LSD passes after its error; both: the
    hybrid skipped).  Mode 1's k_segsort route is the constructed inputs'."""
    assert 11 <= len(THINNED_NAMES) <= 13
    routes = {1: {}, 2: {}}
    for cs in hm.thinned_cases():
        assert 12289 <= cs.a.size <= 40000
        want = _stable(cs.a)
        for mode in (1, 2):
            r = hm.predicted(cs.name)[mode]
            assert np.array_equal(r.out, want), (cs.name, mode)
            assert r.passes == len(r.shifts)
            routes[mode].setdefault(r.route, []).append(cs.name)
    assert {k: len(v) >= 2 for k, v in routes[1].items()} == {"fused": True, "lsd": True, "direct": True}, routes[1]
    assert {k: len(v) >= 2 for k, v in routes[2].items()} == {"segsort": True, "lsd": True, "direct": True}, routes[2]
    assert {r for mode in routes for r in routes[mode]} >= {"fused", "segsort", "lsd"}
