// Host check of the edge passes' tile decisions (lsb_ostile.h: os_edge_applies,
// os_pass_tile, os_pass_tiles_ok, os_rows_track1/2) against brute force over
// small sorts, and of the k_onesweep instance table (kOsInstances, os_select).
// Stand-alone: plain C++, no device.  tests/test_edgetile_host.py builds it
// with the host sanitizers and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lsb_ostile.h"

static int failures = 0;
#define CHECK(cond, what)                                            \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (++failures < 20) fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, what); \
    }                                                                \
  } while (0)

constexpr int kRegions = 256 * lsb::kOnesweepSubs;

static int sub_by_definition(int64_t t, int64_t TT) {
  for (int x = 0; x < lsb::kOnesweepSubs; ++x)
    if (lsb::os_sub_first_tile(x, TT) <= t && t < lsb::os_sub_first_tile(x + 1, TT)) return x;
  return -1;
}

// The most next-pass sub-array boundaries strictly inside any run of at most
// t consecutive output slots of m records, the next pass taking tn per tile.
static int most_boundaries_in_a_run(int64_t m, int t, int tn) {
  const int64_t TTn = lsb::os_tiles(m, tn);
  std::vector<int64_t> b;  // slots s whose sub-array differs from slot s - 1's
  for (int64_t s = 1; s < m; ++s)
    if (sub_by_definition(s / tn, TTn) != sub_by_definition((s - 1) / tn, TTn)) b.push_back(s);
  int most = 0;
  for (size_t i = 0; i < b.size(); ++i) {
    // a run [R, R + t) with R < b[i] holds boundary b[i] and those up to R + t - 1 at most b[i] + t - 2
    int k = 0;
    for (size_t j = i; j < b.size() && b[j] <= b[i] + t - 2; ++j) ++k;
    most = std::max(most, k);
  }
  return most;
}

int main() {
  const int small = 4096, big = lsb::kOsEdgeTile;
  // Small stand-ins for the two sizes keep the slot-by-slot search cheap:
  // the rule is arithmetic in (t, tn, m) alone.
  const int ts[] = {4, 5, 8, 10};
  for (int t : ts)
    for (int tn : ts)
      for (int64_t m = 1; m <= 40 * 10; ++m) {
        const int most = most_boundaries_in_a_run(m, t, tn);
        if (lsb::os_tile_fits(t, tn, m)) CHECK(most <= 1, "an admitted (t, tn, m): a run crosses at most one boundary");
      }
  // At the real sizes: wherever os_edge_applies admits an edge pass, every
  // seam of the sort's eight passes fits (first -> layout is regional: whole
  // regions per sub-array whatever either pass's tile, checked below), and
  // the instance table has it.
  for (int64_t m = 1; m <= 200000; m += 97)
    for (int64_t cap : {int64_t(0), int64_t(4096), int64_t(12288), int64_t(20480), int64_t(40960)})
      for (unsigned setting = 0; setting < 8; ++setting)
        for (int mid : {0, 4096, 4608, 5120}) {
          const unsigned e = lsb::os_edge_applies(m, cap, setting, mid, small);
          CHECK((e & ~(setting & lsb::kOsEdgeAll)) == 0, "only what the setting names");
          if (mid != big || !lsb::os_big_applies(m, big, small)) CHECK(e == 0, "no edge pass without large middle passes");
          {
            // The runtime's tile rule against the same model by hand, for every
            // pass of the eight (and a sort of whole records: 4096 throughout).
            const int midt = mid > small && lsb::os_big_applies(m, mid, small) ? mid : small;
            int want[8];
            want[0] = e & lsb::kOsEdgeFirst ? big : small;
            want[1] = e & lsb::kOsEdgeLayout ? big : small;
            for (int i = 2; i < 7; ++i) want[i] = midt;
            want[7] = e & lsb::kOsEdgeLast ? big : small;
            for (int i = 0; i < 8; ++i) {
              const lsb::OsPassKind pass = i == 0 ? lsb::kOsPassFirst : i == 1 ? lsb::kOsPassLayout : i == 7 ? lsb::kOsPassLast : lsb::kOsPassMiddle;
              CHECK(lsb::os_pass_tile(pass, true, m, cap, mid, setting, small) == want[i], "the tile rule: a packed sort's pass");
              CHECK(lsb::os_pass_tile(pass, false, m, cap, mid, setting, small) == small, "the tile rule: whole records");
            }
            CHECK(lsb::os_pass_tile(lsb::kOsPassOther, true, m, cap, mid, setting, small) == small, "the tile rule: any other pass");
          }
          if (!e) continue;
          if (e & lsb::kOsEdgeLayout) CHECK(cap > 0 && cap % big == 0, "the layout in whole large tiles");
          int tile[8];
          tile[0] = e & lsb::kOsEdgeFirst ? big : small;
          tile[1] = e & lsb::kOsEdgeLayout ? big : small;
          for (int i = 2; i < 7; ++i) tile[i] = big;
          tile[7] = e & lsb::kOsEdgeLast ? big : small;
          for (int i = 1; i < 7; ++i) CHECK(lsb::os_tile_fits(tile[i], tile[i + 1], m), "every seam fits");
          CHECK(lsb::os_pass_tiles_ok(lsb::kOsPassFirst, tile[0], tile[1], small), "first pass instance");
          CHECK(lsb::os_pass_tiles_ok(lsb::kOsPassLayout, tile[1], tile[2], small), "layout pass instance");
          for (int i = 2; i < 7; ++i) CHECK(lsb::os_pass_tiles_ok(lsb::kOsPassMiddle, tile[i], tile[i + 1], small), "middle instance");
          CHECK(lsb::os_pass_tiles_ok(lsb::kOsPassLast, tile[7], small, small), "last pass instance");
        }
  // The seams at the real tile sizes by the slot search, around the bound.
  for (int64_t m : {int64_t(61440), int64_t(61441), int64_t(65536), int64_t(81921), int64_t(100003)})
    for (int t : {4096, 5120})
      for (int tn : {4096, 5120})
        if (lsb::os_tile_fits(t, tn, m)) CHECK(most_boundaries_in_a_run(m, t, tn) <= 1, "real sizes: at most one boundary");
  // The table refuses what has no instance.
  CHECK(!lsb::os_pass_tiles_ok(lsb::kOsPassFirst, 4608, small, small), "no 4608 first pass");
  CHECK(!lsb::os_pass_tiles_ok(lsb::kOsPassLayout, big, small, small) && !lsb::os_pass_tiles_ok(lsb::kOsPassLayout, 4608, 4608, small),
        "the layout's pass: 5120 -> 5120 or 4096");
  CHECK(!lsb::os_pass_tiles_ok(lsb::kOsPassLast, 4608, small, small), "no 4608 last pass");
  CHECK(!lsb::os_pass_tiles_ok(lsb::kOsPassOther, big, small, small) && !lsb::os_pass_tiles_ok(lsb::kOsPassOther, small, big, small),
        "every other instance keeps 4096");
  CHECK(lsb::os_pass_tiles_ok(lsb::kOsPassMiddle, big, small, small) && !lsb::os_pass_tiles_ok(lsb::kOsPassMiddle, big, 4608, small),
        "a middle pass: its own size next, or 4096");
  // The instance table (kOsInstances): no two rows equal, and every row is
  // the one os_select gives the request that reached that instantiation in
  // the if-ladder launch_onesweep used to be (the list below is that ladder,
  // arm by arm, not the table).
  for (int i = 0; i < lsb::kOsInstanceCount; ++i)
    for (int j = i + 1; j < lsb::kOsInstanceCount; ++j) CHECK(!(lsb::kOsInstances[i] == lsb::kOsInstances[j]), "no two rows equal");
  {
    struct Arm {
      int rm;
      bool pin, pout;
      int shift, next_shift;
      bool c16, seg, gather, totals;
      int halves, tile, next_tile;
      lsb::OsInstance row;
    };
    const bool T = true, F = false;
    const Arm arms[] = {
        // the regional first pass: packing in large tiles (any next tile), packing, whole records
        {1, F, T, 0, 8, F, F, F, F, 1, 5120, 4096, {512, 10, T, F, 1, F, F, 1, F, T, 5120}},
        {1, F, T, 0, 8, F, F, F, F, 1, 0, 5120, {512, 8, T, F, 1, F, F, 1, F, T, 4096}},
        {1, F, F, 0, 8, F, F, F, F, 1, 0, 0, {512, 8, T, F, 1, F, F, 1, F, F, 4096}},
        // the pass that reads the layout: packed (large; before 5120, 4608, 4096), whole records (next digit or none)
        {2, T, T, 8, 16, F, F, F, F, 1, 5120, 5120, {512, 10, T, F, 1, F, F, 2, T, T, 5120}},
        {2, T, T, 8, 16, F, F, F, F, 1, 0, 5120, {512, 8, T, F, 1, F, F, 2, T, T, 5120}},
        {2, T, T, 8, 16, F, F, F, F, 1, 0, 4608, {512, 8, T, F, 1, F, F, 2, T, T, 4608}},
        {2, T, T, 8, 16, F, F, F, F, 1, 0, 0, {512, 8, T, F, 1, F, F, 2, T, T, 4096}},
        {2, F, F, 8, 16, F, F, F, F, 1, 0, 0, {512, 8, T, F, 1, F, F, 2, F, F, 4096}},
        {2, F, F, 8, -1, F, F, F, F, 1, 0, 0, {512, 8, F, F, 1, F, F, 2, F, F, 4096}},
        // a packed sort's middle passes
        {0, T, T, 16, 24, F, F, F, F, 1, 5120, 5120, {512, 10, T, F, 1, F, F, 0, T, T, 5120}},
        {0, T, T, 16, 24, F, F, F, F, 1, 5120, 0, {512, 10, T, F, 1, F, F, 0, T, T, 4096}},
        {0, T, T, 16, 24, F, F, F, F, 1, 4608, 4608, {512, 9, T, F, 1, F, F, 0, T, T, 4608}},
        {0, T, T, 16, 24, F, F, F, F, 1, 4608, 0, {512, 9, T, F, 1, F, F, 0, T, T, 4096}},
        {0, T, T, 16, 24, F, F, F, F, 1, 0, 0, {512, 8, T, F, 1, F, F, 0, T, T, 4096}},
        // its last pass: no next digit, whatever next_tile says
        {0, T, F, 56, -1, F, F, F, F, 1, 5120, 4608, {512, 10, F, F, 1, F, F, 0, T, F, 5120}},
        {0, T, F, 56, -1, F, F, F, F, 1, 0, 0, {512, 8, F, F, 1, F, F, 0, T, F, 4096}},
        // the hybrid's last pass (with totals)
        {0, F, F, 32, -1, F, T, F, T, 1, 0, 0, {512, 8, F, F, 1, T, F, 0, F, F, 4096}},
        // the 16-bit counts (halves = 2 still runs the whole stage), gathered or not
        {0, F, F, 8, -1, T, F, F, T, 2, 0, 0, {512, 8, F, T, 1, F, F, 0, F, F, 4096}},
        {0, F, F, 8, -1, T, F, T, T, 1, 0, 0, {512, 8, F, T, 1, F, T, 0, F, F, 4096}},
        // the next digit: split, plain, gathered
        {0, F, F, 0, 8, F, F, F, F, 2, 0, 0, {256, 16, T, F, 2, F, F, 0, F, F, 4096}},
        {0, F, F, 0, 8, F, F, F, T, 1, 0, 0, {512, 8, T, F, 1, F, F, 0, F, F, 4096}},
        {0, F, F, 0, 8, F, F, T, F, 1, 0, 0, {512, 8, T, F, 1, F, T, 0, F, F, 4096}},
        // no next digit: split, plain, gathered
        {0, F, F, 56, -1, F, F, F, F, 2, 0, 0, {256, 16, F, F, 2, F, F, 0, F, F, 4096}},
        {0, F, F, 56, -1, F, F, F, T, 1, 0, 0, {512, 8, F, F, 1, F, F, 0, F, F, 4096}},
        {0, F, F, 56, -1, F, F, T, F, 1, 0, 0, {512, 8, F, F, 1, F, T, 0, F, F, 4096}},
    };
    const int narms = (int)(sizeof arms / sizeof arms[0]);
    CHECK(narms == lsb::kOsInstanceCount, "as many rows as the ladder had instantiations");
    std::vector<int> hits(lsb::kOsInstanceCount, 0);
    auto request = [](const Arm& a) {
      lsb::OsRequest q;
      q.m = int64_t(1) << 20;
      q.region_mode = a.rm;
      q.pack_in = a.pin;
      q.pack_out = a.pout;
      q.shift = a.shift;
      q.next_shift = a.next_shift;
      q.count16 = a.c16;
      q.seg = a.seg;
      q.gather = a.gather;
      q.totals = a.totals;
      q.halves = a.halves;
      q.tile = a.tile;
      q.next_tile = a.next_tile;
      return q;
    };
    for (const Arm& a : arms) {
      const int row = lsb::os_select(request(a));
      CHECK(row >= 0 && lsb::kOsInstances[row] == a.row, "a ladder arm's request selects that arm's instance");
      if (row >= 0) ++hits[row];
    }
    for (int h : hits) CHECK(h == 1, "every row reached by exactly one arm");
    // The placement probe: the plain next-counting row.
    lsb::OsRequest probe = request(arms[20]);
    probe.totals = false;
    probe.probe = true;
    CHECK(lsb::os_select(probe) == lsb::os_select(request(arms[20])), "the probe selects the plain next-counting row");
    // What the ladder refused is still refused: each request is an arm above with one thing changed.
    auto refused = [&](int arm, auto change) {
      lsb::OsRequest q = request(arms[arm]);
      change(q);
      return lsb::os_select(q) < 0;
    };
    CHECK(refused(13, [](lsb::OsRequest& q) { q.next_tile = 5120; }), "no middle pass 4096 -> 5120");
    CHECK(refused(3, [](lsb::OsRequest& q) { q.next_tile = 0; }), "no layout pass 5120 -> 4096");
    CHECK(refused(0, [](lsb::OsRequest& q) { q.tile = 4608; }), "no 4608 first pass");
    CHECK(refused(3, [](lsb::OsRequest& q) { q.tile = q.next_tile = 4608; }) && refused(3, [](lsb::OsRequest& q) { q.tile = 4608, q.next_tile = 0; }),
          "no 4608 layout pass");
    CHECK(refused(14, [](lsb::OsRequest& q) { q.tile = 4608; }), "no 4608 last pass");
    for (int arm : {2, 7, 8, 16, 17, 19, 20, 21, 22, 23, 24}) {
      CHECK(refused(arm, [](lsb::OsRequest& q) { q.tile = 5120; }), "no large tile without packed records");
      CHECK(refused(arm, [](lsb::OsRequest& q) { q.next_tile = 5120; }), "no large next tile without packed records");
    }
    for (int arm : {17, 19, 22}) CHECK(refused(arm, [](lsb::OsRequest& q) { q.halves = 2, q.gather = true; }), "split + gathered");
    CHECK(refused(16, [](lsb::OsRequest& q) { q.next_shift = 40; }), "seg with a next digit");
    CHECK(refused(17, [](lsb::OsRequest& q) { q.shift = 7; }) && refused(18, [](lsb::OsRequest& q) { q.shift = 0; }), "count16 with shift < 8");
    CHECK(refused(17, [](lsb::OsRequest& q) { q.next_shift = 16; }), "count16 with a next digit");
    CHECK(refused(23, [](lsb::OsRequest& q) { q.pack_out = true; }), "only the regional first pass packs");
    CHECK(refused(20, [](lsb::OsRequest& q) { q.probe = true, q.next_shift = -1; }) && refused(21, [](lsb::OsRequest& q) { q.probe = true; }) &&
              refused(19, [](lsb::OsRequest& q) { q.probe = true; }),
          "the probe: a next digit, whole stage, not gathered");
    CHECK(refused(1, [](lsb::OsRequest& q) { q.next_tile = 1234; }) && refused(1, [](lsb::OsRequest& q) { q.next_shift = -1; }),
          "the first pass: a built next tile, a next digit");
    for (int arm : {0, 3, 9, 14}) {
      CHECK(refused(arm, [](lsb::OsRequest& q) { q.totals = true; }) && refused(arm, [](lsb::OsRequest& q) { q.halves = 2; }) &&
                refused(arm, [](lsb::OsRequest& q) { q.gather = true; }) && refused(arm, [](lsb::OsRequest& q) { q.seg = true; }) &&
                refused(arm, [](lsb::OsRequest& q) { q.count16 = true; }) && refused(arm, [](lsb::OsRequest& q) { q.probe = true; }),
            "a regional or packed pass: nothing else set");
    }
    CHECK(refused(10, [](lsb::OsRequest& q) { q.m = 61440; }) && !refused(10, [](lsb::OsRequest& q) { q.m = 61441; }), "the seam 5120 -> 4096 from 61,441 records on");
    CHECK(refused(23, [](lsb::OsRequest& q) { q.region_mode = 3; }) && refused(23, [](lsb::OsRequest& q) { q.halves = 3; }), "unknown modes");
  }
  // The layout's sub-arrays are 256 whole regions whatever tile divides cap:
  // the first pass's counts do not depend on the tile of the pass that reads it.
  for (int64_t cap : {int64_t(20480), int64_t(40960), int64_t(532480)})
    for (int t : {small, big}) {
      const int64_t TT = lsb::os_rows_track2(cap, t, kRegions);
      CHECK(TT * t == cap * kRegions, "whole tiles cover the layout");
      for (int x = 0; x <= lsb::kOnesweepSubs; ++x)
        CHECK(lsb::os_sub_first_tile(x, TT) * t == (int64_t)x * 256 * cap, "sub-array x starts at region 256 x");
    }
  // Rows of either track against a count of the tiles.
  for (int64_t m = 1; m < 30000; m += 37)
    for (int t : {small, 4608, big}) {
      int64_t n = 0;
      for (int64_t s = 0; s < m; s += t) ++n;
      CHECK(lsb::os_rows_track1(m, t) == n, "track 1: tiles of the m records");
    }
  CHECK(lsb::os_rows_track2(532480, big, kRegions) == 104 * 2048 && lsb::os_rows_track2(532480, small, kRegions) == 130 * 2048,
        "track 2 at 2^30 records");
  if (failures) {
    fprintf(stderr, "edge tile host check: %d failure(s)\n", failures);
    return 1;
  }
  printf("edge tile host check: ok\n");
  return 0;
}
