// Host check of the edge passes' tile decisions (lsb_ostile.h: os_edge_applies,
// os_pass_tiles_ok, os_rows_track1/2) against brute force over small sorts.
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
