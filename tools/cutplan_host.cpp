// Host check of k_onesweep's cut plans (lsb_ostile.h: os_cut_plan, os_cut,
// os_cut_words) against os_run_cut, word for word, over small geometries
// searched exhaustively on a grid around every next-pass sub-array boundary.
// Stand-alone: plain C++, no device.  tests/test_cutplan_host.py builds it
// with the host sanitizers and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lsb_ostile.h"

static long failures = 0, checked = 0, generals = 0, straddles = 0;
#define CHECK(cond, what)                                                                          \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      if (++failures < 20) fprintf(stderr, "FAIL %s:%d %s (tn %d m %lld base %lld len %lld)\n", __FILE__, __LINE__, what, \
                                   g_tn, (long long)g_m, (long long)g_base, (long long)g_len);    \
    }                                                                                              \
  } while (0)
static int g_tn;
static int64_t g_m, g_base, g_len;

// Sub-array of tile t by the definition: the x whose tiles [x TT / 8, (x + 1) TT / 8) hold it.
static int sub_by_definition(int64_t t, int64_t TT) {
  for (int x = 0; x < lsb::kOnesweepSubs; ++x)
    if (lsb::os_sub_first_tile(x, TT) <= t && t < lsb::os_sub_first_tile(x + 1, TT)) return x;
  return lsb::kOnesweepSubs - 1;
}

// One geometry: m output slots, the next pass taking tn records per tile.
static void geometry(int64_t m, int tn) {
  const int64_t TTn = lsb::os_tiles(m, tn), mcap = m;
  g_m = m;
  g_tn = tn;
  // The boundaries: first slots of the non-empty sub-arrays after the first.
  std::vector<int64_t> bnds;
  for (int x = 1; x < lsb::kOnesweepSubs; ++x) {
    const int64_t s = lsb::os_sub_first_tile(x, TTn) * tn;
    if (s > 0 && s < m && (bnds.empty() || bnds.back() != s)) bnds.push_back(s);
  }
  // The grid: both ends, every boundary at -1, 0, +1, and a slot inside each sub-array.
  std::vector<int64_t> grid = {0, m};
  for (size_t i = 0; i < bnds.size(); ++i) {
    for (int d = -1; d <= 1; ++d) grid.push_back(bnds[i] + d);
    grid.push_back((bnds[i] + (i + 1 < bnds.size() ? bnds[i + 1] : m)) / 2);
  }
  std::sort(grid.begin(), grid.end());
  grid.erase(std::unique(grid.begin(), grid.end()), grid.end());
  while (!grid.empty() && grid.back() > m) grid.pop_back();
  const int kMaxTile = 5120;
  for (int64_t base : grid) {
    if (base < 0 || base >= m) continue;
    for (int64_t end : grid) {
      if (end <= base) continue;
      const int64_t len = end - base;
      if (len > (int64_t)0xFFFFFFFFu) continue;  // a bucket's count in a sub-array is a 32-bit word
      g_base = base;
      g_len = len;
      const lsb::OsCutPlan p = lsb::os_cut_plan(base, len, tn, TTn, mcap);
      const lsb::OsCutWords w = lsb::os_cut_words(p, base, (uint32_t)len);
      // The plan against the definitions.
      const auto above = std::upper_bound(bnds.begin(), bnds.end(), base);
      CHECK(p.x0 == sub_by_definition(base / tn, TTn), "x0: the sub-array of slot base");
      CHECK(p.bnd == (above != bnds.end() ? *above : mcap), "bnd: the first boundary above base");
      if (above != bnds.end()) CHECK(p.x1 == sub_by_definition(p.bnd / tn, TTn), "x1: the sub-array that starts at bnd");
      long inside = 0;  // boundaries b with base < b < base + len: those a run of the range can cross
      for (int64_t b : bnds) inside += b > base && b < end ? 1 : 0;
      CHECK(p.general == (inside >= 2), "general: exactly the ranges over two boundaries");
      CHECK(((w.xs & lsb::kOsCutGeneral) != 0) == p.general, "the words carry general");
      if (p.general) {
        ++generals;
        continue;  // such ranges keep calling os_run_cut
      }
      // Every run [R, R + cnt) of the range on the grid, cnt up to the largest tile.
      for (int64_t R : grid) {
        if (R < base || R >= end) continue;
        std::vector<int64_t> cnts = {1, 2, 4095, 4096, 4097, 4607, 4608, 5119, 5120};
        for (int64_t e : grid)
          if (e > R) cnts.push_back(e - R);
        for (int64_t cnt : cnts) {
          if (cnt < 1 || cnt > kMaxTile || R + cnt > end) continue;
          for (uint32_t lstart : {0u, 17u, (uint32_t)(kMaxTile - cnt)}) {
            const uint32_t want = lsb::os_run_cut(R, (uint32_t)cnt, lstart, tn, TTn, mcap);
            const uint32_t a = lsb::os_cut(p, R, (uint32_t)cnt, lstart);
            const uint32_t b = lsb::os_cut(w, (uint32_t)(R - base), (uint32_t)cnt, lstart);
            ++checked;
            straddles += (want & 0xFFFFu) != 0xFFFFu ? 1 : 0;
            CHECK(a == want, "os_cut(plan) == os_run_cut");
            CHECK(b == want, "os_cut(words) == os_run_cut");
            if (a != want || b != want) {
              if (failures < 20)
                fprintf(stderr, "  R %lld cnt %lld lstart %u: want %08x plan %08x words %08x\n", (long long)R,
                        (long long)cnt, lstart, want, a, b);
            }
          }
        }
      }
    }
  }
}

int main() {
  for (int tn : {4096, 4608, 5120}) {
    for (int k = 1; k <= 40; ++k) {
      geometry((int64_t)k * tn, tn);                          // whole tiles
      geometry((int64_t)k * tn - 1, tn);                      // ragged: one short,
      geometry((int64_t)(k - 1) * tn + 1, tn);                // one record in the last tile,
      geometry((int64_t)(k - 1) * tn + 1 + (977 * k) % (tn - 1), tn);  // and somewhere inside it
    }
    geometry(61441, tn);   // the seam sizes of the three tile sizes
    geometry(300007, tn);
  }
  // Beyond 32 bits of slots: the boundary relative to base still fits a word.
  geometry((int64_t(1) << 33) + 12345, 5120);
  CHECK(generals > 0 && straddles > 0, "the search met general ranges and straddling runs");
  if (failures) {
    fprintf(stderr, "cut plan host check: %ld failure(s)\n", failures);
    return 1;
  }
  printf("cut plan host check: ok (%ld runs, %ld straddling, %ld general ranges)\n", checked, straddles, generals);
  return 0;
}
