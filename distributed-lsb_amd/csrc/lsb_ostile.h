// k_onesweep's tile geometry where passes of different tile sizes meet: the
// sub-arrays a pass counts the next digit by, when a larger tile applies, and
// which look-back rows to refill.  Plain arithmetic, shared by the kernels
// (lsb_kernels.hip), the runtime (lsb_passes.cpp) and the host checks
// (tools/host_asan.cpp): no HIP types.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSB_HD __host__ __device__
#else
#define LSB_HD
#endif

namespace lsb {

// A pass's records are tiles in kOnesweepSubs contiguous sub-arrays:
// sub-array x holds tiles [x * TT / 8, (x + 1) * TT / 8) of its TT tiles.
constexpr int kOnesweepSubs = 8;

LSB_HD inline int64_t os_tiles(int64_t m, int t) { return (m + t - 1) / t; }
LSB_HD inline int64_t os_sub_first_tile(int x, int64_t TT) { return (int64_t)x * TT / kOnesweepSubs; }
// Sub-array of tile t without a division: the number of x in 1..7 with
// x * TT <= 8 * t + 7, i.e. floor(x * TT / 8) <= t (32-bit exact: TT < 2^22).
LSB_HD inline int os_sub_of_tile(int64_t t, int64_t TT) {
  const uint32_t num = (uint32_t)kOnesweepSubs * (uint32_t)t + (uint32_t)(kOnesweepSubs - 1), tt = (uint32_t)TT;
  int x = 0;
  for (int k = 1; k < kOnesweepSubs; ++k) x += num >= (uint32_t)k * tt ? 1 : 0;
  return x;
}

// A bucket's run of one tile, output slots [R, R + cnt) with cnt <= the
// tile's records, staged from tile position lstart on, among the next pass's
// TTn tiles of tn records over mcap slots: it lies in next-pass sub-array x0,
// except from stage position jb on (x1) when it crosses a sub-array boundary.
// Packed as jb | x0 << 16 | x1 << 24; jb = 0xFFFF: never.  At most one
// boundary is crossed where os_tile_fits holds.
LSB_HD inline uint32_t os_run_cut(int64_t R, uint32_t cnt, uint32_t lstart, int tn, int64_t TTn, int64_t mcap) {
  const int x0 = os_sub_of_tile(R / tn, TTn);
  const int64_t bnd = x0 + 1 < kOnesweepSubs ? os_sub_first_tile(x0 + 1, TTn) * tn : mcap;
  if (R + cnt > bnd) {
    const int x1 = os_sub_of_tile(bnd / tn, TTn);
    return (uint32_t)(lstart + (bnd - R)) | ((uint32_t)x0 << 16) | ((uint32_t)x1 << 24);
  }
  return 0xFFFFu | ((uint32_t)x0 << 16) | ((uint32_t)x0 << 24);
}

// A run of at most t records may cross at most one boundary of the next
// pass's sub-arrays, so every non-empty sub-array that a run can cover whole
// and go on past must hold at least t records.  A non-empty sub-array holds
// at least max(1, TTn / 8) tiles, and only the last tile is short: it lies in
// sub-array 7, where no run goes on.  Hence tn * max(1, TTn / 8) >= t: always
// true for t <= tn; for t = 5120 over tn = 4096 from 16 tiles (61,441
// records) on.
LSB_HD inline bool os_tile_fits(int t, int tn, int64_t m) {
  const int64_t per = os_tiles(m, tn) / kOnesweepSubs;
  return (int64_t)tn * (per > 1 ? per : 1) >= t;
}
// The runtime's rule for a sort of m records whose other passes take `small`
// records per tile: the large tile only when it fits beside them (the seams
// before the first and after the last large-tile pass) and beside itself.
LSB_HD inline bool os_big_applies(int64_t m, int big, int small) {
  return big > small && os_tile_fits(big, small, m) && os_tile_fits(big, big, m) && os_tile_fits(small, big, m);
}

// A packed sort's edge passes (the packing first pass, the pass that reads
// the regional layout and the last pass) take the large tile too, each when
// its bit of the context's setting is on.
constexpr unsigned kOsEdgeFirst = 1u, kOsEdgeLayout = 2u, kOsEdgeLast = 4u;
constexpr unsigned kOsEdgeAll = kOsEdgeFirst | kOsEdgeLayout | kOsEdgeLast;
constexpr int kOsEdgeTile = 5120;  // the only large tile the edge instances are built at
// Which edge passes of a packed sort of m records over regions of `cap` slots
// take `big` records per tile, where its middle passes do (big = 0: they do
// not, nor does any edge pass).  The layout's tile k of a region is that
// region's slots [k * big, (k + 1) * big), so whole tiles must fill `cap`.
// The first pass writes regions, which no run crosses, whatever its tile;
// every other seam is one os_big_applies already admits (small -> big,
// big -> big, big -> small).
LSB_HD inline unsigned os_edge_applies(int64_t m, int64_t cap, unsigned setting, int big, int small) {
  if (big != kOsEdgeTile || !os_big_applies(m, big, small)) return 0u;
  unsigned e = setting & kOsEdgeAll;
  if (cap <= 0 || cap % big != 0) e &= ~kOsEdgeLayout;
  return e;
}
// The kinds of pass launch_onesweep tells apart by tile size, and the
// (kind, t, tn) combinations it has instances for: t records per tile, the
// next pass's tn (ignored by a pass that counts no next digit).
enum OsPassKind { kOsPassOther = 0, kOsPassFirst, kOsPassLayout, kOsPassMiddle, kOsPassLast };
LSB_HD inline bool os_pass_tiles_ok(OsPassKind kind, int t, int tn, int small) {
  const bool any_t = t == small || t == 4608 || t == kOsEdgeTile;
  const bool any_tn = tn == small || tn == 4608 || tn == kOsEdgeTile;
  switch (kind) {
    case kOsPassFirst: return (t == small || t == kOsEdgeTile) && any_tn;  // regions: tn does not enter its counts
    case kOsPassLayout: return (t == small && any_tn) || (t == kOsEdgeTile && tn == kOsEdgeTile);
    case kOsPassMiddle: return any_t && (tn == t || tn == small);
    case kOsPassLast: return t == small || t == kOsEdgeTile;
    default: return t == small && tn == small;
  }
}
// Look-back rows a launch writes: the first track's, over the m records, and
// the second track's (the pass that reads the regional layout), over the
// layout's slots.
LSB_HD inline int64_t os_rows_track1(int64_t m, int t) { return os_tiles(m, t); }
LSB_HD inline int64_t os_rows_track2(int64_t cap, int t, int regions) { return cap / t * regions; }

// Look-back rows shared by launches of different tile counts.  Invariant:
// after a launch of `rows` tiles at epoch e, the rows below `rows` carry e's
// parity and the rows from there on are untrusted (an earlier, longer launch
// left them with either parity).  A launch of more tiles than the one before
// on that buffer first fills rows [first, first + count) with `word`, whose
// parity is the opposite of the coming epoch's, so the launch can take none
// of them for a row of its own (not 0: that reads as an even epoch's
// aggregate).
struct StatusFill {
  int64_t first = 0, count = 0;  // rows
  uint32_t word = 0;
};
inline StatusFill status_fill(int64_t prev_rows, int64_t now_rows, uint32_t epoch) {
  StatusFill f;
  if (now_rows > prev_rows) {
    f.first = prev_rows;
    f.count = now_rows - prev_rows;
    f.word = ((epoch & 1u) ^ 1u) << 31;
  }
  return f;
}

}  // namespace lsb
