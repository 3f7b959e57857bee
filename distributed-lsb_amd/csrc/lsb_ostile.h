// k_onesweep's tile geometry where passes of different tile sizes meet: the
// sub-arrays a pass counts the next digit by, when a larger tile applies, and
// which look-back rows to refill; and the table of the instances that are
// built.  Plain arithmetic, shared by the kernels (lsb_kernels.hip), the
// runtime (lsb_passes.cpp) and the host checks (tools/host_asan.cpp,
// tools/edgetile_host.cpp): no HIP types.
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

// os_run_cut's answer hardly depends on the tile: bucket t's runs of one
// sub-array of this pass all lie in the output slots [base, base + len), len
// being the bucket's count in that sub-array, and the next pass's seven
// boundaries fall inside few such ranges.  The plan of a range, made once
// when a workgroup enters the sub-array: x0, the next-pass sub-array of slot
// `base`; bnd, the first next-pass boundary above `base` (mcap past the last
// one); x1, the sub-array that starts at bnd; general: the range goes on past
// a second boundary (a bucket that covers a whole next-pass sub-array), and
// its runs keep calling os_run_cut.
struct OsCutPlan {
  int64_t bnd;
  int x0, x1;
  bool general;
};
LSB_HD inline OsCutPlan os_cut_plan(int64_t base, int64_t len, int tn, int64_t TTn, int64_t mcap) {
  OsCutPlan p;
  p.x0 = os_sub_of_tile(base / tn, TTn);
  p.bnd = p.x0 + 1 < kOnesweepSubs ? os_sub_first_tile(p.x0 + 1, TTn) * tn : mcap;
  p.x1 = os_sub_of_tile(p.bnd / tn, TTn);
  const int64_t bnd2 = p.x1 + 1 < kOnesweepSubs ? os_sub_first_tile(p.x1 + 1, TTn) * tn : mcap;
  p.general = base + len > bnd2;
  return p;
}
// os_run_cut's word for a run [R, R + cnt) of a range whose plan is not
// general: two compares of R against the one boundary.
LSB_HD inline uint32_t os_cut(const OsCutPlan& p, int64_t R, uint32_t cnt, uint32_t lstart) {
  const uint32_t x0 = (uint32_t)p.x0, x1 = (uint32_t)p.x1;
  if (R + cnt <= p.bnd) return 0xFFFFu | (x0 << 16) | (x0 << 24);
  if (R >= p.bnd) return 0xFFFFu | (x1 << 16) | (x1 << 24);
  return (uint32_t)(lstart + (p.bnd - R)) | (x0 << 16) | (x1 << 24);
}
// The plan as the two words a bucket thread keeps: the boundary relative to
// `base` (a run starts at base + excl with excl + cnt <= len < 2^32, so 32
// bits hold it whatever m is) and x0 << 16 | x1 << 24 | general.  A range
// that ends at or before the boundary takes x1 = x0 and rel = 0: every run
// is then "past the boundary", all in x0.
struct OsCutWords {
  uint32_t rel, xs;
};
constexpr uint32_t kOsCutGeneral = 1u;
LSB_HD inline OsCutWords os_cut_words(const OsCutPlan& p, int64_t base, uint32_t len) {
  const bool reach = p.bnd - base < (int64_t)len;  // some run may start, or end, past bnd
  const uint32_t x0 = (uint32_t)p.x0, x1 = reach ? (uint32_t)p.x1 : x0;
  OsCutWords w;
  w.rel = reach ? (uint32_t)(p.bnd - base) : 0u;
  w.xs = (x0 << 16) | (x1 << 24) | (p.general ? kOsCutGeneral : 0u);
  return w;
}
// os_cut from the words: the run starts excl slots into the range.
LSB_HD inline uint32_t os_cut(const OsCutWords& w, uint32_t excl, uint32_t cnt, uint32_t lstart) {
  const uint32_t hi = w.xs & 0xFF000000u, lo = w.xs & 0x00FF0000u;
  if (excl >= w.rel) return 0xFFFFu | (hi >> 8) | hi;
  if (w.rel - excl >= cnt) return 0xFFFFu | lo | (lo << 8);
  return (lstart + (w.rel - excl)) | lo | hi;
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
// The passes of a sort that differ in tile size: a packed sort's first pass
// (into the regional layout), the pass that reads the layout, its middle
// passes (Packed -> Packed) and its last; every other pass is kOsPassOther.
enum OsPassKind { kOsPassOther = 0, kOsPassFirst, kOsPassLayout, kOsPassMiddle, kOsPassLast };
// Records per tile of one pass of a sort of m records whose other passes take
// `small`: `packed_tile` (the context's setting) for the middle passes of a
// packed sort where it fits, and for the edge passes where os_edge_applies
// (cap: slots per region of the layout, 0 without one) and the context's
// `edge_tiles` say so too.
LSB_HD inline int os_pass_tile(OsPassKind pass, bool packed, int64_t m, int64_t cap, int packed_tile,
                               unsigned edge_tiles, int small) {
  if (pass == kOsPassOther || !packed || !os_big_applies(m, packed_tile, small)) return small;
  if (pass == kOsPassMiddle) return packed_tile;
  const unsigned bit = pass == kOsPassFirst ? kOsEdgeFirst : pass == kOsPassLayout ? kOsEdgeLayout : kOsEdgeLast;
  return os_edge_applies(m, cap, edge_tiles, packed_tile, small) & bit ? packed_tile : small;
}

// Every k_onesweep instance that is built, one row per instantiation, by the
// kernel's template arguments.  This is the only list: lsb_kernels.hip
// instantiates the kernel of every row (adding a row is what builds it), and
// launch_onesweep launches the row os_select picks.
constexpr int kOsTile = 4096;                             // == kTile (lsb_kernels.h)
constexpr int kOsWholeBlock = 512, kOsHalvesBlock = 256;  // threads: the whole stage, the split stage
struct OsInstance {
  int block, ipt;  // block x ipt records per tile
  bool next, c16;
  int halves;
  bool seg, gather;
  int rg;
  bool pin, pout;
  int tn;  // the next pass's records per tile (its own where no next digit is counted, and for rg = 1)
};
constexpr bool operator==(const OsInstance& a, const OsInstance& b) {
  return a.block == b.block && a.ipt == b.ipt && a.next == b.next && a.c16 == b.c16 && a.halves == b.halves &&
         a.seg == b.seg && a.gather == b.gather && a.rg == b.rg && a.pin == b.pin && a.pout == b.pout && a.tn == b.tn;
}
constexpr OsInstance kOsInstances[] = {
    // Whole records, dense input: plain or gathered, the next digit or the
    // 16-bit counts, the split stage, the hybrid's last pass.
    {512, 8, false, false, 1, false, false, 0, false, false, 4096},
    {512, 8, false, false, 1, false, true, 0, false, false, 4096},
    {512, 8, true, false, 1, false, false, 0, false, false, 4096},  // the placement probe runs this one's body
    {512, 8, true, false, 1, false, true, 0, false, false, 4096},
    {512, 8, false, true, 1, false, false, 0, false, false, 4096},
    {512, 8, false, true, 1, false, true, 0, false, false, 4096},
    {256, 16, false, false, 2, false, false, 0, false, false, 4096},
    {256, 16, true, false, 2, false, false, 0, false, false, 4096},
    {512, 8, false, false, 1, true, false, 0, false, false, 4096},
    // The first pass into the regional layout: whole records, packing, packing in large tiles.
    {512, 8, true, false, 1, false, false, 1, false, false, 4096},
    {512, 8, true, false, 1, false, false, 1, false, true, 4096},
    {512, 10, true, false, 1, false, false, 1, false, true, 5120},
    // The pass that reads the layout: whole records (last or not), packed
    // before a pass of each tile size, packed in large tiles.
    {512, 8, false, false, 1, false, false, 2, false, false, 4096},
    {512, 8, true, false, 1, false, false, 2, false, false, 4096},
    {512, 8, true, false, 1, false, false, 2, true, true, 4096},
    {512, 8, true, false, 1, false, false, 2, true, true, 4608},
    {512, 8, true, false, 1, false, false, 2, true, true, 5120},
    {512, 10, true, false, 1, false, false, 2, true, true, 5120},
    // A packed sort's middle passes: before a pass of their own tile size, or of 4096.
    {512, 8, true, false, 1, false, false, 0, true, true, 4096},
    {512, 9, true, false, 1, false, false, 0, true, true, 4608},
    {512, 9, true, false, 1, false, false, 0, true, true, 4096},
    {512, 10, true, false, 1, false, false, 0, true, true, 5120},
    {512, 10, true, false, 1, false, false, 0, true, true, 4096},
    // A packed sort's last pass (Packed -> Elem).
    {512, 8, false, false, 1, false, false, 0, true, false, 4096},
    {512, 10, false, false, 1, false, false, 0, true, false, 5120},
};
constexpr int kOsInstanceCount = (int)(sizeof(kOsInstances) / sizeof(kOsInstances[0]));
constexpr int os_instance_tile(const OsInstance& r) { return r.block * r.ipt; }
constexpr OsPassKind os_instance_kind(const OsInstance& r) {
  return r.rg == 1 ? kOsPassFirst : r.rg == 2 ? kOsPassLayout : !r.pin ? kOsPassOther : r.next ? kOsPassMiddle : kOsPassLast;
}
// Some instance takes t records per tile.
inline bool os_tile_built(int t) {
  for (const OsInstance& r : kOsInstances)
    if (os_instance_tile(r) == t) return true;
  return false;
}
// A pass of that kind with t records per tile before one of tn has an
// instance (tn: ignored by the last pass, which counts no next digit; any
// built size for the first, whose counts are per region whatever tile reads
// them).  Only at small = kOsTile: the table is built for no other.
inline bool os_pass_tiles_ok(OsPassKind kind, int t, int tn, int small) {
  if (small != kOsTile) return false;
  for (const OsInstance& r : kOsInstances)
    if (os_instance_kind(r) == kind && os_instance_tile(r) == t &&
        (kind == kOsPassLast || (kind == kOsPassFirst ? os_tile_built(tn) : r.tn == tn)))
      return true;
  return false;
}

// A launch_onesweep request in plain terms (OnesweepExtra's pointers as
// "set or not"; tile, next_tile: 0 = kOsTile), and the row of kOsInstances
// that serves it: -1 when the request is refused or no instance is built.
struct OsRequest {
  int64_t m = 0;
  int shift = 0, next_shift = -1;
  int region_mode = 0;
  bool pack_in = false, pack_out = false;
  bool count16 = false, seg = false, gather = false, probe = false, totals = false;
  int halves = 1;
  int tile = 0, next_tile = 0;
};
inline int os_select(const OsRequest& q) {
  const int rm = q.region_mode;
  const bool next = q.next_shift >= 0;
  const int T = q.tile ? q.tile : kOsTile, TN = q.next_tile ? q.next_tile : kOsTile;
  if (rm < 0 || rm > 2 || (q.halves != 1 && q.halves != 2)) return -1;
  // Tiles over kOsTile for packed records only; the first pass's next tile
  // does not enter its instance, so it is checked here.
  if ((T != kOsTile || TN != kOsTile) && !q.pack_in && !(rm == 1 && q.pack_out)) return -1;
  if (rm == 1 && !os_tile_built(TN)) return -1;
  // The seam to the next pass (the first pass writes regions, which no run crosses).
  if (next && rm != 1 && !os_tile_fits(T, TN, q.m)) return -1;
  // A regional or packed pass: whole stage, nothing else set.
  if ((rm != 0 || q.pack_in) && (q.count16 || q.halves != 1 || q.seg || q.gather || q.probe || q.totals)) return -1;
  // The placement probe: the plain pass counting the next digit, whole stage.
  if (q.probe && (!next || q.count16 || q.halves != 1 || q.seg || q.gather)) return -1;
  // The 16-bit counts need the low byte below this digit.
  if (q.count16 && q.shift < 8) return -1;
  // The split stage only for the plain and next-digit forms, never gathered
  // (its gathered instances spill: 160-236 B per lane at 168 VGPRs; a
  // gathered pass takes the whole stage, lsb_exchange.cpp local_pass_os), and
  // not with the 16-bit counts, which run the whole stage.
  if (q.halves == 2 && q.gather) return -1;
  const bool split = q.halves == 2 && !q.count16;
  const int block = split ? kOsHalvesBlock : kOsWholeBlock;
  if (T % block != 0) return -1;
  const OsInstance want = {block, T / block, next, q.count16, split ? 2 : 1, q.seg, q.gather,
                           rm,    q.pack_in, q.pack_out, next && rm != 1 ? TN : T};
  for (int i = 0; i < kOsInstanceCount; ++i)
    if (kOsInstances[i] == want) return i;
  return -1;
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
