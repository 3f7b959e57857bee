// Runs of equal keys (lsb_count_runs / lsb_store_runs, include/lsb.h;
// DESIGN.md §7.2): three plain kernels and a scan.
//   k_run_count  one read of A: heads per tile, the smallest head
//   k_run_scan   one workgroup: tile counts -> exclusive tile bases, the
//                rank's four summary words
//   k_run_write  one more read of A: every head writes its run's key, start
//                and first value at its rank among the heads
//   k_run_diff   counts from adjacent starts
// and the reductions over the runs' values (lsb_plan_reduce /
// lsb_store_reduce):
//   k_run_reduce one more read of A: a segmented reduction per tile; a run's
//                last record of the tile writes its value, the tile's leading
//                part goes to tile_lead
//   k_run_carry  one workgroup: the later tiles' leads and the later ranks'
//                tail into the runs that go on past their tile
//   k_run_lead, k_run_lead_sum  the values of a rank's leading run
// and the run id of every record (lsb_label_runs):
//   k_run_label  one more read of A and one write of B: every record with
//                the global index of its run
// and the scan within the runs (lsb_plan_scan / lsb_store_scan /
// lsb_scan_runs):
//   k_run_scan_tile   one more read of A: what every tile leaves open at its end
//   k_run_scan_chain  one workgroup: what the tiles before it bring into every
//                     tile, and the rank's trailing word
//   k_run_scan_write  one more read of A and one write: every record's result,
//                     into a column or into the records of B
// No workgroup waits for another: a tile's base is ready before k_run_write,
// k_run_reduce or k_run_label starts, every tile's lead before k_run_carry does,
// every tile_open before k_run_scan_chain, every tile_in before k_run_scan_write.  No
// floating-point atomics: the order of every addition is the code's.
// Positions, bases and counts are 64-bit throughout.
//
// The kernels that read A share one tile skeleton.  lsb_tile.h holds the
// workgroup's geometry, the scan of the (wave, item) cells that numbers a
// tile's heads (tile_cells) and the recount guard (tile_recount): a tile whose
// own count of its heads is not the count's tile_cnt sets *err and writes
// nothing.  Here are the loads and head ballots (wave_heads), and for the
// kernels that combine values the scan of a wave's items (wave_scan_items) and
// the waves' hand-over through LDS (tile_hand_over).
#include <type_traits>

#include "lsb_kernels.h"
#include "lsb_keyform.h"
#include "lsb_tile.h"

namespace lsb {

namespace {

constexpr int kRunGridCap = 8192;
constexpr int kRunScanBlock = 1024;

// The previous lane's x by DPP wave_shr:1 (every lane active); lane 0 gets edge.
__device__ __forceinline__ uint64_t prev_lane(uint64_t x, uint64_t edge) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)edge, (int)(uint32_t)x, 0x138, 0xf, 0xf, false);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(edge >> 32), (int)(uint32_t)(x >> 32), 0x138, 0xf, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t last_lane(uint64_t x) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
}

// One wave's kTileWaveRecs records from position wave0 on, lane-striped: item
// j of lane l is position wave0 + 64 j + l, so every load instruction reads
// 1 KiB of adjacent records in 16-byte accesses.  heads[j] = ballot of the
// item's heads (positions >= here have none; position 0 is one exactly when
// head0).  A record's predecessor key comes from the lane below it, lane 0's
// from lane 63 of the item before; only item 0 of lane 0 loads A[wave0 - 1].
// Every lane of the wave must call it.
template <bool VALS>
__device__ __forceinline__ void wave_heads(const Elem* __restrict__ A, int64_t here, int64_t wave0, bool head0,
                                           uint64_t (&key)[kTileItems], uint64_t (&val)[kTileItems],
                                           uint64_t (&heads)[kTileItems]) {
  const int lane = tile_lane();
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const int64_t i = wave0 + j * 64 + lane;
    ulonglong2 v = make_ulonglong2(0, 0);
    if (i < here) v = *reinterpret_cast<const ulonglong2*>(A + i);
    key[j] = v.x;
    val[j] = v.y;
    // The value is part of the access whether it is used or not: the record
    // stays one 16-byte load (an 8-byte load of the key alone streams slower).
    if constexpr (!VALS) asm volatile("" ::"v"(v.y));
  }
  uint64_t edge = 0;
  if (lane == 0 && wave0 > 0 && wave0 < here) edge = A[wave0 - 1].key;
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const int64_t i = wave0 + j * 64 + lane;
    const uint64_t prev = prev_lane(key[j], edge);
    const bool head = i < here && (i == 0 ? head0 : key[j] != prev);
    heads[j] = __ballot(head);
    edge = last_lane(key[j]);
  }
}

// tile_cnt[t] = heads of tile t (position 0 is never one); *lead = the
// smallest head of the rank, when it is below the value *lead held.
__global__ __launch_bounds__(kTileBlock) void k_run_count(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         uint32_t* __restrict__ tile_cnt,
                                                         unsigned long long* __restrict__ lead) {
  __shared__ uint32_t s_cnt[kTileWaves], s_first[kTileWaves];
  const int wave = (int)(threadIdx.x >> 6);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], heads[kTileItems];
    wave_heads<false>(A, here, tile * kTile + (int64_t)wave * kTileWaveRecs, false, key, val, heads);
    uint32_t cnt = 0, first = kTile;  // the same in every lane
#pragma unroll
    for (int j = kTileItems - 1; j >= 0; --j) {
      cnt += (uint32_t)__popcll(heads[j]);
      if (heads[j]) first = (uint32_t)(wave * kTileWaveRecs + j * 64 + __builtin_ctzll(heads[j]));
    }
    if (tile_lane() == 0) {
      s_cnt[wave] = cnt;
      s_first[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0, f = kTile;
#pragma unroll
      for (int w = 0; w < kTileWaves; ++w) {
        total += s_cnt[w];
        f = s_first[w] < f ? s_first[w] : f;
      }
      tile_cnt[tile] = total;
      if (f < (uint32_t)kTile) {
        // *lead only falls: a tile whose head is not below a value already
        // seen there cannot lower it, and skips the atomic.
        const unsigned long long pos = (unsigned long long)(tile * kTile + f);
        if (pos < *reinterpret_cast<volatile unsigned long long*>(lead)) atomicMin(lead, pos);
      }
    }
    __syncthreads();
  }
}

// One workgroup.  Thread t takes the adjacent tiles [t * chunk, (t + 1) *
// chunk): their sum, a scan of the kRunScanBlock sums in LDS, then their
// exclusive bases, so any number of tiles goes through one workgroup.
// sum[0..3] = first key, last key, the heads of the rank, min(*lead, here).
__global__ __launch_bounds__(kRunScanBlock) void k_run_scan(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                            const uint32_t* __restrict__ tile_cnt,
                                                            int64_t* __restrict__ tile_base,
                                                            uint64_t* __restrict__ sum) {
  __shared__ int64_t s[kRunScanBlock];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (tiles + kRunScanBlock - 1) / kRunScanBlock;
  const int64_t lo = t * chunk < tiles ? t * chunk : tiles;
  const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  int64_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += tile_cnt[i];
  s[t] = mine;
  __syncthreads();
  for (int off = 1; off < kRunScanBlock; off <<= 1) {
    const int64_t v = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int64_t base = s[t] - mine;
  for (int64_t i = lo; i < hi; ++i) {
    tile_base[i] = base;
    base += tile_cnt[i];
  }
  if (t == 0) {
    sum[0] = A[0].key;
    sum[1] = A[here - 1].key;
    sum[2] = (uint64_t)s[kRunScanBlock - 1];
    sum[3] = sum[3] < (uint64_t)here ? sum[3] : (uint64_t)here;
  }
}

// Head number h of the rank (position 0 among them when head0) at position
// i writes keys[h], starts[h], firsts[h].  Within a tile a head's number is
// the tile's base + the heads of the (wave, item) cells before its own (a
// 64-entry scan in LDS) + the heads below its lane in its cell's ballot:
// adjacent heads write adjacent elements.  The recount guards every store of
// the tile, so no index leaves [0, runs).
__global__ __launch_bounds__(kTileBlock) void k_run_write(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         int64_t gbase, uint32_t head0,
                                                         const uint32_t* __restrict__ tile_cnt,
                                                         const int64_t* __restrict__ tile_base, void* __restrict__ keys,
                                                         int key_type, int flags, int64_t* __restrict__ starts,
                                                         void* __restrict__ firsts, int val_bytes,
                                                         uint32_t* __restrict__ err) {
  __shared__ uint32_t s_cell[kTileCells];
  __shared__ uint32_t s_total;
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(key_type, flags);
  const bool k32 = key_bytes(key_type) == 4;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], heads[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    wave_heads<true>(A, here, wave0, head0 != 0, key, val, heads);
    tile_cells(s_cell, &s_total, [&](int j) { return (uint32_t)__popcll(heads[j]); });
    if (tile_recount(s_total, tile, head0, tile_cnt, err)) {
      const int64_t out0 = tile_base[tile] + (int64_t)(head0 - tile_first(tile, head0));
#pragma unroll
      for (int j = 0; j < kTileItems; ++j) {
        if ((heads[j] >> lane) & 1) {
          const int64_t h = out0 + s_cell[wave * kTileItems + j] + tile_mbcnt(heads[j]);
          if (keys) {
            const uint64_t k = decode(key[j], form);
            if (k32) static_cast<uint32_t*>(keys)[h] = (uint32_t)k;
            else static_cast<uint64_t*>(keys)[h] = k;
          }
          if (starts) starts[h] = gbase + wave0 + j * 64 + lane;
          if (val_bytes == 8) static_cast<uint64_t*>(firsts)[h] = val[j];
          if (val_bytes == 4) static_cast<uint32_t*>(firsts)[h] = (uint32_t)val[j];
        }
      }
    }
    __syncthreads();
  }
}

// Build knob for experiments: 1 stores k_run_label's records nontemporally.
#ifndef LSB_LABEL_NT
#define LSB_LABEL_NT 0
#endif
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// B[i] = {A[i].key (kLabelKeep) or A[i].val (kLabelByValue), id}, id = the global index
// of the run that holds position i: gid0 + the rank's heads at or below i
// (position 0 among them when head0) - 1, so the records in front of the
// rank's first head, which belong to an earlier rank's run, get gid0 - 1.
// k_run_write's tile shape and head numbering, with the heads *at or below*
// the lane where a head there counts those below it.  Every record is stored
// whole, at the position it was loaded from: each store instruction writes
// 1 KiB of adjacent records, like the loads.  Plain stores.
// A and B are different buffers: a wave reads A[wave0 - 1], another wave's
// record.  The recount guards every store of the tile.
template <int MODE>
__global__ __launch_bounds__(kTileBlock) void k_run_label(const Elem* __restrict__ A, Elem* __restrict__ B,
                                                         int64_t here, int64_t tiles, int64_t gid0, uint32_t head0,
                                                         const uint32_t* __restrict__ tile_cnt,
                                                         const int64_t* __restrict__ tile_base,
                                                         uint32_t* __restrict__ err) {
  __shared__ uint32_t s_cell[kTileCells];
  __shared__ uint32_t s_total;
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], heads[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    // kLabelKeep drops the old value, and still loads whole records (as k_run_count)
    wave_heads<MODE != kLabelKeep>(A, here, wave0, head0 != 0, key, val, heads);
    tile_cells(s_cell, &s_total, [&](int j) { return (uint32_t)__popcll(heads[j]); });
    if (tile_recount(s_total, tile, head0, tile_cnt, err)) {
      // the id of a record with no head of the tile at or below it
      const int64_t id0 = gid0 + tile_base[tile] + (int64_t)(head0 - tile_first(tile, head0)) - 1;
#pragma unroll
      for (int j = 0; j < kTileItems; ++j) {
        const int64_t i = wave0 + j * 64 + lane;
        const uint32_t upto = s_cell[wave * kTileItems + j] + tile_mbcnt(heads[j]) + (uint32_t)((heads[j] >> lane) & 1);
        if (i < here) {
          const u64x2 rec = {MODE == kLabelKeep ? key[j] : val[j], (uint64_t)(id0 + upto)};
          if constexpr (LSB_LABEL_NT) __builtin_nontemporal_store(rec, reinterpret_cast<u64x2*>(B + i));
          else *reinterpret_cast<u64x2*>(B + i) = rec;
        }
      }
    }
    __syncthreads();
  }
}

// counts[j] = starts[j + 1] - starts[j]; the last run ends at `end`.
__global__ __launch_bounds__(256) void k_run_diff(const int64_t* __restrict__ starts, int64_t* __restrict__ counts,
                                                  int64_t runs, int64_t end) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < runs; j += stride)
    counts[j] = (j + 1 < runs ? starts[j + 1] : end) - starts[j];
}

// ---- reductions over the values of a run --------------------
static_assert(kRunLeadParts == kRunGridCap, "one partial per workgroup of k_run_lead");

// x of another lane by DPP (every lane active): row_shr:k (0x110 + k) takes
// the lane k below within a row of 16, row_bcast:15 (0x142) lane 15 of the row
// before, row_bcast:31 (0x143) lane 31.  A lane without a source keeps its own
// x; the scan does not use it there.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)x, (int)(uint32_t)x, CTRL, 0xf, 0xf, false);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(x >> 32), (int)(uint32_t)(x >> 32), CTRL, 0xf, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}

// The segmented inclusive reduction of v over the wave's lanes: lane l gets F
// over the lanes [l - reach, l].  Rows of 16 first (a lane takes the lane k
// below it while that lane is in its row and its segment), then lane 15 of
// row 0 into row 1 and of row 2 into row 3, then lane 31 into the upper half,
// each into the lanes whose segment reaches back that far.
template <int F>
__device__ __forceinline__ uint64_t wave_seg_scan(uint64_t v, int lane, int reach) {
  const int in_row = lane & 15, in_half = lane & 31;
  const int lim = reach < in_row ? reach : in_row;
  uint64_t y = dpp64<0x111>(v);
  if (1 <= lim) v = red<F>(y, v);
  y = dpp64<0x112>(v);
  if (2 <= lim) v = red<F>(y, v);
  y = dpp64<0x114>(v);
  if (4 <= lim) v = red<F>(y, v);
  y = dpp64<0x118>(v);
  if (8 <= lim) v = red<F>(y, v);
  y = dpp64<0x142>(v);
  if ((lane & 16) && in_row < reach) v = red<F>(y, v);
  y = dpp64<0x143>(v);
  if ((lane & 32) && in_half < reach) v = red<F>(y, v);
  return v;
}

__device__ __forceinline__ uint64_t shfl_down64(uint64_t x, int off) {
  return ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(x >> 32), off, 64) << 32) |
         (uint32_t)__shfl_down((int)(uint32_t)x, off, 64);
}

// A wave's items after wave_heads, x[j] in the combine's working form:
// x[j] becomes the segmented inclusive scan in position order from the wave's
// first record on, within an item across the lanes (wave_seg_scan), between
// the items by the value of lane 63.  Returns what the wave leaves open at its
// end (its records since its last head, all of them without one; the same in
// every lane), *cnt = its heads.
template <int F>
__device__ __forceinline__ uint64_t wave_scan_items(const uint64_t (&heads)[kTileItems], uint64_t (&x)[kTileItems],
                                                    int lane, uint32_t* cnt) {
  const uint64_t le = ~0ull >> (63 - lane);  // the lanes at or below this one
  uint64_t carry = red_identity(F);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const uint64_t m = heads[j] & le;
    // the lanes below this one that belong to its segment
    const int reach = m ? lane - (63 - __builtin_clzll(m)) : lane;
    uint64_t v = wave_seg_scan<F>(x[j], lane, reach);
    if (m == 0) v = red<F>(carry, v);  // in front of the item's first head: the segment open at the item's start
    carry = last_lane(v);
    c += (uint32_t)__popcll(heads[j]);
    x[j] = v;
  }
  *cnt = c;
  return carry;
}

// The waves' hand-over through LDS (s_part, s_cnt: kTileWaves entries each):
// every wave leaves its open part and its head count, and folds those of the
// waves before it in wave order, a wave with a head starting anew.  Returns
// what they leave open at this wave's first record; *before = their heads;
// *open = the same fold over all the waves, the tile's records since its last
// head; *total = the tile's heads.  One barrier inside; the caller puts another
// before the next tile's call.
template <int F>
__device__ __forceinline__ uint64_t tile_hand_over(uint64_t part, uint32_t cnt, int lane, int wave, uint64_t* s_part,
                                                   uint32_t* s_cnt, uint32_t* before, uint64_t* open,
                                                   uint32_t* total) {
  if (lane == 0) {
    s_part[wave] = part;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  uint64_t acc = red_identity(F), cw = acc;
  uint32_t t = 0, b = 0;
#pragma unroll
  for (int w = 0; w < kTileWaves; ++w) {
    if (w == wave) {
      cw = acc;
      b = t;
    }
    acc = s_cnt[w] ? s_part[w] : red<F>(acc, s_part[w]);
    t += s_cnt[w];
  }
  *before = b;
  *open = acc;
  *total = t;
  return cw;
}

// out[h] = F over the values of the records from head h up to the next head
// or the tile's end, h numbered as in k_run_write; tile_lead[t] = F over the
// tile's records in front of its first head (the whole tile without one, the
// identity when its first record is a head).  k_run_carry adds the later
// tiles' leads to a run that goes on past its tile.
// A segmented inclusive reduction in position order, keyed by the head
// ballots: within an item across the lanes (wave_seg_scan, six DPP steps),
// between a wave's items by the value of lane 63, between the four waves
// through LDS (wave_scan_items, tile_hand_over).  The hand-over's head counts
// number the heads as well: those of the waves before, then of the wave's
// items before, then of the lanes below.
// The last record of a segment (the next position is a head, or the tile or
// the rank ends there) holds the segment's value and writes it: every out[h]
// and every tile_lead[t] is written once, by one lane.  The recount guards
// all of it.
template <int F>
__global__ __launch_bounds__(kTileBlock) void k_run_reduce(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                          uint32_t head0, const uint32_t* __restrict__ tile_cnt,
                                                          const int64_t* __restrict__ tile_base, int val_type,
                                                          uint64_t* __restrict__ out,
                                                          uint64_t* __restrict__ tile_lead,
                                                          uint32_t* __restrict__ err) {
  __shared__ uint64_t s_part[kTileWaves];
  __shared__ uint32_t s_cnt[kTileWaves], s_first[kTileWaves];  // s_first: a wave's first record is a head
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(val_type, 0);
  const uint64_t le = ~0ull >> (63 - lane);  // the lanes at or below this one
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], x[kTileItems], heads[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    wave_heads<true>(A, here, wave0, head0 != 0, key, x, heads);
#pragma unroll
    for (int j = 0; j < kTileItems; ++j) x[j] = red_load(F, x[j], form);
    uint32_t cnt, before, total;
    uint64_t open;
    const uint64_t part = wave_scan_items<F>(heads, x, lane, &cnt);
    if (lane == 0) s_first[wave] = (uint32_t)(heads[0] & 1);
    // What the waves before this one leave open at its first record.
    const uint64_t cw = tile_hand_over<F>(part, cnt, lane, wave, s_part, s_cnt, &before, &open, &total);
    if (tile_recount(total, tile, head0, tile_cnt, err)) {
      const int64_t out0 = tile_base[tile] + (int64_t)(head0 - tile_first(tile, head0));
      const uint64_t after = wave + 1 < kTileWaves ? s_first[wave + 1] : 1;  // the tile ends after wave 3
      uint32_t cell = before;  // the tile's heads in front of item j: the waves before, then this wave's items
#pragma unroll
      for (int j = 0; j < kTileItems; ++j) {
        const int64_t i = wave0 + j * 64 + lane;
        const uint64_t nb = j + 1 < kTileItems ? heads[(j + 1) % kTileItems] & 1 : after;
        const uint64_t next = (heads[j] >> 1) | (nb << 63);  // the heads of the positions one up
        const uint64_t m = heads[j] & le;
        if (i < here && (((next >> lane) & 1) || i + 1 == here)) {
          uint64_t v = x[j];
          if (cell == before && m == 0) v = red<F>(cw, v);  // no head of this wave at or below the record
          v = red_store(F, v, form);
          const uint32_t upto = cell + (uint32_t)__popcll(m);  // heads of the tile up to here
          if (upto) out[out0 + upto - 1] = v;
          else tile_lead[tile] = v;
        }
        cell += (uint32_t)__popcll(heads[j]);
      }
      if (threadIdx.x == 0 && (heads[0] & 1)) tile_lead[tile] = red_store(F, red_identity(F), form);
    }
    __syncthreads();
  }
}

// One workgroup, chunked over adjacent tiles as k_run_scan.  A tile with a
// head leaves its last run open; the leads of the tiles after it, up to and
// including the next tile with a head (or the rank's last tile), belong to
// that run and are folded into out at the tile's last head, in tile order;
// the rank's last such run also takes `tail`.  Leads in front of the rank's
// first head belong to an earlier rank's run and are dropped.  A thread folds
// the runs that end inside its chunk itself; for its chunk's last one it walks
// the later chunks' leading parts in LDS, so out[h] has one writer.
__global__ __launch_bounds__(kRunScanBlock) void k_run_carry(int64_t tiles, uint32_t head0,
                                                             const uint32_t* __restrict__ tile_cnt,
                                                             const int64_t* __restrict__ tile_base,
                                                             const uint64_t* __restrict__ tile_lead, int F,
                                                             int val_type, uint64_t tail,
                                                             uint64_t* __restrict__ out) {
  __shared__ uint64_t s_pre[kRunScanBlock];  // a chunk's leads up to and including its first tile with a head
  __shared__ uint32_t s_has[kRunScanBlock];  // the chunk has such a tile
  const KeyForm form = key_form(val_type, 0);
  const int t = (int)threadIdx.x;
  const int64_t chunk = (tiles + kRunScanBlock - 1) / kRunScanBlock;
  const int64_t lo = t * chunk < tiles ? t * chunk : tiles;
  const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  uint64_t acc = red_identity(F), pre = red_identity(F);
  int64_t target = -1;  // the last head of the last tile with one, so far
  for (int64_t i = lo; i < hi; ++i) {
    acc = red(F, acc, red_load(F, tile_lead[i], form));
    const uint32_t cnt = tile_cnt[i] + (i == 0 ? head0 : 0u);
    if (cnt) {
      if (target >= 0) out[target] = red_store(F, red(F, red_load(F, out[target], form), acc), form);
      else pre = acc;
      target = tile_base[i] + (i == 0 ? 0 : (int64_t)head0) + cnt - 1;
      acc = red_identity(F);
    }
  }
  s_pre[t] = target >= 0 ? pre : acc;
  s_has[t] = target >= 0;
  __syncthreads();
  if (target >= 0) {
    bool open = true;  // no later tile has a head: the run goes on to the rank's end
    for (int k = t + 1; k < kRunScanBlock && open; ++k) {
      acc = red(F, acc, s_pre[k]);
      open = !s_has[k];
    }
    if (open) acc = red(F, acc, red_load(F, tail, form));
    out[target] = red_store(F, red(F, red_load(F, out[target], form), acc), form);
  }
}

// The workgroup's F over every thread's acc, in an order the code fixes (a
// tree over each wave's lanes, then the waves in order); thread 0 has it.
__device__ __forceinline__ uint64_t block_red(int F, uint64_t acc, uint64_t* s_wave) {
  const int lane = tile_lane();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t y = shfl_down64(acc, off);
    if (lane + off < 64) acc = red(F, acc, y);
  }
  if (lane == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  for (int w = 1; w < kTileWaves; ++w) acc = red(F, acc, s_wave[w]);
  return acc;
}

// parts[b] = F over the values of workgroup b's tiles of A[0, lead), tile by
// tile in a grid stride.
__global__ __launch_bounds__(kTileBlock) void k_run_lead(const Elem* __restrict__ A, int64_t lead, int F, int val_type,
                                                        uint64_t* __restrict__ parts) {
  __shared__ uint64_t s_wave[kTileWaves];
  const KeyForm form = key_form(val_type, 0);
  uint64_t acc = red_identity(F);
  for (int64_t base = (int64_t)blockIdx.x * kTile; base < lead; base += (int64_t)gridDim.x * kTile)
    for (int j = 0; j < kTileItems; ++j) {
      const int64_t i = base + j * kTileBlock + threadIdx.x;
      if (i < lead) acc = red(F, acc, red_load(F, A[i].val, form));
    }
  acc = block_red(F, acc, s_wave);
  if (threadIdx.x == 0) parts[blockIdx.x] = red_store(F, acc, form);
}

// One workgroup: *out = F over parts[0, cnt), thread t taking cnt / kTileBlock
// (rounded up) adjacent ones in index order.
__global__ __launch_bounds__(kTileBlock) void k_run_lead_sum(const uint64_t* __restrict__ parts, int cnt, int F,
                                                            int val_type, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_wave[kTileWaves];
  const KeyForm form = key_form(val_type, 0);
  const int chunk = (cnt + kTileBlock - 1) / kTileBlock;
  uint64_t acc = red_identity(F);
  for (int i = (int)threadIdx.x * chunk; i < ((int)threadIdx.x + 1) * chunk && i < cnt; ++i)
    acc = red(F, acc, red_load(F, parts[i], form));
  acc = block_red(F, acc, s_wave);
  if (threadIdx.x == 0) *out = red_store(F, acc, form);
}

// ---- the scan within the runs -------------------------------
// The scan's op as the kernels are instantiated: the four combines, and the
// two that count (every operand 1 under the integer add).
enum ScanKind { kSkAdd = kRedAdd, kSkFadd = kRedFadd, kSkMin = kRedMin, kSkMax = kRedMax, kSkCount = 4, kSkStart = 5 };
constexpr int sk_form(int K) { return K >= kSkCount ? (int)kRedAdd : K; }

// The records' operands in the working form: the value (encoded for min and
// max), 1 for the counting kinds, the identity past the rank's end, so that
// the last tile's open part holds the rank's records only.
template <int K>
__device__ __forceinline__ void scan_operands(uint64_t (&x)[kTileItems], int64_t wave0, int64_t here, int lane,
                                              const KeyForm& form) {
  constexpr int F = sk_form(K);
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const int64_t i = wave0 + j * 64 + lane;
    x[j] = i < here ? (K >= kSkCount ? 1ull : red_load(F, x[j], form)) : red_identity(F);
  }
}

// tile_open[t] = the combine over tile t's records from its last head on, in
// the working form (the whole tile without a head; position 0 is a head
// exactly when head0).  A tile whose heads are not tile_cnt[t] sets *err
// (tile_recount) and writes its tile_open all the same: the plan is dropped.
template <int K>
__global__ __launch_bounds__(kTileBlock) void k_run_scan_tile(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                             uint32_t head0, const uint32_t* __restrict__ tile_cnt,
                                                             int val_type, uint64_t* __restrict__ tile_open,
                                                             uint32_t* __restrict__ err) {
  constexpr int F = sk_form(K);
  __shared__ uint64_t s_part[kTileWaves];
  __shared__ uint32_t s_cnt[kTileWaves];
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(val_type, 0);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], x[kTileItems], heads[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    wave_heads<(K < kSkCount)>(A, here, wave0, head0 != 0, key, x, heads);
    scan_operands<K>(x, wave0, here, lane, form);
    uint32_t cnt, before, total;
    uint64_t open;
    const uint64_t part = wave_scan_items<F>(heads, x, lane, &cnt);
    tile_hand_over<F>(part, cnt, lane, wave, s_part, s_cnt, &before, &open, &total);
    if (threadIdx.x == 0) {  // nothing to keep the other threads from: only the guard's word matters here
      tile_recount(total, tile, head0, tile_cnt, err);
      tile_open[tile] = open;
    }
    __syncthreads();
  }
}

// One workgroup, chunked over adjacent tiles as k_run_scan: a segmented
// exclusive scan of tile_open in tile order, a tile with a head starting anew.
// With S(t) = tile_open[t] when tile t has a head, else S(t - 1) + tile_open[t]
// (S(-1) the identity): tile_in[t] = S(t - 1), *trail = S(tiles - 1) in the
// caller's bits.  A thread folds its chunk, the chunks' (value, has a head)
// pairs are scanned in LDS, and the thread walks its chunk again from what the
// chunks before it leave open.
__global__ __launch_bounds__(kRunScanBlock) void k_run_scan_chain(int64_t tiles, uint32_t head0,
                                                                  const uint32_t* __restrict__ tile_cnt,
                                                                  const uint64_t* __restrict__ tile_open, int F,
                                                                  int val_type, uint64_t* __restrict__ tile_in,
                                                                  uint64_t* __restrict__ trail) {
  __shared__ uint64_t s_v[kRunScanBlock];
  __shared__ uint32_t s_h[kRunScanBlock];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (tiles + kRunScanBlock - 1) / kRunScanBlock;
  const int64_t lo = t * chunk < tiles ? t * chunk : tiles;
  const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  uint64_t acc = red_identity(F);
  uint32_t has = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const uint32_t h = tile_cnt[i] + (i == 0 ? head0 : 0u);
    acc = h ? tile_open[i] : red(F, acc, tile_open[i]);
    has |= h;
  }
  s_v[t] = acc;
  s_h[t] = has;
  __syncthreads();
  for (int off = 1; off < kRunScanBlock; off <<= 1) {
    uint64_t v = s_v[t];
    uint32_t h = s_h[t];
    if (t >= off && !h) {
      v = red(F, s_v[t - off], v);
      h = s_h[t - off];
    }
    __syncthreads();
    s_v[t] = v;
    s_h[t] = h;
    __syncthreads();
  }
  uint64_t open = t ? s_v[t - 1] : red_identity(F);
  for (int64_t i = lo; i < hi; ++i) {
    tile_in[i] = open;
    const uint32_t h = tile_cnt[i] + (i == 0 ? head0 : 0u);
    open = h ? tile_open[i] : red(F, open, tile_open[i]);
  }
  // the chunks after the last tile are empty: the last thread holds S(tiles - 1)
  if (t == kRunScanBlock - 1) *trail = red_store(F, open, key_form(val_type, 0));
}

// The result of every record, one read of A and one write: out[i] (SINK
// kScanColumn, 8-byte elements) or the record {key (kScanKeep) or old value
// (kScanByValue), result} at out[i] (another buffer than A: a wave reads
// A[wave0 - 1]).  A result is a fold of up to three parts, in one association:
//   ((carry + tile_in[t]) + s)  for a record in front of the rank's first head (i < lead)
//   (tile_in[t] + s)            for a later record in front of its tile's first head
//   s                           otherwise
// with s the scan inside the tile, itself (what the waves before leave open,
// folded in wave order) + (the value of lane 63 of the item before + the
// scan across the item's lanes), each part only where no head lies between.
// The counting kinds scan ones: with c the inclusive count, kSkCount gives
// c - 1 and kSkStart the record's global position - (c - 1).
// Every store is at the position its record was loaded from: a store
// instruction writes adjacent elements across the lanes, like the loads.  The
// recount guards every store of the tile.
template <int K, int SINK>
__global__ __launch_bounds__(kTileBlock) void k_run_scan_write(const Elem* __restrict__ A, void* __restrict__ out,
                                                              int64_t here, int64_t tiles, int64_t gbase,
                                                              uint32_t head0, int64_t lead,
                                                              const uint32_t* __restrict__ tile_cnt,
                                                              const uint64_t* __restrict__ tile_in, int val_type,
                                                              uint64_t carry_bits, uint32_t* __restrict__ err) {
  constexpr int F = sk_form(K);
  __shared__ uint64_t s_part[kTileWaves];
  __shared__ uint32_t s_cnt[kTileWaves];
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(val_type, 0);
  const uint64_t carry = red_load(F, carry_bits, form);
  const uint64_t le = ~0ull >> (63 - lane);  // the lanes at or below this one
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], x[kTileItems], heads[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    wave_heads<(K < kSkCount || SINK == kScanByValue)>(A, here, wave0, head0 != 0, key, val, heads);
#pragma unroll
    for (int j = 0; j < kTileItems; ++j) x[j] = val[j];
    scan_operands<K>(x, wave0, here, lane, form);
    uint32_t cnt, before, total;
    uint64_t open;
    const uint64_t part = wave_scan_items<F>(heads, x, lane, &cnt);
    const uint64_t cw = tile_hand_over<F>(part, cnt, lane, wave, s_part, s_cnt, &before, &open, &total);
    if (tile_recount(total, tile, head0, tile_cnt, err)) {
      const uint64_t tin = tile_in[tile];
      const uint64_t tc = red<F>(carry, tin);
      bool pre = true;  // no head of this wave in the items before j
#pragma unroll
      for (int j = 0; j < kTileItems; ++j) {
        const int64_t i = wave0 + j * 64 + lane;
        uint64_t v = x[j];
        if (pre && (heads[j] & le) == 0) {  // no head of this wave at or below the record
          v = red<F>(cw, v);
          if (before == 0) v = red<F>(i < lead ? tc : tin, v);  // nor of the tile
        }
        uint64_t res;
        if constexpr (K == kSkCount) res = v - 1;
        else if constexpr (K == kSkStart) res = (uint64_t)(gbase + i) - (v - 1);
        else res = red_store(F, v, form);
        if (i < here) {
          if constexpr (SINK == kScanColumn) {
            static_cast<uint64_t*>(out)[i] = res;
          } else {
            const u64x2 rec = {SINK == kScanKeep ? key[j] : val[j], res};
            *reinterpret_cast<u64x2*>(static_cast<Elem*>(out) + i) = rec;
          }
        }
        pre = pre && heads[j] == 0;
      }
    }
    __syncthreads();
  }
}

int scan_kind(int op, int val_type) {
  return op == kScanCount ? (int)kSkCount : op == kScanStart ? (int)kSkStart : red_form(op, val_type);
}

// f(std::integral_constant<int, V>()) for the run-time value V of a template
// argument, so that a launch is written once: the reduce form, the scan kind,
// the scan's sink.
template <int V>
using Const = std::integral_constant<int, V>;

template <typename Fn>
void with_red_form(int F, Fn&& f) {
  switch (F) {
    case kRedAdd: return f(Const<kRedAdd>());
    case kRedFadd: return f(Const<kRedFadd>());
    case kRedMin: return f(Const<kRedMin>());
    default: return f(Const<kRedMax>());
  }
}

template <typename Fn>
void with_scan_kind(int K, Fn&& f) {
  switch (K) {
    case kSkCount: return f(Const<kSkCount>());
    case kSkStart: return f(Const<kSkStart>());
    default: return with_red_form(K, f);  // the four combines are the reduce forms
  }
}

template <typename Fn>
void with_scan_sink(int sink, Fn&& f) {
  switch (sink) {
    case kScanColumn: return f(Const<kScanColumn>());
    case kScanKeep: return f(Const<kScanKeep>());
    default: return f(Const<kScanByValue>());
  }
}

int run_grid(int64_t work, int block) {
  const int64_t g = (work + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > kRunGridCap ? kRunGridCap : g));
}

}  // namespace

hipError_t launch_run_count(const Elem* A, int64_t here, uint32_t* tile_cnt, int64_t* tile_base, uint64_t* sum,
                            hipStream_t s) {
  if (here <= 0 || !A || !tile_cnt || !tile_base || !sum) return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  hipError_t e = hipMemsetAsync(sum + 3, 0xff, sizeof(uint64_t), s);  // lead: no head seen
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_run_count, dim3(run_grid(tiles, 1)), dim3(kTileBlock), 0, s, A, here, tiles, tile_cnt,
                     reinterpret_cast<unsigned long long*>(sum + 3));
  hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(kRunScanBlock), 0, s, A, here, tiles, tile_cnt, tile_base, sum);
  return hipGetLastError();
}

hipError_t launch_run_write(const Elem* A, int64_t here, int64_t gbase, int head0, const uint32_t* tile_cnt,
                            const int64_t* tile_base, void* keys, int key_type, int flags, int64_t* starts,
                            int64_t* counts, void* firsts, int val_bytes, int64_t runs, int64_t end, uint32_t* err,
                            hipStream_t s) {
  if (!key_form_valid(key_type, flags) || (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) ||
      (val_bytes == 0) != (firsts == nullptr) || (!keys && !starts && !firsts) || (counts && !starts) ||
      (head0 != 0 && head0 != 1) || !A || !tile_cnt || !tile_base || !err)
    return hipErrorInvalidValue;
  if (here <= 0 || runs <= 0) return hipSuccess;
  const int64_t tiles = run_tiles(here);
  hipLaunchKernelGGL(k_run_write, dim3(run_grid(tiles, 1)), dim3(kTileBlock), 0, s, A, here, tiles, gbase,
                     (uint32_t)head0, tile_cnt, tile_base, keys, key_type, flags, starts, firsts, val_bytes, err);
  if (counts)
    hipLaunchKernelGGL(k_run_diff, dim3(run_grid(runs, 256)), dim3(256), 0, s, starts, counts, runs, end);
  return hipGetLastError();
}

hipError_t launch_run_label(const Elem* A, Elem* B, int64_t here, int64_t gid0, int head0, const uint32_t* tile_cnt,
                            const int64_t* tile_base, int mode, uint32_t* err, hipStream_t s) {
  if ((mode != kLabelKeep && mode != kLabelByValue) || (head0 != 0 && head0 != 1) || gid0 < 1 - head0 || !A || !B ||
      A == B || !tile_cnt || !tile_base || !err)
    return hipErrorInvalidValue;
  if (here <= 0) return hipSuccess;
  const int64_t tiles = run_tiles(here);
  const dim3 grid(run_grid(tiles, 1)), block(kTileBlock);
  if (mode == kLabelKeep)
    hipLaunchKernelGGL(k_run_label<kLabelKeep>, grid, block, 0, s, A, B, here, tiles, gid0, (uint32_t)head0, tile_cnt,
                       tile_base, err);
  else
    hipLaunchKernelGGL(k_run_label<kLabelByValue>, grid, block, 0, s, A, B, here, tiles, gid0, (uint32_t)head0,
                       tile_cnt, tile_base, err);
  return hipGetLastError();
}

hipError_t launch_run_lead(const Elem* A, int64_t lead, int op, int val_type, uint64_t* parts, uint64_t* out,
                           hipStream_t s) {
  if (!reduce_valid(op, val_type) || lead <= 0 || !A || !parts || !out) return hipErrorInvalidValue;
  const int F = red_form(op, val_type);
  const int grid = run_grid(run_tiles(lead), 1);
  hipLaunchKernelGGL(k_run_lead, dim3(grid), dim3(kTileBlock), 0, s, A, lead, F, val_type, parts);
  hipLaunchKernelGGL(k_run_lead_sum, dim3(1), dim3(kTileBlock), 0, s, parts, grid, F, val_type, out);
  return hipGetLastError();
}

hipError_t launch_run_reduce(const Elem* A, int64_t here, int head0, const uint32_t* tile_cnt,
                             const int64_t* tile_base, int op, int val_type, uint64_t tail, uint64_t* tile_lead,
                             uint64_t* out, int64_t runs, uint32_t* err, hipStream_t s) {
  if (!reduce_valid(op, val_type) || (head0 != 0 && head0 != 1) || here <= 0 || runs <= 0 || !A || !tile_cnt ||
      !tile_base || !tile_lead || !out || !err)
    return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  const int F = red_form(op, val_type);
  const dim3 grid(run_grid(tiles, 1)), block(kTileBlock);
  with_red_form(F, [&](auto f) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_reduce<decltype(f)::value>), grid, block, 0, s, A, here, tiles,
                       (uint32_t)head0, tile_cnt, tile_base, val_type, out, tile_lead, err);
  });
  hipLaunchKernelGGL(k_run_carry, dim3(1), dim3(kRunScanBlock), 0, s, tiles, (uint32_t)head0, tile_cnt, tile_base,
                     tile_lead, F, val_type, tail, out);
  return hipGetLastError();
}

hipError_t launch_run_scan_plan(const Elem* A, int64_t here, int head0, const uint32_t* tile_cnt, int op,
                                int val_type, uint64_t* tile_open, uint64_t* tile_in, uint64_t* trail,
                                uint32_t* err, hipStream_t s) {
  if (!scan_valid(op, val_type) || (head0 != 0 && head0 != 1) || here <= 0 || !A || !tile_cnt || !tile_open ||
      !tile_in || !trail || !err)
    return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  const dim3 grid(run_grid(tiles, 1)), block(kTileBlock);
  with_scan_kind(scan_kind(op, val_type), [&](auto k) {
    constexpr int K = decltype(k)::value == kSkStart ? (int)kSkCount : decltype(k)::value;  // both counting kinds scan ones
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_scan_tile<K>), grid, block, 0, s, A, here, tiles, (uint32_t)head0,
                       tile_cnt, val_type, tile_open, err);
  });
  hipLaunchKernelGGL(k_run_scan_chain, dim3(1), dim3(kRunScanBlock), 0, s, tiles, (uint32_t)head0, tile_cnt,
                     tile_open, scan_form(op, val_type), val_type, tile_in, trail);
  return hipGetLastError();
}

hipError_t launch_run_scan_write(const Elem* A, int64_t here, int64_t gbase, int head0, int64_t lead,
                                 const uint32_t* tile_cnt, const uint64_t* tile_in, int op, int val_type,
                                 uint64_t carry, int sink, void* out, uint32_t* err, hipStream_t s) {
  if (!scan_valid(op, val_type) || (head0 != 0 && head0 != 1) || lead < 0 || lead > here || (head0 && lead != 0) ||
      (sink != kScanColumn && sink != kScanKeep && sink != kScanByValue) || !A || !out || out == A || !tile_cnt ||
      !tile_in || !err)
    return hipErrorInvalidValue;
  if (here <= 0) return hipSuccess;
  const int64_t tiles = run_tiles(here);
  const dim3 grid(run_grid(tiles, 1)), block(kTileBlock);
  with_scan_kind(scan_kind(op, val_type), [&](auto k) {
    with_scan_sink(sink, [&](auto snk) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_scan_write<decltype(k)::value, decltype(snk)::value>), grid, block, 0,
                         s, A, out, here, tiles, gbase, (uint32_t)head0, lead, tile_cnt, tile_in, val_type, carry, err);
    });
  });
  return hipGetLastError();
}

}  // namespace lsb
