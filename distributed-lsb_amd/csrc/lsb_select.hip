// The k-th key and the first k + 1 records of the stable sort, without the
// sort (lsb_select / lsb_store_select, include/lsb.h): an MSD
// radix select, one byte per round from the top.
//   k_sel_hist   one read of the round's source (A, or a candidate range in
//                B): the histogram of one key byte over the records whose
//                upper bits equal the prefix found so far; round one also
//                reduces the span of the keys; a later round may copy the
//                matching records, whole, into B (the compaction)
//   k_sel_count  one read of A: keys below and equal to the pivot per tile
//   k_sel_scan   one workgroup: tile counts -> exclusive tile bases
//   k_sel_write  one more read of A: every selected record writes its key and
//                value at its rank among the selected, in slot order
// No workgroup waits for another: a round's counts go to the host between two
// launches, a tile's base is ready before k_sel_write starts.  Positions,
// bases and counts are 64-bit throughout.
// The workgroup's geometry and the scan of a tile's (wave, item) cells are
// lsb_tile.h's, shared with lsb_runs.hip.
#include "lsb_kernels.h"
#include "lsb_keyform.h"
#include "lsb_tile.h"

namespace lsb {

namespace {

constexpr int kSelGridCap = 2048;   // 8 workgroups per CU; the tiles beyond are strided over
constexpr int kSelScanBlock = 1024;
constexpr int kSelStage = 512;      // records a wave stages in LDS per reservation in dst
static_assert(kTile < (1 << 16), "a tile's two counts share one 32-bit word");

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t first_lane(uint64_t x) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// k_subhist's shape: wave-private histogram rows in LDS, one atomic for an
// item whose 64 lanes agree, nontemporal 8-byte key loads with the records'
// stride, a capped grid that strides over the tiles.  A record counts when
// (key & mask) == prefix.
// COMPACT: every counted record is also appended to dst.  A wave stages its
// matches in its own kSelStage records of LDS and, when they would not take
// another item's, reserves that many slots of dst with one returning add on
// words[kSelHist] and stores them there in 16-byte accesses: one reservation
// per kSelStage - 63 records or more, never one per tile, and no workgroup
// barrier in the loop.  A matching record's value is loaded on its own, from
// the line its key came from.  The host knows `bound`, the number of matching
// records, from the round before: a slot at or past it is not stored and sets
// words[kSelHist + 1].
template <bool SPAN, bool COMPACT>
__global__ __launch_bounds__(kTileBlock) void k_sel_hist(const Elem* __restrict__ src, int64_t m, int64_t tiles,
                                                        int shift, uint64_t prefix, uint64_t mask,
                                                        Elem* __restrict__ dst, int64_t bound,
                                                        unsigned long long* __restrict__ words) {
  __shared__ uint32_t hist[kTileWaves][kSelHist];
  __shared__ uint64_t span_or[kTileWaves], span_nor[kTileWaves];
  __shared__ u64x2 stage[COMPACT ? kTileWaves * kSelStage : 1];
  const int lane = tile_lane(), w = (int)(threadIdx.x >> 6);
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(src);
  u64x2* const mine = stage + (COMPACT ? w * kSelStage : 0);
  uint64_t kor = 0, knor = 0;
  uint32_t fill = 0;  // staged records of this wave: the same in every lane
  for (int i = threadIdx.x; i < kTileWaves * kSelHist; i += kTileBlock) (&hist[0][0])[i] = 0;
  __syncthreads();

  // The wave's staged records into dst, at the slots it reserves for them.
  auto flush = [&]() {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&words[kSelHist], (unsigned long long)fill);
    base = first_lane(base);
    bool past = false;
    for (uint32_t i = lane; i < fill; i += 64) {
      const int64_t at = (int64_t)base + i;
      if (at < bound) *reinterpret_cast<u64x2*>(dst + at) = mine[i];
      else past = true;
    }
    if (past) atomicOr(&words[kSelHist + 1], 1ull);
    __builtin_amdgcn_wave_barrier();  // the stage is read before it is written again
    fill = 0;
  };

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t tb = tile * kTile;
    uint64_t k[kTileItems];
#pragma unroll
    for (int i = 0; i < kTileItems; ++i) {
      const int64_t idx = tb + (int64_t)i * kTileBlock + threadIdx.x;
      k[i] = idx < m ? __builtin_nontemporal_load(keys + 2 * idx) : 0ull;  // streaming
    }
#pragma unroll
    for (int i = 0; i < kTileItems; ++i) {
      const int64_t idx = tb + (int64_t)i * kTileBlock + threadIdx.x;
      const bool valid = idx < m;
      if (SPAN && valid) {
        kor |= k[i];
        knor |= ~k[i];
      }
      const bool match = valid && (k[i] & mask) == prefix;
      const uint32_t d = (uint32_t)(k[i] >> shift) & (kSelHist - 1);
      const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
      if (__all(match && d == d0)) {
        if (lane == 0) atomicAdd(&hist[w][d0], 64u);
      } else if (match) {
        atomicAdd(&hist[w][d], 1u);
      }
      if constexpr (COMPACT) {
        const uint64_t hits = __ballot(match);
        if (hits) {  // the same in every lane
          const uint32_t cnt = (uint32_t)__popcll(hits);
          if (fill + cnt > (uint32_t)kSelStage) flush();
          if (match) mine[fill + tile_mbcnt(hits)] = u64x2{k[i], src[idx].val};
          fill += cnt;
        }
      }
    }
  }
  if constexpr (COMPACT) {
    __builtin_amdgcn_wave_barrier();
    if (fill) flush();
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSelHist; b += kTileBlock) {
    uint64_t s = 0;
#pragma unroll
    for (int ww = 0; ww < kTileWaves; ++ww) s += hist[ww][b];
    if (s) atomicAdd(&words[b], (unsigned long long)s);
  }
  if constexpr (SPAN) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      kor |= __shfl_xor(kor, off, 64);
      knor |= __shfl_xor(knor, off, 64);
    }
    if (lane == 0) {
      span_or[w] = kor;
      span_nor[w] = knor;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t o = 0, no = 0;
#pragma unroll
      for (int ww = 0; ww < kTileWaves; ++ww) {
        o |= span_or[ww];
        no |= span_nor[ww];
      }
      atomicOr(&words[kSelHist], (unsigned long long)o);
      atomicOr(&words[kSelHist + 1], (unsigned long long)no);
    }
  }
}

// One wave's kTileWaveRecs records from position wave0 on, lane-striped as in
// lsb_runs.hip's wave_heads: item j of lane l is position wave0 + 64 j + l,
// every load instruction reads 1 KiB of adjacent records in 16-byte accesses.
// lt[j], eq[j] = ballots of the item's keys below and equal to the pivot
// (positions >= here have neither).  Every lane of the wave must call it.
template <bool VALS>
__device__ __forceinline__ void wave_compare(const Elem* __restrict__ A, int64_t here, int64_t wave0, uint64_t pivot,
                                             uint64_t (&key)[kTileItems], uint64_t (&val)[kTileItems],
                                             uint64_t (&lt)[kTileItems], uint64_t (&eq)[kTileItems]) {
  const int lane = tile_lane();
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const int64_t i = wave0 + j * 64 + lane;
    ulonglong2 v = make_ulonglong2(0, 0);
    if (i < here) v = *reinterpret_cast<const ulonglong2*>(A + i);
    key[j] = v.x;
    val[j] = v.y;
    // The record stays one 16-byte load whether the value is used or not.
    if constexpr (!VALS) asm volatile("" ::"v"(v.y));
  }
#pragma unroll
  for (int j = 0; j < kTileItems; ++j) {
    const bool in = wave0 + j * 64 + lane < here;
    lt[j] = __ballot(in && key[j] < pivot);
    eq[j] = __ballot(in && key[j] == pivot);
  }
}

__global__ __launch_bounds__(kTileBlock) void k_sel_count(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         uint64_t pivot, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_cnt[kTileWaves];
  const int wave = (int)(threadIdx.x >> 6);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], lt[kTileItems], eq[kTileItems];
    wave_compare<false>(A, here, tile * kTile + (int64_t)wave * kTileWaveRecs, pivot, key, val, lt, eq);
    uint32_t cnt = 0;  // the same in every lane
#pragma unroll
    for (int j = 0; j < kTileItems; ++j) cnt += (uint32_t)__popcll(lt[j]) | ((uint32_t)__popcll(eq[j]) << 16);
    if (tile_lane() == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < kTileWaves; ++w) total += s_cnt[w];
      tile_cnt[tile] = total;
    }
    __syncthreads();
  }
}

// One workgroup, chunked over adjacent tiles as k_run_scan: tile_base[2 t] =
// the keys below the pivot in the tiles before t, tile_base[2 t + 1] = those
// equal to it.  The rank's totals must be the plan's.
__global__ __launch_bounds__(kSelScanBlock) void k_sel_scan(int64_t tiles, const uint32_t* __restrict__ tile_cnt,
                                                            int64_t* __restrict__ tile_base, int64_t below,
                                                            int64_t equal, uint32_t* __restrict__ err) {
  __shared__ int64_t s_lt[kSelScanBlock], s_eq[kSelScanBlock];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (tiles + kSelScanBlock - 1) / kSelScanBlock;
  const int64_t lo = t * chunk < tiles ? t * chunk : tiles;
  const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  int64_t my_lt = 0, my_eq = 0;
  for (int64_t i = lo; i < hi; ++i) {
    my_lt += tile_cnt[i] & 0xffffu;
    my_eq += tile_cnt[i] >> 16;
  }
  s_lt[t] = my_lt;
  s_eq[t] = my_eq;
  __syncthreads();
  for (int off = 1; off < kSelScanBlock; off <<= 1) {
    const int64_t a = t >= off ? s_lt[t - off] : 0, b = t >= off ? s_eq[t - off] : 0;
    __syncthreads();
    s_lt[t] += a;
    s_eq[t] += b;
    __syncthreads();
  }
  int64_t base_lt = s_lt[t] - my_lt, base_eq = s_eq[t] - my_eq;
  for (int64_t i = lo; i < hi; ++i) {
    tile_base[2 * i] = base_lt;
    tile_base[2 * i + 1] = base_eq;
    base_lt += tile_cnt[i] & 0xffffu;
    base_eq += tile_cnt[i] >> 16;
  }
  if (t == 0 && (s_lt[kSelScanBlock - 1] != below || s_eq[kSelScanBlock - 1] != equal)) atomicOr(err, 1u);
}

// cnt staged elements, element g0 + i of col from lds[i]: in 16-byte accesses
// between the 16-byte boundaries of col when VEC (col itself is aligned to 16
// bytes then), the elements in front of the first and behind the last boundary
// one by one; element by element throughout otherwise.
template <typename T, bool VEC>
__device__ __forceinline__ void store_range(T* __restrict__ col, int64_t g0, int cnt, const uint64_t* lds) {
  constexpr int G = 16 / (int)sizeof(T);
  int head = cnt, groups = 0;
  if constexpr (VEC) {
    const int to_edge = (int)((G - (g0 & (G - 1))) & (G - 1));
    head = to_edge < cnt ? to_edge : cnt;
    groups = (cnt - head) / G;
  }
  const int tail0 = head + groups * G;
  for (int i = threadIdx.x; i < head; i += kTileBlock) col[g0 + i] = (T)lds[i];
  for (int g = threadIdx.x; g < groups; g += kTileBlock) {
    const int i = head + g * G;
    if constexpr (sizeof(T) == 8)
      *reinterpret_cast<u64x2*>(col + g0 + i) = u64x2{lds[i], lds[i + 1]};
    else
      *reinterpret_cast<u32x4*>(col + g0 + i) =
          u32x4{(uint32_t)lds[i], (uint32_t)lds[i + 1], (uint32_t)lds[i + 2], (uint32_t)lds[i + 3]};
  }
  for (int i = tail0 + threadIdx.x; i < cnt; i += kTileBlock) col[g0 + i] = (T)lds[i];
}

// The selected records of a tile lie at adjacent indices of the outputs: the
// tile's first at out0 = (keys below in the tiles before) + min(equal keys in
// the tiles before, share), a record at out0's formula with the counts in
// front of it inside the tile added (a 64-entry scan of the (wave, item)
// cells in LDS, then the lanes below it in its cell's ballots).  The tile's
// decoded keys and values are staged in LDS in that order and stored from
// there, so every store instruction writes adjacent elements.  The tile's own
// recount must equal the count's tile_cnt; otherwise A has changed since,
// *err is set and the tile writes nothing.  No index leaves [0, take).
template <typename KeyT, int ValBytes, bool VEC>
__global__ __launch_bounds__(kTileBlock) void k_sel_write(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         uint64_t pivot, int64_t share, int64_t take,
                                                         const uint32_t* __restrict__ tile_cnt,
                                                         const int64_t* __restrict__ tile_base,
                                                         KeyT* __restrict__ keys, int key_type, int flags,
                                                         void* __restrict__ vals, uint32_t* __restrict__ err) {
  __shared__ uint32_t s_cell[kTileCells];
  __shared__ uint32_t s_total;
  __shared__ uint64_t s_key[kTile];
  __shared__ uint64_t s_val[ValBytes ? kTile : 1];
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(key_type, flags);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kTileItems], val[kTileItems], lt[kTileItems], eq[kTileItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kTileWaveRecs;
    wave_compare<ValBytes != 0>(A, here, wave0, pivot, key, val, lt, eq);
    // both counts in one word, scanned at once: no carry between the halves, kTile < 2^16
    tile_cells(s_cell, &s_total,
               [&](int j) { return (uint32_t)__popcll(lt[j]) | ((uint32_t)__popcll(eq[j]) << 16); });
    const int64_t lt0 = tile_base[2 * tile], eq0 = tile_base[2 * tile + 1];
    const int64_t taken0 = eq0 < share ? eq0 : share;  // equal keys taken in the tiles before
    const int64_t out0 = lt0 + taken0;
    const int64_t eq1 = eq0 + (int64_t)(s_total >> 16);
    const int cnt = (int)(s_total & 0xffffu) + (int)((eq1 < share ? eq1 : share) - taken0);
    const bool good = s_total == tile_cnt[tile] && out0 >= 0 && out0 + cnt <= take;
    if (!good) {
      if (threadIdx.x == 0) atomicOr(err, 1u);
    } else {
#pragma unroll
      for (int j = 0; j < kTileItems; ++j) {
        const uint32_t cell = s_cell[wave * kTileItems + j];
        const int64_t e = eq0 + (int64_t)(cell >> 16) + tile_mbcnt(eq[j]);  // equal keys in front of this record
        const bool is_lt = (lt[j] >> lane) & 1, is_eq = (eq[j] >> lane) & 1;
        if (is_lt || (is_eq && e < share)) {
          const int at = (int)(cell & 0xffffu) + (int)tile_mbcnt(lt[j]) + (int)((e < share ? e : share) - taken0);
          if (keys) s_key[at] = decode(key[j], form);
          if constexpr (ValBytes != 0) s_val[at] = val[j];
        }
      }
    }
    __syncthreads();
    if (good) {
      if (keys) store_range<KeyT, VEC>(keys, out0, cnt, s_key);
      if constexpr (ValBytes == 8) store_range<uint64_t, VEC>(static_cast<uint64_t*>(vals), out0, cnt, s_val);
      if constexpr (ValBytes == 4) store_range<uint32_t, VEC>(static_cast<uint32_t*>(vals), out0, cnt, s_val);
    }
    __syncthreads();
  }
}

int sel_grid(int64_t tiles) { return (int)(tiles < 1 ? 1 : (tiles > kSelGridCap ? kSelGridCap : tiles)); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename KeyT, int ValBytes>
void select_write_form(const Elem* A, int64_t here, uint64_t pivot, int64_t share, int64_t take,
                       const uint32_t* tile_cnt, const int64_t* tile_base, void* keys, int key_type, int flags,
                       void* vals, uint32_t* err, hipStream_t s) {
  const int64_t tiles = run_tiles(here);
  const dim3 grid(sel_grid(tiles)), block(kTileBlock);
  if (aligned16(keys) && aligned16(vals))
    hipLaunchKernelGGL((k_sel_write<KeyT, ValBytes, true>), grid, block, 0, s, A, here, tiles, pivot, share, take,
                       tile_cnt, tile_base, static_cast<KeyT*>(keys), key_type, flags, vals, err);
  else
    hipLaunchKernelGGL((k_sel_write<KeyT, ValBytes, false>), grid, block, 0, s, A, here, tiles, pivot, share, take,
                       tile_cnt, tile_base, static_cast<KeyT*>(keys), key_type, flags, vals, err);
}

}  // namespace

hipError_t launch_select_hist(const Elem* src, int64_t m, int shift, uint64_t prefix, uint64_t mask, bool span,
                              Elem* dst, int64_t bound, uint64_t* words, hipStream_t s) {
  if (!src || m <= 0 || !words || shift < 0 || shift > 56 || (shift & 7) || (prefix & ~mask) || (span && dst) ||
      (dst && bound <= 0))
    return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(m);
  const dim3 grid(sel_grid(tiles)), block(kTileBlock);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(words);
  if (span)
    hipLaunchKernelGGL((k_sel_hist<true, false>), grid, block, 0, s, src, m, tiles, shift, prefix, mask, dst, bound, w);
  else if (dst)
    hipLaunchKernelGGL((k_sel_hist<false, true>), grid, block, 0, s, src, m, tiles, shift, prefix, mask, dst, bound, w);
  else
    hipLaunchKernelGGL((k_sel_hist<false, false>), grid, block, 0, s, src, m, tiles, shift, prefix, mask, dst, bound,
                       w);
  return hipGetLastError();
}

hipError_t launch_select_count(const Elem* A, int64_t here, uint64_t pivot, int64_t below, int64_t equal,
                               uint32_t* tile_cnt, int64_t* tile_base, uint32_t* err, hipStream_t s) {
  if (here <= 0 || !A || !tile_cnt || !tile_base || !err || below < 0 || equal < 0) return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  hipLaunchKernelGGL(k_sel_count, dim3(sel_grid(tiles)), dim3(kTileBlock), 0, s, A, here, tiles, pivot, tile_cnt);
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kSelScanBlock), 0, s, tiles, tile_cnt, tile_base, below, equal, err);
  return hipGetLastError();
}

hipError_t launch_select_write(const Elem* A, int64_t here, uint64_t pivot, int64_t share, int64_t take,
                               const uint32_t* tile_cnt, const int64_t* tile_base, void* keys, int key_type, int flags,
                               void* vals, int val_bytes, uint32_t* err, hipStream_t s) {
  if (!key_form_valid(key_type, flags) || (!keys && !vals) || (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) ||
      (val_bytes == 0) != (vals == nullptr) || !A || !tile_cnt || !tile_base || !err || share < 0 || take < share)
    return hipErrorInvalidValue;
  if (here <= 0 || take <= 0) return hipSuccess;
  const bool k32 = key_bytes(key_type) == 4;
  if (val_bytes == 8) {
    if (k32) select_write_form<uint32_t, 8>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
    else select_write_form<uint64_t, 8>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
  } else if (val_bytes == 4) {
    if (k32) select_write_form<uint32_t, 4>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
    else select_write_form<uint64_t, 4>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
  } else {
    if (k32) select_write_form<uint32_t, 0>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
    else select_write_form<uint64_t, 0>(A, here, pivot, share, take, tile_cnt, tile_base, keys, key_type, flags, vals, err, s);
  }
  return hipGetLastError();
}

}  // namespace lsb
