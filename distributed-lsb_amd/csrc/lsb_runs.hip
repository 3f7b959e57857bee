// Runs of equal keys (lsb_count_runs / lsb_store_runs, include/lsb.h;
// DESIGN.md §7.2): three plain kernels and a scan.
//   k_run_count  one read of A: heads per tile, the smallest head
//   k_run_scan   one workgroup: tile counts -> exclusive tile bases, the
//                rank's four summary words
//   k_run_write  one more read of A: every head writes its run's key, start
//                and first value at its rank among the heads
//   k_run_diff   counts from adjacent starts
// No workgroup waits for another: a tile's base is ready before k_run_write
// starts.  Positions, bases and counts are 64-bit throughout.
#include "lsb_kernels.h"
#include "lsb_keyform.h"

namespace lsb {

namespace {

constexpr int kRunBlock = 256;                    // 4 waves
constexpr int kRunWaves = kRunBlock / 64;
constexpr int kRunItems = kTile / kRunBlock;      // records per lane and tile
constexpr int kRunWaveRecs = kTile / kRunWaves;   // a wave's adjacent records of a tile
constexpr int kRunCells = kRunWaves * kRunItems;  // (wave, item) cells of a tile, in position order
constexpr int kRunGridCap = 8192;
constexpr int kRunScanBlock = 1024;
static_assert(kRunCells == 64, "k_run_write scans the cells in one wave");

__device__ __forceinline__ int run_lane() { return (int)(threadIdx.x & 63); }

// Set bits of mask below this lane.
__device__ __forceinline__ uint32_t run_mbcnt(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

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

// One wave's kRunWaveRecs records from position wave0 on, lane-striped: item
// j of lane l is position wave0 + 64 j + l, so every load instruction reads
// 1 KiB of adjacent records in 16-byte accesses.  heads[j] = ballot of the
// item's heads (positions >= here have none; position 0 is one exactly when
// head0).  A record's predecessor key comes from the lane below it, lane 0's
// from lane 63 of the item before; only item 0 of lane 0 loads A[wave0 - 1].
// Every lane of the wave must call it.
template <bool VALS>
__device__ __forceinline__ void wave_heads(const Elem* __restrict__ A, int64_t here, int64_t wave0, bool head0,
                                           uint64_t (&key)[kRunItems], uint64_t (&val)[kRunItems],
                                           uint64_t (&heads)[kRunItems]) {
  const int lane = run_lane();
#pragma unroll
  for (int j = 0; j < kRunItems; ++j) {
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
  for (int j = 0; j < kRunItems; ++j) {
    const int64_t i = wave0 + j * 64 + lane;
    const uint64_t prev = prev_lane(key[j], edge);
    const bool head = i < here && (i == 0 ? head0 : key[j] != prev);
    heads[j] = __ballot(head);
    edge = last_lane(key[j]);
  }
}

// tile_cnt[t] = heads of tile t (position 0 is never one); *lead = the
// smallest head of the rank, when it is below the value *lead held.
__global__ __launch_bounds__(kRunBlock) void k_run_count(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         uint32_t* __restrict__ tile_cnt,
                                                         unsigned long long* __restrict__ lead) {
  __shared__ uint32_t s_cnt[kRunWaves], s_first[kRunWaves];
  const int wave = (int)(threadIdx.x >> 6);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kRunItems], val[kRunItems], heads[kRunItems];
    wave_heads<false>(A, here, tile * kTile + (int64_t)wave * kRunWaveRecs, false, key, val, heads);
    uint32_t cnt = 0, first = kTile;  // the same in every lane
#pragma unroll
    for (int j = kRunItems - 1; j >= 0; --j) {
      cnt += (uint32_t)__popcll(heads[j]);
      if (heads[j]) first = (uint32_t)(wave * kRunWaveRecs + j * 64 + __builtin_ctzll(heads[j]));
    }
    if (run_lane() == 0) {
      s_cnt[wave] = cnt;
      s_first[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0, f = kTile;
#pragma unroll
      for (int w = 0; w < kRunWaves; ++w) {
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
// adjacent heads write adjacent elements.  The tile's own recount must equal
// the count's tile_cnt; otherwise A has changed since, *err is set and the
// tile writes nothing, so no index leaves [0, runs).
__global__ __launch_bounds__(kRunBlock) void k_run_write(const Elem* __restrict__ A, int64_t here, int64_t tiles,
                                                         int64_t gbase, uint32_t head0,
                                                         const uint32_t* __restrict__ tile_cnt,
                                                         const int64_t* __restrict__ tile_base, void* __restrict__ keys,
                                                         int key_type, int flags, int64_t* __restrict__ starts,
                                                         void* __restrict__ firsts, int val_bytes,
                                                         uint32_t* __restrict__ err) {
  __shared__ uint32_t s_cell[kRunCells];
  __shared__ uint32_t s_total;
  const int lane = run_lane(), wave = (int)(threadIdx.x >> 6);
  const KeyForm form = key_form(key_type, flags);
  const bool k32 = key_bytes(key_type) == 4;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint64_t key[kRunItems], val[kRunItems], heads[kRunItems];
    const int64_t wave0 = tile * kTile + (int64_t)wave * kRunWaveRecs;
    wave_heads<true>(A, here, wave0, head0 != 0, key, val, heads);
#pragma unroll
    for (int j = 0; j < kRunItems; ++j)
      if (lane == j) s_cell[wave * kRunItems + j] = (uint32_t)__popcll(heads[j]);
    __syncthreads();
    if (wave == 0) {  // cell counts -> exclusive prefixes, and their total
      const uint32_t c = s_cell[lane];
      uint32_t incl = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      s_cell[lane] = incl - c;
      if (lane == 63) s_total = incl;
    }
    __syncthreads();
    const uint32_t first = tile == 0 ? head0 : 0u;  // position 0 is the plan's, not the count's
    if (s_total - first != tile_cnt[tile]) {
      if (threadIdx.x == 0) atomicOr(err, 1u);
    } else {
      const int64_t out0 = tile_base[tile] + (int64_t)(head0 - first);
#pragma unroll
      for (int j = 0; j < kRunItems; ++j) {
        if ((heads[j] >> lane) & 1) {
          const int64_t h = out0 + s_cell[wave * kRunItems + j] + run_mbcnt(heads[j]);
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

// counts[j] = starts[j + 1] - starts[j]; the last run ends at `end`.
__global__ __launch_bounds__(256) void k_run_diff(const int64_t* __restrict__ starts, int64_t* __restrict__ counts,
                                                  int64_t runs, int64_t end) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < runs; j += stride)
    counts[j] = (j + 1 < runs ? starts[j + 1] : end) - starts[j];
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
  hipLaunchKernelGGL(k_run_count, dim3(run_grid(tiles, 1)), dim3(kRunBlock), 0, s, A, here, tiles, tile_cnt,
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
  hipLaunchKernelGGL(k_run_write, dim3(run_grid(tiles, 1)), dim3(kRunBlock), 0, s, A, here, tiles, gbase,
                     (uint32_t)head0, tile_cnt, tile_base, keys, key_type, flags, starts, firsts, val_bytes, err);
  if (counts)
    hipLaunchKernelGGL(k_run_diff, dim3(run_grid(runs, 256)), dim3(256), 0, s, starts, counts, runs, end);
  return hipGetLastError();
}

}  // namespace lsb
