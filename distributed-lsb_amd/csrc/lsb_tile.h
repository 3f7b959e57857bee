// The tile skeleton of the kernels that walk A a tile at a time with a head
// numbering inside the tile (lsb_runs.hip, lsb_select.hip):
// the workgroup's geometry, the lane helpers, the scan of the (wave, item)
// cells and the recount guard.  Device code: for .hip units only.
#pragma once
#include "lsb_kernels.h"

namespace lsb {

// A workgroup of four waves takes a tile.  A wave takes kTileWaveRecs adjacent
// records, lane-striped: item j of lane l is position wave0 + 64 j + l.
constexpr int kTileBlock = 256;
constexpr int kTileWaves = kTileBlock / 64;
constexpr int kTileItems = kTile / kTileBlock;        // records per lane and tile
constexpr int kTileWaveRecs = kTile / kTileWaves;     // a wave's adjacent records of a tile
constexpr int kTileCells = kTileWaves * kTileItems;   // (wave, item) cells of a tile, in position order
static_assert(kTileCells == 64, "tile_cells scans the cells in one wave");

__device__ __forceinline__ int tile_lane() { return (int)(threadIdx.x & 63); }

// Set bits of mask below this lane.
__device__ __forceinline__ uint32_t tile_mbcnt(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The (wave, item) cells of a tile in s_cell[kTileCells]: cell (wave, j) takes
// mine(j), a count that is the same in every lane of the wave; wave 0 turns the
// counts into their exclusive prefixes in position order and leaves their sum
// in *s_total.  A plain 32-bit add: two 16-bit counts packed into a word scan
// as two, while neither sum leaves its half.  Every thread of the workgroup
// calls it.  Two barriers inside, behind the counts and behind the scan; the
// caller puts another before the next tile's call, which writes s_cell again.
template <typename Mine>
__device__ __forceinline__ void tile_cells(uint32_t* s_cell, uint32_t* s_total, Mine&& mine) {
  const int lane = tile_lane(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int j = 0; j < kTileItems; ++j)
    if (lane == j) s_cell[wave * kTileItems + j] = mine(j);
  __syncthreads();
  if (wave == 0) {
    const uint32_t c = s_cell[lane];
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    s_cell[lane] = incl - c;
    if (lane == 63) *s_total = incl;
  }
  __syncthreads();
}

// Position 0 of the rank is a head by the plan's word (head0), not by a
// comparison, so the count's tile_cnt[0] leaves it out: what a recount of the
// tile holds on top of tile_cnt[tile].
__device__ __forceinline__ uint32_t tile_first(int64_t tile, uint32_t head0) { return tile == 0 ? head0 : 0u; }

// The recount guard: whether the tile's own count of its heads, `total` (the
// same in every thread), is the count's tile_cnt[tile], so that the tile may
// write.  Otherwise A has changed since lsb_count_runs: thread 0 sets *err and
// the caller writes nothing, so no index leaves the outputs.
__device__ __forceinline__ bool tile_recount(uint32_t total, int64_t tile, uint32_t head0,
                                             const uint32_t* __restrict__ tile_cnt, uint32_t* __restrict__ err) {
  if (total - tile_first(tile, head0) == tile_cnt[tile]) return true;
  if (threadIdx.x == 0) atomicOr(err, 1u);
  return false;
}

}  // namespace lsb
