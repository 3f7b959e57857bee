// Searching a rank's sorted records for a column of queries: lower bound,
// upper bound and match count (lsb_search, include/lsb.h).
//   k_search_fence  one strided read of A: fence[t] = the key of record
//                   t * kTile, the library's tile
//   k_search        one query per thread: the two early-outs against the
//                   rank's first and last key, a binary search of the fence
//                   table for the tile (its top level staged in LDS), a binary
//                   search of that tile's records; COUNT then gallops from the
//                   lower bound over the run
// A latency-bound gather: every probe depends on the one before.  What makes it
// cheap is where the probes are served from: every kSearchTop-th part of the
// fence table from LDS, the rest of it (8 bytes per 4096 records) from L2, and
// of a tile's 12 probes the last few from one cache line.  The searches are
// bounded by construction: a probe index comes from [lo, hi) of a range that
// starts inside the rank's records and only shrinks, so unsorted records give
// unspecified counts, never a read outside A.
#include "lsb_kernels.h"
#include "lsb_keyform.h"

#ifdef LSB_DEBUG
#include <cassert>
#define LSB_SEARCH_ASSERT(c) assert(c)
#else
#define LSB_SEARCH_ASSERT(c) ((void)0)
#endif

namespace lsb {

namespace {

constexpr int kSearchBlock = 256;     // 4 waves
constexpr int kSearchTop = 1024;      // fences a workgroup stages in LDS (8 KiB): every ceil(tiles / 1024)-th
constexpr int kSearchGridCap = 2048;  // 8 workgroups per CU: every wave slot; the queries beyond are strided over

__global__ __launch_bounds__(kSearchBlock) void k_search_fence(const Elem* __restrict__ A, int64_t tiles,
                                                               uint64_t* __restrict__ fence) {
  const int64_t stride = (int64_t)gridDim.x * kSearchBlock;
  for (int64_t t = (int64_t)blockIdx.x * kSearchBlock + threadIdx.x; t < tiles; t += stride)
    fence[t] = __builtin_nontemporal_load(&A[t * kTile].key);  // one key per 64 KiB: nothing to keep
}

// Does a record with key k count for query e: below it (LOWER), or not above.
template <bool UPPER>
__device__ __forceinline__ bool counts(uint64_t k, uint64_t e) {
  return UPPER ? k <= e : k < e;
}

// The records of A[0, here) that count for e, A sorted: those in front of the
// first that does not.  first = fence[0], last = the key of record here - 1;
// top[j] = fence[j * step] for every j * step < tiles.  The comparison that
// walks the records also picks the tile, so with a key that fills whole tiles
// (equal adjacent fences) LOWER lands in the tile before the first such fence
// and UPPER in the tile of the last.  0 <= the result <= here.
template <bool UPPER>
__device__ __forceinline__ int64_t bound(const uint64_t* __restrict__ keys, int64_t here,
                                         const uint64_t* __restrict__ fence, int64_t tiles, const uint64_t* top,
                                         int64_t step, uint64_t first, uint64_t last, uint64_t e) {
  if (!counts<UPPER>(first, e)) return 0;
  if (counts<UPPER>(last, e)) return here;
  // c = the staged fences that count: top[0] = fence[0] does, the others are
  // searched.  1 <= c <= tops.
  const int tops = (int)((tiles + step - 1) / step);
  int c = 1;
  for (int len = tops - c; len > 0;) {
    const int half = len >> 1, mid = c + half;
    LSB_SEARCH_ASSERT(mid >= 1 && mid < tops);
    if (counts<UPPER>(top[mid], e)) {
      c = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  // base = the fences that count: fence[(c - 1) * step] does, fence[c * step]
  // does not (or there is none); those between are searched.  1 <= base <= tiles.
  int64_t base = (int64_t)(c - 1) * step + 1;
  const int64_t fend = (int64_t)c * step < tiles ? (int64_t)c * step : tiles;
  for (int64_t len = fend - base; len > 0;) {
    const int64_t half = len >> 1, mid = base + half;
    LSB_SEARCH_ASSERT(mid >= 1 && mid < tiles);
    if (counts<UPPER>(fence[mid], e)) {
      base = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  // Tile base - 1: its first record counts, the next tile's first does not
  // (or there is none).  The answer lies in (tile0, end], and tile0 < here.
  const int64_t tile0 = (base - 1) * kTile;
  const int64_t end = tile0 + kTile < here ? tile0 + kTile : here;
  int64_t lo = tile0 + 1;
  for (int64_t len = end - lo; len > 0;) {
    const int64_t half = len >> 1, mid = lo + half;
    LSB_SEARCH_ASSERT(mid >= 1 && mid < here);
    if (counts<UPPER>(keys[2 * mid], e)) {
      lo = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return lo;
}

// The records from the lower bound `from` of e on that are not above e, A
// sorted: the run of e.  A gallop from `from`, then a binary search of the last
// step: a query without a match (the common one) costs one probe of the line
// the lower bound's last probes read, a run of r records 2 log2 r probes, and
// no fence.  Every probe lies in [from, here); 0 <= the result <= here - from.
__device__ __forceinline__ int64_t run_from(const uint64_t* __restrict__ keys, int64_t here, uint64_t e,
                                            int64_t from) {
  int64_t b = 1;  // the records [from, from + b / 2) are not above e
  while (b <= here - from) {
    LSB_SEARCH_ASSERT(from + b - 1 >= 0 && from + b - 1 < here);
    if (keys[2 * (from + b - 1)] > e) break;
    b <<= 1;
  }
  int64_t lo = from + (b >> 1);
  const int64_t end = from + b - 1 < here ? from + b - 1 : here;  // this record is above e, or the rank ends
  for (int64_t len = end - lo; len > 0;) {
    const int64_t half = len >> 1, mid = lo + half;
    LSB_SEARCH_ASSERT(mid >= from && mid < here);
    if (keys[2 * mid] <= e) {
      lo = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return lo - from;
}

// Grid-stride, one query per thread and sweep.  Adjacent lanes read adjacent
// queries and write adjacent 8-byte results; ADD reads and writes the element
// this thread owns, so it needs no atomic.
template <typename KeyT, int MODE, bool ADD>
__global__ __launch_bounds__(kSearchBlock) void k_search(const Elem* __restrict__ A, int64_t here,
                                                         const uint64_t* __restrict__ fence, int64_t tiles,
                                                         const KeyT* __restrict__ queries, int64_t m, int key_type,
                                                         int flags, int64_t* __restrict__ out) {
  __shared__ uint64_t top[kSearchTop];
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(A);
  const KeyForm form = key_form(key_type, flags);
  const uint64_t first = fence[0], last = keys[2 * (here - 1)];  // wave-uniform addresses
  const int64_t step = (tiles + kSearchTop - 1) / kSearchTop;
  for (int64_t j = threadIdx.x; j * step < tiles; j += kSearchBlock) top[j] = fence[j * step];  // j < kSearchTop
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kSearchBlock;
  for (int64_t i = (int64_t)blockIdx.x * kSearchBlock + threadIdx.x; i < m; i += stride) {
    const uint64_t e = encode((uint64_t)__builtin_nontemporal_load(queries + i), form);  // read once
    int64_t c;
    if constexpr (MODE == kSearchLower) {
      c = bound<false>(keys, here, fence, tiles, top, step, first, last, e);
    } else if constexpr (MODE == kSearchUpper) {
      c = bound<true>(keys, here, fence, tiles, top, step, first, last, e);
    } else {
      c = run_from(keys, here, e, bound<false>(keys, here, fence, tiles, top, step, first, last, e));
    }
    LSB_SEARCH_ASSERT(c >= 0 && c <= here);
    if constexpr (ADD) c += out[i];
    out[i] = c;
  }
}

int search_grid(int64_t items) {
  const int64_t blocks = (items + kSearchBlock - 1) / kSearchBlock;
  return (int)(blocks < 1 ? 1 : (blocks > kSearchGridCap ? kSearchGridCap : blocks));
}

template <typename KeyT, int MODE>
void search_form(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m, int key_type,
                 int flags, bool add, int64_t* out, hipStream_t s) {
  const int64_t tiles = run_tiles(here);
  const dim3 grid(search_grid(m)), block(kSearchBlock);
  const KeyT* q = static_cast<const KeyT*>(queries);
  if (add)
    hipLaunchKernelGGL((k_search<KeyT, MODE, true>), grid, block, 0, s, A, here, fence, tiles, q, m, key_type, flags,
                       out);
  else
    hipLaunchKernelGGL((k_search<KeyT, MODE, false>), grid, block, 0, s, A, here, fence, tiles, q, m, key_type, flags,
                       out);
}

template <typename KeyT>
void search_type(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m, int key_type,
                 int flags, int mode, int64_t* out, hipStream_t s) {
  const bool add = (mode & kSearchAdd) != 0;
  switch (mode & ~kSearchAdd) {
    case kSearchLower: search_form<KeyT, kSearchLower>(A, here, fence, queries, m, key_type, flags, add, out, s); break;
    case kSearchUpper: search_form<KeyT, kSearchUpper>(A, here, fence, queries, m, key_type, flags, add, out, s); break;
    default: search_form<KeyT, kSearchCount>(A, here, fence, queries, m, key_type, flags, add, out, s); break;
  }
}

}  // namespace

hipError_t launch_search_fence(const Elem* A, int64_t here, uint64_t* fence, hipStream_t s) {
  if (!A || here <= 0 || !fence) return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  hipLaunchKernelGGL(k_search_fence, dim3(search_grid(tiles)), dim3(kSearchBlock), 0, s, A, tiles, fence);
  return hipGetLastError();
}

hipError_t launch_search(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                         int key_type, int flags, int mode, int64_t* out, hipStream_t s) {
  if (!A || here <= 0 || !fence || !queries || m <= 0 || !out || !key_form_valid(key_type, flags) ||
      !search_mode_valid(mode))
    return hipErrorInvalidValue;
  if (key_bytes(key_type) == 4) search_type<uint32_t>(A, here, fence, queries, m, key_type, flags, mode, out, s);
  else search_type<uint64_t>(A, here, fence, queries, m, key_type, flags, mode, out, s);
  return hipGetLastError();
}

}  // namespace lsb
