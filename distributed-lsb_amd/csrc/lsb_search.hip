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
// The kernels that hand the matches back (lsb_lookup, lsb_join_count,
// lsb_store_join) stand behind k_search and search with the
// same bound<> and run_from.
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

// ---- lookup and join (lsb_lookup, lsb_join_count, lsb_store_join) ----
//   k_lookup        k_search's loop with the lower bound, one key compare, a
//                   guarded store of the first match's value and the found byte
//   k_join_count    per query its lower bound and its run (k_search's COUNT,
//                   both numbers kept), and the runs' sum per tile of queries
//   k_join_scan     one workgroup: tile sums -> exclusive tile bases, in sweeps
//   k_join_offsets  counts -> exclusive offsets, in place, a tile per workgroup
//   k_join_expand   a tile of outputs per workgroup: the queries that meet it
//                   by two wave-wide searches of the offsets, their offsets in
//                   LDS, then every output finds its query there
// Reduce-then-scan, as the tile counts of lsb_runs.hip and lsb_select.hip: no
// kernel waits for another workgroup.
constexpr int kJoinQItems = kJoinQTile / kSearchBlock;
constexpr int kJoinScanSweep = 256;  // tile sums k_join_scan takes per sweep, one per thread
constexpr int kJoinBlock = 256;      // 4 waves
constexpr int kJoinTile = 2048;      // T: outputs per workgroup of k_join_expand
constexpr int kJoinSpan = 4096;      // S: offsets a workgroup stages in LDS (32 KiB); a longer span is searched in global memory
constexpr int kJoinItems = kJoinTile / kJoinBlock;
static_assert(kJoinQTile % kSearchBlock == 0 && kJoinTile % kJoinBlock == 0 && kSearchBlock == 256, "join tile shapes");

// top[j] = fence[j * step], as k_search stages it; the barrier included.
__device__ __forceinline__ int64_t stage_top(const uint64_t* __restrict__ fence, int64_t tiles, uint64_t* top) {
  const int64_t step = (tiles + kSearchTop - 1) / kSearchTop;
  for (int64_t j = threadIdx.x; j * step < tiles; j += kSearchBlock) top[j] = fence[j * step];  // j < kSearchTop
  __syncthreads();
  return step;
}

// Grid-stride as k_search.  A query with a match writes the elements it owns;
// one without touches nothing.
template <typename KeyT>
__global__ __launch_bounds__(kSearchBlock) void k_lookup(const Elem* __restrict__ A, int64_t here,
                                                         const uint64_t* __restrict__ fence, int64_t tiles,
                                                         const KeyT* __restrict__ queries, int64_t m, int key_type,
                                                         int flags, void* __restrict__ vals, int val_bytes,
                                                         uint8_t* __restrict__ found) {
  __shared__ uint64_t top[kSearchTop];
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(A);
  const KeyForm form = key_form(key_type, flags);
  const uint64_t first = fence[0], last = keys[2 * (here - 1)];
  const int64_t step = stage_top(fence, tiles, top);
  const int64_t stride = (int64_t)gridDim.x * kSearchBlock;
  for (int64_t i = (int64_t)blockIdx.x * kSearchBlock + threadIdx.x; i < m; i += stride) {
    const uint64_t e = encode((uint64_t)__builtin_nontemporal_load(queries + i), form);
    const int64_t lo = bound<false>(keys, here, fence, tiles, top, step, first, last, e);
    LSB_SEARCH_ASSERT(lo >= 0 && lo <= here);
    if (lo >= here || keys[2 * lo] != e) continue;
    if (val_bytes == 8) static_cast<uint64_t*>(vals)[i] = keys[2 * lo + 1];
    else if (val_bytes == 4) static_cast<uint32_t*>(vals)[i] = (uint32_t)keys[2 * lo + 1];
    if (found) found[i] = 1;
  }
}

// A tile of kJoinQTile queries per workgroup and sweep, lane-striped: lower[i]
// and cnt[i] of every query, counts[i] = cnt[i] too when given, and
// tile_sum[t] = the tile's sum of cnt.  lower[i] + cnt[i] <= here whatever A
// holds (bound<> and run_from).
template <typename KeyT>
__global__ __launch_bounds__(kSearchBlock) void k_join_count(const Elem* __restrict__ A, int64_t here,
                                                             const uint64_t* __restrict__ fence, int64_t tiles,
                                                             const KeyT* __restrict__ queries, int64_t m, int key_type,
                                                             int flags, int64_t* __restrict__ lower,
                                                             int64_t* __restrict__ cnt, int64_t* __restrict__ counts,
                                                             int64_t* __restrict__ tile_sum) {
  __shared__ uint64_t top[kSearchTop];
  __shared__ int64_t s_wave[kSearchBlock / 64];
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(A);
  const KeyForm form = key_form(key_type, flags);
  const uint64_t first = fence[0], last = keys[2 * (here - 1)];
  const int64_t step = stage_top(fence, tiles, top);
  const int64_t qtiles = join_qtiles(m);
  for (int64_t t = blockIdx.x; t < qtiles; t += gridDim.x) {
    int64_t sum = 0;
    for (int j = 0; j < kJoinQItems; ++j) {
      const int64_t i = t * kJoinQTile + j * kSearchBlock + threadIdx.x;
      if (i >= m) break;
      const uint64_t e = encode((uint64_t)__builtin_nontemporal_load(queries + i), form);
      const int64_t lo = bound<false>(keys, here, fence, tiles, top, step, first, last, e);
      const int64_t c = run_from(keys, here, e, lo);
      LSB_SEARCH_ASSERT(lo >= 0 && c >= 0 && lo + c <= here);
      lower[i] = lo;
      cnt[i] = c;
      if (counts) counts[i] = c;
      sum += c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[t] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
}

// One workgroup: tile[t] = the sums of the tiles before t, in place, and
// tile[qtiles] = the sum of all.  kJoinScanSweep tiles per sweep, one per
// thread; the sweeps before are carried in a register that every thread keeps.
__global__ __launch_bounds__(kJoinScanSweep) void k_join_scan(int64_t qtiles, int64_t* __restrict__ tile) {
  __shared__ int64_t s[kJoinScanSweep];
  const int tid = (int)threadIdx.x;
  int64_t carry = 0;
  for (int64_t t0 = 0; t0 < qtiles; t0 += kJoinScanSweep) {
    const int64_t t = t0 + tid;
    const int64_t mine = t < qtiles ? tile[t] : 0;
    s[tid] = mine;
    __syncthreads();
    for (int off = 1; off < kJoinScanSweep; off <<= 1) {
      const int64_t a = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += a;
      __syncthreads();
    }
    if (t < qtiles) tile[t] = carry + s[tid] - mine;
    carry += s[kJoinScanSweep - 1];
    __syncthreads();  // s is written again
  }
  if (tid == 0) tile[qtiles] = carry;
}

// A tile of kJoinQTile counts per workgroup and sweep, kJoinQItems adjacent
// ones per thread: cnt[i] -> tile_base[t] + the counts of the tile in front
// of i, in place.
__global__ __launch_bounds__(kSearchBlock) void k_join_offsets(int64_t m, const int64_t* __restrict__ tile_base,
                                                               int64_t* __restrict__ cnt) {
  __shared__ int64_t s_wave[kSearchBlock / 64];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int64_t qtiles = join_qtiles(m);
  for (int64_t t = blockIdx.x; t < qtiles; t += gridDim.x) {
    const int64_t i0 = t * kJoinQTile + (int64_t)threadIdx.x * kJoinQItems;
    int64_t c[kJoinQItems];
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < kJoinQItems; ++j) {
      c[j] = i0 + j < m ? cnt[i0 + j] : 0;
      sum += c[j];
    }
    int64_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int64_t base = tile_base[t] + incl - sum;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
#pragma unroll
    for (int j = 0; j < kJoinQItems; ++j) {
      if (i0 + j < m) cnt[i0 + j] = base;
      base += c[j];
    }
    __syncthreads();
  }
}

// The entries of off[0, m) that are not above x (off ascending, off[0] <= x
// in every call: >= 1), by one whole wave: its lanes probe 64 places spread
// over the range, the ballot tells between which two the answer lies.  Every
// probe index lies in [0, m); the result is the same in every lane.
__device__ __forceinline__ int64_t wave_not_above(const int64_t* __restrict__ off, int64_t m, int64_t x) {
  const int lane = (int)(threadIdx.x & 63);
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t idx = lo + lane * step;
    LSB_SEARCH_ASSERT(idx >= 0 && (idx >= hi || idx < m));
    const bool in = idx < hi && off[idx] <= x;
    const int k = __popcll(__ballot(in));  // the probes that are not above x: a prefix of the lanes
    if (k == 0) {
      hi = lo;
    } else {
      const int64_t end = lo + k * step;
      lo += (k - 1) * step + 1;
      hi = end < hi ? end : hi;
    }
  }
  return lo;
}

// base[j] = the last index k of a[0, len) with a[k] <= x[j], for N values at
// once; a ascending, len >= 1 and a[0] <= x[j].  The trip count depends on len
// alone, so the N searches advance together and their loads overlap.
template <int N>
__device__ __forceinline__ void last_not_above(const int64_t* a, int64_t len, const int64_t (&x)[N], int64_t (&base)[N]) {
  const int64_t n = len;
  (void)n;
#pragma unroll
  for (int j = 0; j < N; ++j) base[j] = 0;
  while (len > 1) {
    const int64_t half = len >> 1;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      LSB_SEARCH_ASSERT(base[j] >= 0 && base[j] + half < n);
      if (a[base[j] + half] <= x[j]) base[j] += half;
    }
    len -= half;
  }
}

// Workgroup b writes the outputs [b * kJoinTile, (b + 1) * kJoinTile) of
// [0, total): output o of query i = the last one with off[i] <= o (the
// queries without a match share their successor's offset and are never the
// last) is record p = lower[i] + o - off[i].  Adjacent lanes take adjacent
// outputs, and inside one query's range adjacent records.
__global__ __launch_bounds__(kJoinBlock) void k_join_expand(const Elem* __restrict__ A, int64_t here,
                                                            const int64_t* __restrict__ lower,
                                                            const int64_t* __restrict__ off, int64_t m, int64_t total,
                                                            int64_t query_base, int64_t gbase,
                                                            int64_t* __restrict__ left, void* __restrict__ right,
                                                            int val_bytes, int64_t* __restrict__ pos) {
  __shared__ int64_t s_off[kJoinSpan];
  __shared__ int64_t s_q[2];
  const int tid = (int)threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * kJoinTile;
  const int64_t o1 = o0 + kJoinTile < total ? o0 + kJoinTile : total;  // o0 < total: the grid is ceil(total / kJoinTile)
  // The first and the last query whose outputs meet the tile, one wave each.
  if (tid < 128) {
    const int64_t q = wave_not_above(off, m, tid < 64 ? o0 : o1 - 1) - 1;
    if ((tid & 63) == 0) s_q[tid >> 6] = q;
  }
  __syncthreads();
  const int64_t q0 = s_q[0], span = s_q[1] - q0 + 1;
  LSB_SEARCH_ASSERT(q0 >= 0 && span >= 1 && q0 + span <= m);
  const bool staged = span <= kJoinSpan;  // the same in every thread
  if (staged) {
    for (int64_t k = tid; k < span; k += kJoinBlock) s_off[k] = off[q0 + k];
    __syncthreads();
  }
  int64_t o[kJoinItems], k[kJoinItems];
#pragma unroll
  for (int j = 0; j < kJoinItems; ++j) {
    const int64_t mine = o0 + j * kJoinBlock + tid;
    o[j] = mine < o1 ? mine : o1 - 1;  // past the end: searched like the last output, not stored
  }
  if (staged) last_not_above(s_off, span, o, k);
  else last_not_above(off + q0, span, o, k);
#pragma unroll
  for (int j = 0; j < kJoinItems; ++j) {
    if (o0 + j * kJoinBlock + tid >= o1) continue;
    const int64_t i = q0 + k[j];
    const int64_t p = lower[i] + (o[j] - (staged ? s_off[k[j]] : off[i]));
    LSB_SEARCH_ASSERT(i >= 0 && i < m && p >= 0 && p < here && o[j] >= 0 && o[j] < total);
    if (left) left[o[j]] = query_base + i;
    if (val_bytes == 8) static_cast<uint64_t*>(right)[o[j]] = A[p].val;
    else if (val_bytes == 4) static_cast<uint32_t*>(right)[o[j]] = (uint32_t)A[p].val;
    if (pos) pos[o[j]] = gbase + p;
  }
}

}  // namespace

hipError_t launch_lookup(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                         int key_type, int flags, void* vals, int val_bytes, uint8_t* found, hipStream_t s) {
  if (!A || here <= 0 || !fence || !queries || m <= 0 || !key_form_valid(key_type, flags) ||
      (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) || (val_bytes == 0) != (vals == nullptr) ||
      (!vals && !found))
    return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here);
  const dim3 grid(search_grid(m)), block(kSearchBlock);
  if (key_bytes(key_type) == 4)
    hipLaunchKernelGGL(k_lookup<uint32_t>, grid, block, 0, s, A, here, fence, tiles,
                       static_cast<const uint32_t*>(queries), m, key_type, flags, vals, val_bytes, found);
  else
    hipLaunchKernelGGL(k_lookup<uint64_t>, grid, block, 0, s, A, here, fence, tiles,
                       static_cast<const uint64_t*>(queries), m, key_type, flags, vals, val_bytes, found);
  return hipGetLastError();
}

hipError_t launch_join_count(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                             int key_type, int flags, int64_t* lower, int64_t* off, int64_t* counts, int64_t* tile,
                             hipStream_t s) {
  if (!A || here <= 0 || !fence || !queries || m <= 0 || !key_form_valid(key_type, flags) || !lower || !off || !tile)
    return hipErrorInvalidValue;
  const int64_t tiles = run_tiles(here), qtiles = join_qtiles(m);
  const dim3 grid((unsigned)(qtiles > kSearchGridCap ? kSearchGridCap : qtiles)), block(kSearchBlock);
  if (key_bytes(key_type) == 4)
    hipLaunchKernelGGL(k_join_count<uint32_t>, grid, block, 0, s, A, here, fence, tiles,
                       static_cast<const uint32_t*>(queries), m, key_type, flags, lower, off, counts, tile);
  else
    hipLaunchKernelGGL(k_join_count<uint64_t>, grid, block, 0, s, A, here, fence, tiles,
                       static_cast<const uint64_t*>(queries), m, key_type, flags, lower, off, counts, tile);
  hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(kJoinScanSweep), 0, s, qtiles, tile);
  hipLaunchKernelGGL(k_join_offsets, grid, block, 0, s, m, tile, off);
  return hipGetLastError();
}

hipError_t launch_join_expand(const Elem* A, int64_t here, const int64_t* lower, const int64_t* off, int64_t m,
                              int64_t total, int64_t query_base, int64_t gbase, int64_t* left, void* right,
                              int val_bytes, int64_t* pos, hipStream_t s) {
  const int64_t blocks = total > 0 ? (total + kJoinTile - 1) / kJoinTile : 0;
  if (!A || here <= 0 || !lower || !off || m <= 0 || total <= 0 || total > m * here || blocks > 0x7fffffff ||
      (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) || (val_bytes == 0) != (right == nullptr) ||
      (!left && !right && !pos))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_join_expand, dim3((unsigned)blocks), dim3(kJoinBlock), 0, s, A, here, lower, off, m, total,
                     query_base, gbase, left, right, val_bytes, pos);
  return hipGetLastError();
}

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
