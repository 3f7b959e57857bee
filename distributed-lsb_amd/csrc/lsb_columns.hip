// Caller-owned columns <-> records (lsb_load_columns / lsb_store_columns,
// include/lsb.h; DESIGN.md "Caller-owned columns"): the caller's separate key
// and value arrays on the device become the {u64 key, u64 val} records the
// passes sort, and back.  Keys go through the order-preserving forms of
// lsb_keyform.h.  Both kernels are pure streams: every byte is read once and
// written once, nothing else is done.  k_rekey (lsb_rekey_columns /
// lsb_rekey_index) is the third: it streams the records in
// place and gathers each one's new key from a caller's column by its value.
#include "lsb_kernels.h"
#include "lsb_keyform.h"

#ifdef LSB_DEBUG
#include <cassert>
#define LSB_REKEY_ASSERT(c) assert(c)
#else
#define LSB_REKEY_ASSERT(c) ((void)0)
#endif

namespace lsb {

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ Elem load_elem(const Elem* p) {
  const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p);
  return Elem{v.x, v.y};
}

__device__ __forceinline__ void store_elem(Elem* p, const Elem& e) {
  *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2(e.key, e.val);
}

// E consecutive column elements at p, zero-extended.  E > 1: p is 16-byte
// aligned and the elements are E * sizeof(T) / 16 accesses of 16 bytes (8-byte
// accesses stream at 0.54-0.70 of the 16-byte rate); E == 1: one element.  A
// column is read once: nontemporal.
template <typename T, int E>
__device__ __forceinline__ void load_column(const T* p, uint64_t (&x)[E]) {
  if constexpr (E == 1) {
    x[0] = __builtin_nontemporal_load(p);
  } else if constexpr (sizeof(T) == 8) {
#pragma unroll
    for (int j = 0; j < E; j += 2) {
      const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p + j));
      x[j] = v.x;
      x[j + 1] = v.y;
    }
  } else {
    static_assert(E % 4 == 0, "32-bit columns: four elements per 16-byte access");
#pragma unroll
    for (int j = 0; j < E; j += 4) {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + j));
      x[j] = v.x;
      x[j + 1] = v.y;
      x[j + 2] = v.z;
      x[j + 3] = v.w;
    }
  }
}

// The inverse: E consecutive column elements (the low words of x for a 32-bit
// column) to p, in 16-byte accesses when E > 1.
template <typename T, int E>
__device__ __forceinline__ void store_column(T* p, const uint64_t (&x)[E]) {
  if constexpr (E == 1) {
    *p = (T)x[0];
  } else if constexpr (sizeof(T) == 8) {
#pragma unroll
    for (int j = 0; j < E; j += 2) *reinterpret_cast<u64x2*>(p + j) = u64x2{x[j], x[j + 1]};
  } else {
    static_assert(E % 4 == 0, "32-bit columns: four elements per 16-byte access");
#pragma unroll
    for (int j = 0; j < E; j += 4)
      *reinterpret_cast<u32x4*>(p + j) =
          u32x4{(uint32_t)x[j], (uint32_t)x[j + 1], (uint32_t)x[j + 2], (uint32_t)x[j + 3]};
  }
}

// Elements per thread and iteration: the vector path takes as many as make
// the narrowest column's access 16 bytes wide (two 64-bit or four 32-bit
// elements); the element path one.
template <typename KeyT, int ValBytes, bool VEC>
constexpr int column_group() {
  return !VEC ? 1 : (sizeof(KeyT) == 4 || ValBytes == 4) ? 4 : 2;
}

// 4 x 4 transpose of one 32-bit word inside every quad of lanes (r = lane & 3,
// all four lanes active): lane r's a[j] becomes lane j's a[r].  Two butterfly
// steps, each one DPP quad permute and two selects per pair of registers.
__device__ __forceinline__ uint32_t quad_xor1(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
}
__device__ __forceinline__ uint32_t quad_xor2(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true);  // quad_perm:[2,3,0,1]
}
__device__ __forceinline__ void quad_transpose(uint32_t (&a)[4], int r) {
  const bool o1 = (r & 1) != 0, o2 = (r & 2) != 0;
#pragma unroll
  for (int i = 0; i < 4; i += 2) {
    const uint32_t t = quad_xor1(o1 ? a[i] : a[i + 1]);
    a[i] = o1 ? t : a[i];
    a[i + 1] = o1 ? a[i + 1] : t;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t t = quad_xor2(o2 ? a[i] : a[i + 2]);
    a[i] = o2 ? t : a[i];
    a[i + 2] = o2 ? a[i + 2] : t;
  }
}
// The same for 64-bit words whose upper halves are zero unless WIDE.
template <bool WIDE>
__device__ __forceinline__ void quad_transpose(uint64_t (&x)[4], int r) {
  uint32_t lo[4], hi[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (uint32_t)x[j];
    hi[j] = (uint32_t)(x[j] >> 32);
  }
  quad_transpose(lo, r);
  if constexpr (WIDE) quad_transpose(hi, r);
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = WIDE ? ((uint64_t)hi[j] << 32) | lo[j] : (uint64_t)lo[j];
}

// A[i] = {encode(keys[i]), value}, i in [0, cnt): value = vals[i] (ValBytes 8,
// or 4 zero-extended) or val0 + i (ValBytes 0).  VEC: keys and vals are
// 16-byte aligned; thread t of the grid takes elements [t * E, (t + 1) * E)
// per iteration, and the cnt % E last elements go one per thread.  !VEC: the
// same element by element, for columns aligned to their element only.
// E == 2: the thread's two records are 32 adjacent bytes, so one store
// instruction fills whole 64-byte blocks from pairs of lanes.  E == 4 would
// leave three quarters of every 64-byte block to the next three instructions
// (measured: 0.76 of a copy's rate where E == 2 runs at 1.17), so the four
// lanes of a quad transpose their 4 x 4 elements first, and each instruction
// stores four adjacent records per quad.
template <typename KeyT, int ValBytes, bool VEC>
__global__ __launch_bounds__(256) void k_load_columns(Elem* __restrict__ A, const KeyT* __restrict__ keys,
                                                      const void* __restrict__ vals, int64_t cnt, uint64_t val0,
                                                      int key_type, int flags) {
  constexpr int E = column_group<KeyT, ValBytes, VEC>();
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t groups = cnt / E;
  const KeyForm form = key_form(key_type, flags);
  if constexpr (E == 4) {
    const int r = threadIdx.x & 3;
    // A quad's four groups start at g - r (tid and stride are multiples of 4
    // apart from r); its lanes stay together while any of them has a group.
    for (int64_t g = tid; g - r < groups; g += stride) {
      uint64_t k[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
      if (g < groups) {
        load_column<KeyT, 4>(keys + g * 4, k);
        if constexpr (ValBytes == 8) load_column<uint64_t, 4>(static_cast<const uint64_t*>(vals) + g * 4, v);
        if constexpr (ValBytes == 4) load_column<uint32_t, 4>(static_cast<const uint32_t*>(vals) + g * 4, v);
      }
      quad_transpose<sizeof(KeyT) == 8>(k, r);
      if constexpr (ValBytes != 0) quad_transpose<ValBytes == 8>(v, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = (g - r) * 4 + 4 * j + r;  // lane j of the quad held it as its r-th element
        if constexpr (ValBytes == 0) v[j] = val0 + (uint64_t)i;
        if (i < groups * 4) store_elem(A + i, Elem{encode(k[j], form), v[j]});
      }
    }
  } else {
    for (int64_t g = tid; g < groups; g += stride) {
      const int64_t i = g * E;
      uint64_t k[E], v[E];
      load_column<KeyT, E>(keys + i, k);
      if constexpr (ValBytes == 8) load_column<uint64_t, E>(static_cast<const uint64_t*>(vals) + i, v);
      if constexpr (ValBytes == 4) load_column<uint32_t, E>(static_cast<const uint32_t*>(vals) + i, v);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if constexpr (ValBytes == 0) v[j] = val0 + (uint64_t)(i + j);
        store_elem(A + i + j, Elem{encode(k[j], form), v[j]});
      }
    }
  }
  if constexpr (E > 1) {
    const int64_t i = groups * E + tid;  // the tail: fewer than E elements
    if (i < cnt) {
      uint64_t k[1], v[1];
      load_column<KeyT, 1>(keys + i, k);
      if constexpr (ValBytes == 8) load_column<uint64_t, 1>(static_cast<const uint64_t*>(vals) + i, v);
      if constexpr (ValBytes == 4) load_column<uint32_t, 1>(static_cast<const uint32_t*>(vals) + i, v);
      if constexpr (ValBytes == 0) v[0] = val0 + (uint64_t)i;
      store_elem(A + i, Elem{encode(k[0], form), v[0]});
    }
  }
}

// keys[i] = decode(A[i].key), vals[i] = A[i].val (ValBytes 8) or its low word
// (ValBytes 4); keys may be null, and vals is null exactly when ValBytes is 0.
// Indexing and paths as k_load_columns.  A thread's E records share one or two
// 128-byte lines, so they are read through L1 (plain loads), which serves the
// second to E-th of them.
template <typename KeyT, int ValBytes, bool VEC>
__global__ __launch_bounds__(256) void k_store_columns(const Elem* __restrict__ A, KeyT* __restrict__ keys,
                                                       void* __restrict__ vals, int64_t cnt, int key_type,
                                                       int flags) {
  constexpr int E = column_group<KeyT, ValBytes, VEC>();
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t groups = cnt / E;
  const KeyForm form = key_form(key_type, flags);
  for (int64_t g = tid; g < groups; g += stride) {
    const int64_t i = g * E;
    uint64_t k[E], v[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const Elem e = load_elem(A + i + j);
      k[j] = decode(e.key, form);
      v[j] = e.val;
    }
    if (keys) store_column<KeyT, E>(keys + i, k);
    if constexpr (ValBytes == 8) store_column<uint64_t, E>(static_cast<uint64_t*>(vals) + i, v);
    if constexpr (ValBytes == 4) store_column<uint32_t, E>(static_cast<uint32_t*>(vals) + i, v);
  }
  if constexpr (E > 1) {
    const int64_t i = groups * E + tid;
    if (i < cnt) {
      const Elem e = load_elem(A + i);
      const uint64_t k[1] = {decode(e.key, form)}, v[1] = {e.val};
      if (keys) store_column<KeyT, 1>(keys + i, k);
      if constexpr (ValBytes == 8) store_column<uint64_t, 1>(static_cast<uint64_t*>(vals) + i, v);
      if constexpr (ValBytes == 4) store_column<uint32_t, 1>(static_cast<uint32_t*>(vals) + i, v);
    }
  }
}

// Records per thread and iteration of k_rekey (E): the gathers one thread has
// in flight together.  Measured at 2, 4 and 8: the permuted
// gather is indifferent, and at 2 a lane's records are 32 adjacent bytes, which
// streams best (as k_load_columns' E == 2).
#ifndef LSB_REKEY_GROUP
#define LSB_REKEY_GROUP 2
#endif
constexpr int kRekeyGroup = LSB_REKEY_GROUP;

enum class RekeyBy { kColumn, kIndex };

// x, as a value the compiler knows nothing about.  It keeps the compiler from
// storing only the half of a record that changed (a value that went through
// here is no longer known to equal memory), and from sinking a gather under
// the branch on its bound: that would make the gathers wait for one another.
__device__ __forceinline__ uint64_t opaque(uint64_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// N adjacent records at a, rekeyed in place by their values v = a[j].val:
//   kColumn  key = encode(col[v]); a record with v >= bound (the column's
//            length, >= 1) keeps its key, and the result is true
//   kIndex   key = v / bound (the divisor, >= 1); col is not looked at
// All N records are read, all N bounds decided and all N gathers issued before
// the first gathered key is used, so a thread's N gathers are in flight
// together.  An out-of-range record gathers col[0] instead, so no address is
// ever formed from its value and the body has no branch; it is written back
// with the key it had.
template <typename KeyT, RekeyBy By, int N>
__device__ __forceinline__ bool rekey_records(Elem* __restrict__ a, const KeyT* __restrict__ col, uint64_t bound,
                                              const KeyForm& form) {
  Elem e[N];
  uint64_t k[N];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) e[j] = load_elem(a + j);
#pragma unroll
  for (int j = 0; j < N; ++j) e[j].val = opaque(e[j].val);
  if constexpr (By == RekeyBy::kColumn) {
    uint64_t at[N];
#pragma unroll
    for (int j = 0; j < N; ++j) at[j] = e[j].val < bound ? e[j].val : 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      LSB_REKEY_ASSERT(at[j] < bound);
      k[j] = col[at[j]];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) k[j] = opaque(k[j]);  // all N gathers are in flight by now
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool in = e[j].val < bound;
      bad |= !in;
      k[j] = in ? encode(k[j], form) : e[j].key;
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) k[j] = e[j].val / bound;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) store_elem(a + j, Elem{k[j], e[j].val});
  return bad;
}

// Slots [0, cnt) of A rekeyed in place (rekey_records).  Thread t of the grid
// takes records [t * E, (t + 1) * E) per iteration, and the cnt % E last
// records go one per thread; every thread writes back only what it read, and
// never a value that differs from the one it read.  kColumn: a wave that met
// an out-of-range value raises *err; kIndex: err is not looked at.
template <typename KeyT, RekeyBy By>
__global__ __launch_bounds__(256) void k_rekey(Elem* __restrict__ A, const KeyT* __restrict__ col, int64_t cnt,
                                               uint64_t bound, int key_type, int flags,
                                               uint32_t* __restrict__ err) {
  constexpr int E = kRekeyGroup;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t groups = cnt / E;
  const KeyForm form = key_form(key_type, flags);
  bool bad = false;
  for (int64_t g = tid; g < groups; g += stride) bad |= rekey_records<KeyT, By, E>(A + g * E, col, bound, form);
  if constexpr (E > 1) {
    const int64_t i = groups * E + tid;  // the tail: fewer than E records
    if (i < cnt) bad |= rekey_records<KeyT, By, 1>(A + i, col, bound, form);
  }
  if constexpr (By == RekeyBy::kColumn) {
    // One plain store per wave that met a bad value (every lane gets here).
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) *err = 1u;
  }
}

int grid_for(int64_t work, int block, int cap) {
  const int64_t g = (work + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename KeyT, int ValBytes>
void load_columns_form(Elem* A, int64_t cnt, const void* keys, int key_type, const void* vals, uint64_t val0,
                       int flags, hipStream_t s) {
  const KeyT* k = static_cast<const KeyT*>(keys);
  if (aligned16(keys) && aligned16(vals)) {
    const int64_t groups = cnt / column_group<KeyT, ValBytes, true>();  // the tail: threads 0..2 of block 0
    hipLaunchKernelGGL((k_load_columns<KeyT, ValBytes, true>), dim3(grid_for(groups, 256, 8192)), dim3(256), 0, s,
                       A, k, vals, cnt, val0, key_type, flags);
  } else {
    hipLaunchKernelGGL((k_load_columns<KeyT, ValBytes, false>), dim3(grid_for(cnt, 256, 8192)), dim3(256), 0, s, A,
                       k, vals, cnt, val0, key_type, flags);
  }
}

template <typename KeyT, int ValBytes>
void store_columns_form(const Elem* A, int64_t cnt, void* keys, int key_type, void* vals, int flags,
                        hipStream_t s) {
  KeyT* k = static_cast<KeyT*>(keys);
  if (aligned16(keys) && aligned16(vals)) {
    const int64_t groups = cnt / column_group<KeyT, ValBytes, true>();
    hipLaunchKernelGGL((k_store_columns<KeyT, ValBytes, true>), dim3(grid_for(groups, 256, 8192)), dim3(256), 0, s,
                       A, k, vals, cnt, key_type, flags);
  } else {
    hipLaunchKernelGGL((k_store_columns<KeyT, ValBytes, false>), dim3(grid_for(cnt, 256, 8192)), dim3(256), 0, s, A,
                       k, vals, cnt, key_type, flags);
  }
}

}  // namespace

hipError_t launch_load_columns(Elem* A, int64_t cnt, const void* keys, int key_type, const void* vals,
                               int val_bytes, uint64_t val0, int flags, hipStream_t s) {
  if (!key_form_valid(key_type, flags) || !keys || (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) ||
      (val_bytes == 0) != (vals == nullptr))
    return hipErrorInvalidValue;
  if (cnt <= 0) return hipSuccess;
  const bool k32 = key_bytes(key_type) == 4;
  if (val_bytes == 8) {
    if (k32) load_columns_form<uint32_t, 8>(A, cnt, keys, key_type, vals, val0, flags, s);
    else load_columns_form<uint64_t, 8>(A, cnt, keys, key_type, vals, val0, flags, s);
  } else if (val_bytes == 4) {
    if (k32) load_columns_form<uint32_t, 4>(A, cnt, keys, key_type, vals, val0, flags, s);
    else load_columns_form<uint64_t, 4>(A, cnt, keys, key_type, vals, val0, flags, s);
  } else {
    if (k32) load_columns_form<uint32_t, 0>(A, cnt, keys, key_type, vals, val0, flags, s);
    else load_columns_form<uint64_t, 0>(A, cnt, keys, key_type, vals, val0, flags, s);
  }
  return hipGetLastError();
}

hipError_t launch_store_columns(const Elem* A, int64_t cnt, void* keys, int key_type, void* vals, int val_bytes,
                                int flags, hipStream_t s) {
  if (!key_form_valid(key_type, flags) || (!keys && !vals) || (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) ||
      (val_bytes == 0) != (vals == nullptr))
    return hipErrorInvalidValue;
  if (cnt <= 0) return hipSuccess;
  const bool k32 = key_bytes(key_type) == 4;
  if (val_bytes == 8) {
    if (k32) store_columns_form<uint32_t, 8>(A, cnt, keys, key_type, vals, flags, s);
    else store_columns_form<uint64_t, 8>(A, cnt, keys, key_type, vals, flags, s);
  } else if (val_bytes == 4) {
    if (k32) store_columns_form<uint32_t, 4>(A, cnt, keys, key_type, vals, flags, s);
    else store_columns_form<uint64_t, 4>(A, cnt, keys, key_type, vals, flags, s);
  } else {
    if (k32) store_columns_form<uint32_t, 0>(A, cnt, keys, key_type, vals, flags, s);
    else store_columns_form<uint64_t, 0>(A, cnt, keys, key_type, vals, flags, s);
  }
  return hipGetLastError();
}

hipError_t launch_rekey_columns(Elem* A, int64_t cnt, const void* keys, int64_t n_col, int key_type, int flags,
                                uint32_t* err, hipStream_t s) {
  if (!key_form_valid(key_type, flags) || !keys || n_col <= 0 || !err) return hipErrorInvalidValue;
  if (cnt <= 0) return hipSuccess;
  const dim3 grid(grid_for(cnt / kRekeyGroup, 256, 8192));  // the tail: threads of block 0
  if (key_bytes(key_type) == 4)
    hipLaunchKernelGGL((k_rekey<uint32_t, RekeyBy::kColumn>), grid, dim3(256), 0, s, A,
                       static_cast<const uint32_t*>(keys), cnt, (uint64_t)n_col, key_type, flags, err);
  else
    hipLaunchKernelGGL((k_rekey<uint64_t, RekeyBy::kColumn>), grid, dim3(256), 0, s, A,
                       static_cast<const uint64_t*>(keys), cnt, (uint64_t)n_col, key_type, flags, err);
  return hipGetLastError();
}

hipError_t launch_rekey_index(Elem* A, int64_t cnt, uint64_t divisor, hipStream_t s) {
  if (divisor == 0) return hipErrorInvalidValue;
  if (cnt <= 0) return hipSuccess;
  const dim3 grid(grid_for(cnt / kRekeyGroup, 256, 8192));  // the tail: threads of block 0
  hipLaunchKernelGGL((k_rekey<uint64_t, RekeyBy::kIndex>), grid, dim3(256), 0, s, A,
                     static_cast<const uint64_t*>(nullptr), cnt, divisor, kKeyU64, 0, static_cast<uint32_t*>(nullptr));
  return hipGetLastError();
}

}  // namespace lsb
