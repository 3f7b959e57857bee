// Key forms of caller-owned columns (lsb_load_columns / lsb_store_columns,
// include/lsb.h): the order-preserving map between a typed key's raw bits and
// the unsigned 64-bit key the passes sort by.  Pure integer functions, host
// and device, no device header: the column kernels (lsb_columns.hip), the ABI's
// lsb_key_encode / lsb_key_decode and host tools share this one definition.
//
//   u64 / u32   identity
//   i64 / i32   flip the sign bit
//   f64 / f32   sign set: ~bits; else flip the sign bit
// 32-bit types at 32 bits, zero-extended.  kOrderDescending complements the
// encoded key within the key's width, so a 32-bit key keeps a zero upper word
// (its four upper digits stay constant and the sort skips them), and the
// ascending stable sort of the complement keeps equal keys in input order.
// Float order, ascending: NaNs with the sign set, -inf, finite values
// (-0.0 before +0.0), +inf, NaNs with the sign clear.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSB_KEYFORM_HD __host__ __device__
#else
#define LSB_KEYFORM_HD
#endif

namespace lsb {

// == LSB_KEY_* and LSB_ORDER_DESCENDING (include/lsb.h).
constexpr int kKeyU64 = 0, kKeyI64 = 1, kKeyF64 = 2, kKeyU32 = 3, kKeyI32 = 4, kKeyF32 = 5;
constexpr int kKeyTypes = 6;
constexpr int kOrderDescending = 1;
constexpr int kKeyFlagMask = kOrderDescending;

LSB_KEYFORM_HD inline bool key_form_valid(int key_type, int flags) {
  return key_type >= 0 && key_type < kKeyTypes && (flags & ~kKeyFlagMask) == 0;
}
LSB_KEYFORM_HD inline int key_bytes(int key_type) { return key_type >= kKeyU32 ? 4 : 8; }

// A key form as masks, so that both maps are branch-free (the kernels build
// one per thread, outside their loops): with t = the key cut to its width and
// spread(t) = all ones when t's top bit (at that width) is set,
//   encode(bits) = t ^ enc ^ (spread(t) & fmask),      t = bits & mask
//   decode(key)  = t ^ dec ^ (spread(t) & fmask),      t = (key & mask) ^ desc
// enc = the sign bit for signed and float types, complemented within the width
// when descending; fmask = every bit but the sign for float types (a set sign
// turns "flip the sign" into "flip every bit"), else 0; desc = mask when
// descending; dec = the sign bit for signed types, mask for float types (an
// encoded float with its top bit set had its sign clear).
struct KeyForm {
  uint64_t mask, fmask, enc, desc, dec;
  int shl;  // 64 - the key's width: spread(t) = (int64_t)(t << shl) >> 63
};

LSB_KEYFORM_HD inline KeyForm key_form(int key_type, int flags) {
  const bool k32 = key_type >= kKeyU32;
  const bool is_int = key_type == kKeyI64 || key_type == kKeyI32;
  const bool is_float = key_type == kKeyF64 || key_type == kKeyF32;
  const uint64_t mask = k32 ? 0xffffffffull : ~0ull;
  const uint64_t sign = k32 ? 0x80000000ull : 0x8000000000000000ull;
  KeyForm f;
  f.mask = mask;
  f.fmask = is_float ? mask ^ sign : 0;
  f.desc = (flags & kOrderDescending) ? mask : 0;
  f.enc = ((is_int || is_float) ? sign : 0) ^ f.desc;
  f.dec = is_int ? sign : is_float ? mask : 0;
  f.shl = k32 ? 32 : 0;
  return f;
}

LSB_KEYFORM_HD inline uint64_t encode(uint64_t bits, const KeyForm& f) {
  const uint64_t t = bits & f.mask;
  return t ^ f.enc ^ ((uint64_t)((int64_t)(t << f.shl) >> 63) & f.fmask);
}

LSB_KEYFORM_HD inline uint64_t decode(uint64_t key, const KeyForm& f) {
  const uint64_t t = (key & f.mask) ^ f.desc;
  return t ^ f.dec ^ ((uint64_t)((int64_t)(t << f.shl) >> 63) & f.fmask);
}

// bits of a 32-bit type: the key in the low word (the upper word is ignored).
// 0 on an unknown type or flag.
LSB_KEYFORM_HD inline uint64_t encode(uint64_t bits, int key_type, int flags) {
  return key_form_valid(key_type, flags) ? encode(bits, key_form(key_type, flags)) : 0;
}

LSB_KEYFORM_HD inline uint64_t decode(uint64_t key, int key_type, int flags) {
  return key_form_valid(key_type, flags) ? decode(key, key_form(key_type, flags)) : 0;
}

}  // namespace lsb
