// A column of queries against a rank's sorted records (include/lsb.h,
// DESIGN.md §7.7): the argument checks, the rank's fence table (built at the
// first search after a change of A, for lsb_lookup and lsb_join_count too) and
// the one launch of lsb_search.
#include "lsb_keyform.h"
#include "lsb_rt.h"

using namespace lsb_rt;

namespace lsb_rt {

int ensure_search_fence(lsb_ctx* c, Rank& r) {
  if (!r.search_fence) LSB_TRY(dev_alloc(&r.search_fence, (size_t)lsb::run_tiles(r.here)));
  if (!((c->search_valid >> r.rank) & 1)) {
    HIP_TRY(lsb::launch_search_fence(r.A, r.here, r.search_fence, r.stream));
    c->search_valid |= 1ull << r.rank;
  }
  return LSB_OK;
}

}  // namespace lsb_rt

extern "C" {

int lsb_search(lsb_ctx_t* c, int rank, int64_t m, const void* queries_dev, int key_type, int flags, int mode,
               int64_t* out_dev) {
  const char* where = "lsb_search";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || m < 0) return fail(LSB_ERR_INVALID, where, "rank or m");
  if (!lsb::key_form_valid(key_type, flags)) return fail(LSB_ERR_INVALID, where, "key type or flags");
  if (!lsb::search_mode_valid(mode)) return fail(LSB_ERR_INVALID, where, "mode");
  if (m == 0) return LSB_OK;
  if (!queries_dev || !out_dev) return fail(LSB_ERR_INVALID, where, "null column");
  const size_t kb = (size_t)lsb::key_bytes(key_type);
  HIP_TRY(hipSetDevice(r->dev));
  LSB_TRY(check_column(*r, queries_dev, kb, m, where));
  LSB_TRY(check_column(*r, out_dev, sizeof(int64_t), m, where));
  // Both ranges lie inside their allocations, so their ends do not wrap.
  const uintptr_t q0 = reinterpret_cast<uintptr_t>(queries_dev), o0 = reinterpret_cast<uintptr_t>(out_dev);
  if (q0 < o0 + (uintptr_t)m * sizeof(int64_t) && o0 < q0 + (uintptr_t)m * kb)
    return fail(LSB_ERR_INVALID, where, "queries and out overlap");
  if (c->broken)
    return fail(LSB_ERR_STATE, where, "an earlier sort failed and left packed records in A; load the input again");
  HIP_TRY(hipStreamSynchronize(r->stream));
  const bool add = (mode & lsb::kSearchAdd) != 0;
  if (r->here == 0) {  // no record counts: zeros, or nothing to add
    if (!add) HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)m * sizeof(int64_t), r->stream));
  } else {
    LSB_TRY(ensure_search_fence(c, *r));
    HIP_TRY(lsb::launch_search(r->A, r->here, r->search_fence, queries_dev, m, key_type, flags, mode, out_dev,
                               r->stream));
  }
  HIP_TRY(hipStreamSynchronize(r->stream));
  return LSB_OK;
}

}  // extern "C"
