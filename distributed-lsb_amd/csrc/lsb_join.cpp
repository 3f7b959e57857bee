// The matches of a column of queries in a rank's sorted records (include/lsb.h,
// DESIGN.md §7.8): the first match's value per query (lsb_lookup), and the
// matched pairs in two calls, the rank's join plan (lsb_join_count: lower
// bounds, counts and their prefix sums in the rank's own scratch) and its
// expansion (lsb_store_join).  The searching is lsb_search's: one fence table
// per rank (ensure_search_fence), the same bounded probes.
#include "lsb_keyform.h"
#include "lsb_rt.h"

using namespace lsb_rt;

namespace {

// One given column of a call: where it starts and the bytes it covers.
struct Span {
  const void* p;
  size_t bytes;
};

// Two ranges inside their allocations share a byte (their ends do not wrap).
bool overlap(const Span& a, const Span& b) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// The pointer checks of lsb_load_columns on every given column (elem bytes per
// element, cnt elements each), then no two of them share a byte.
int check_columns(const Rank& r, const Span* cols, const size_t* elem, int n, int64_t cnt, const char* where) {
  for (int i = 0; i < n; ++i)
    if (cols[i].p) LSB_TRY(check_column(r, cols[i].p, elem[i], cnt, where));
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (cols[i].p && cols[j].p && overlap(cols[i], cols[j])) return fail(LSB_ERR_INVALID, where, "two columns overlap");
  return LSB_OK;
}

bool val_bytes_ok(int val_bytes) { return val_bytes == 0 || val_bytes == 4 || val_bytes == 8; }

void drop_plan_scratch(Rank& r) {
  (void)hipFree(r.join_lower);
  (void)hipFree(r.join_off);
  (void)hipFree(r.join_tile);
  r.join_lower = r.join_off = r.join_tile = nullptr;
  r.join_cap = 0;
}

// Room for a plan of m queries: what is there when it is enough, else all
// three anew.  A failed allocation leaves none.
int ensure_plan_scratch(Rank& r, int64_t m) {
  if (m <= r.join_cap) return LSB_OK;
  drop_plan_scratch(r);
  int code = dev_alloc(&r.join_lower, (size_t)m);
  if (code == LSB_OK) code = dev_alloc(&r.join_off, (size_t)m);
  if (code == LSB_OK) code = dev_alloc(&r.join_tile, (size_t)lsb::join_qtiles(m) + 1);
  if (code != LSB_OK) {
    drop_plan_scratch(r);
    return code;
  }
  r.join_cap = m;
  return LSB_OK;
}

}  // namespace

extern "C" {

int lsb_lookup(lsb_ctx_t* c, int rank, int64_t m, const void* queries_dev, int key_type, int flags, void* vals_dev,
               int val_bytes, uint8_t* found_dev) {
  const char* where = "lsb_lookup";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || m < 0) return fail(LSB_ERR_INVALID, where, "rank or m");
  if (!lsb::key_form_valid(key_type, flags)) return fail(LSB_ERR_INVALID, where, "key type or flags");
  if (!val_bytes_ok(val_bytes)) return fail(LSB_ERR_INVALID, where, "val_bytes");
  if ((val_bytes == 0) != (vals_dev == nullptr)) return fail(LSB_ERR_INVALID, where, "val_bytes and values disagree");
  if (!vals_dev && !found_dev) return fail(LSB_ERR_INVALID, where, "no output column");
  if (m == 0) return LSB_OK;
  if (!queries_dev) return fail(LSB_ERR_INVALID, where, "null column");
  const size_t kb = (size_t)lsb::key_bytes(key_type);
  HIP_TRY(hipSetDevice(r->dev));
  const Span cols[3] = {{queries_dev, (size_t)m * kb},
                        {vals_dev, (size_t)m * (size_t)val_bytes},
                        {found_dev, (size_t)m}};
  const size_t elem[3] = {kb, (size_t)(val_bytes ? val_bytes : 1), 1};
  LSB_TRY(check_columns(*r, cols, elem, 3, m, where));
  if (c->broken)
    return fail(LSB_ERR_STATE, where, "an earlier sort failed and left packed records in A; load the input again");
  HIP_TRY(hipStreamSynchronize(r->stream));
  if (r->here > 0) {  // no record, no match: nothing is touched
    LSB_TRY(ensure_search_fence(c, *r));
    HIP_TRY(lsb::launch_lookup(r->A, r->here, r->search_fence, queries_dev, m, key_type, flags, vals_dev, val_bytes,
                               found_dev, r->stream));
  }
  HIP_TRY(hipStreamSynchronize(r->stream));
  return LSB_OK;
}

int lsb_join_count(lsb_ctx_t* c, int rank, int64_t m, const void* queries_dev, int key_type, int flags,
                   int64_t* counts_dev, int64_t* total) {
  const char* where = "lsb_join_count";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || m < 0) return fail(LSB_ERR_INVALID, where, "rank or m");
  if (!lsb::key_form_valid(key_type, flags)) return fail(LSB_ERR_INVALID, where, "key type or flags");
  if (m > 0) {
    if (!queries_dev) return fail(LSB_ERR_INVALID, where, "null column");
    const size_t kb = (size_t)lsb::key_bytes(key_type);
    HIP_TRY(hipSetDevice(r->dev));
    const Span cols[2] = {{queries_dev, (size_t)m * kb}, {counts_dev, (size_t)m * sizeof(int64_t)}};
    const size_t elem[2] = {kb, sizeof(int64_t)};
    LSB_TRY(check_columns(*r, cols, elem, 2, m, where));
  }
  if (c->broken)
    return fail(LSB_ERR_STATE, where, "an earlier sort failed and left packed records in A; load the input again");
  c->join_valid &= ~(1ull << rank);  // this rank's plan is replaced, or gone when the call fails
  r->join_m = m;
  r->join_total = 0;
  if (m > 0 && r->here > 0) {
    HIP_TRY(hipStreamSynchronize(r->stream));
    LSB_TRY(ensure_plan_scratch(*r, m));
    LSB_TRY(ensure_search_fence(c, *r));
    HIP_TRY(lsb::launch_join_count(r->A, r->here, r->search_fence, queries_dev, m, key_type, flags, r->join_lower,
                                   r->join_off, counts_dev, r->join_tile, r->stream));
    int64_t sum = -1;
    HIP_TRY(hipMemcpyAsync(&sum, r->join_tile + lsb::join_qtiles(m), sizeof sum, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    // No query has more matches than the rank has records.
    if (sum < 0 || (uint64_t)sum > (uint64_t)m * (uint64_t)r->here)
      return fail(LSB_ERR_STATE, where, "the device's counts are inconsistent");
    r->join_total = sum;
  } else if (m > 0 && counts_dev) {  // a rank without records: every count is 0
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)m * sizeof(int64_t), r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
  }
  c->join_valid |= 1ull << rank;
  if (total) *total = r->join_total;
  return LSB_OK;
}

int lsb_store_join(lsb_ctx_t* c, int rank, int64_t cap, int64_t query_base, int64_t* left_dev, void* right_dev,
                   int val_bytes, int64_t* pos_dev, int64_t* count) {
  const char* where = "lsb_store_join";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || cap < 0) return fail(LSB_ERR_INVALID, where, "rank or cap");
  if (!val_bytes_ok(val_bytes)) return fail(LSB_ERR_INVALID, where, "val_bytes");
  if ((val_bytes == 0) != (right_dev == nullptr)) return fail(LSB_ERR_INVALID, where, "val_bytes and values disagree");
  if (!left_dev && !right_dev && !pos_dev) return fail(LSB_ERR_INVALID, where, "no output column");
  if (c->broken)
    return fail(LSB_ERR_STATE, where, "an earlier sort failed and left packed records in A; load the input again");
  if (!((c->join_valid >> rank) & 1))
    return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_join_count after the last change of A");
  const int64_t mine = r->join_total;
  if (count) *count = mine;
  if (cap < mine) return fail(LSB_ERR_INVALID, where, "cap below the rank's pairs");
  if (mine == 0) return LSB_OK;  // nothing to write: the pointers are not looked at
  HIP_TRY(hipSetDevice(r->dev));
  const Span cols[3] = {{left_dev, (size_t)cap * sizeof(int64_t)},
                        {right_dev, (size_t)cap * (size_t)val_bytes},
                        {pos_dev, (size_t)cap * sizeof(int64_t)}};
  const size_t elem[3] = {sizeof(int64_t), (size_t)(val_bytes ? val_bytes : 1), sizeof(int64_t)};
  LSB_TRY(check_columns(*r, cols, elem, 3, cap, where));
  HIP_TRY(hipStreamSynchronize(r->stream));
  HIP_TRY(lsb::launch_join_expand(r->A, r->here, r->join_lower, r->join_off, r->join_m, mine, query_base,
                                  (int64_t)rank * c->per, left_dev, right_dev, val_bytes, pos_dev, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  return LSB_OK;
}

}  // extern "C"
