// The k-th key and the first k + 1 records of the stable sort without a sort
// (include/lsb.h): the host planner over the ranks' counts,
// the collective MSD radix select (one histogram round per varying key byte,
// from the top) and the local store of a rank's part of the selection.
#include "lsb_keyform.h"
#include "lsb_rt.h"

using namespace lsb_rt;

namespace {

using lsb::kSelHist;
using lsb::kSelWords;

// Each buffer once: a call that failed part-way leaves what it got to the next.
int ensure_select_scratch(const lsb_ctx* c, Rank& r) {
  if (!r.sel_buf) LSB_TRY(dev_alloc(&r.sel_buf, (size_t)lsb::kSelBufWords));
  if (!r.sel_gather && c->mode != Mode::kLoopback) LSB_TRY(dev_alloc(&r.sel_gather, (size_t)kSelWords * c->P));
  return LSB_OK;
}

// The store's tile tables on top (lsb_store_select), freed with the rest.
int ensure_store_scratch(Rank& r) {
  const size_t tiles = (size_t)lsb::run_tiles(r.here);
  if (!r.sel_cnt) LSB_TRY(dev_alloc(&r.sel_cnt, tiles));
  if (!r.sel_tbase) LSB_TRY(dev_alloc(&r.sel_tbase, 2 * tiles));
  return LSB_OK;
}

// Every rank's table of the round on the host, through the select's own
// gather area (r.gather may be smaller).  Ranks that launched nothing
// (ran[r] == 0) give zeros.
int gather_tables(lsb_ctx* c, const std::vector<char>& ran, std::vector<uint64_t>& tab) {
  return gather_words(c, kSelWords, c->ranks[0].sel_gather,
                      [&](const Rank& r) { return ran[r.rank] ? r.sel_buf : nullptr; }, tab);
}

// Where a rank's candidates are read from in the next round.
struct Source {
  const Elem* at = nullptr;
  int64_t used = 0;  // records of B the compactions have taken so far
};

// The rounds of lsb_select.  On return: the pivot, every rank's keys below and
// equal to it, and what ran.
int select_rounds(lsb_ctx* c, int64_t k, uint64_t* pivot, std::vector<int64_t>& below, std::vector<int64_t>& equal) {
  const char* where = "lsb_select";
  const int P = c->P;
  // What every rank knows of every rank: the records its current source holds
  // and how many of them are still candidates.  The host logic is the same on
  // every rank of a one-rank-per-process world, so all decide alike.
  std::vector<int64_t> held((size_t)P), cand((size_t)P);
  for (int r = 0; r < P; ++r) held[r] = cand[r] = here_of(c->n, P, r);
  std::vector<Source> src(c->ranks.size());
  for (size_t i = 0; i < c->ranks.size(); ++i) {
    src[i].at = c->ranks[i].A;
    HIP_TRY(hipSetDevice(c->ranks[i].dev));
    LSB_TRY(ensure_select_scratch(c, c->ranks[i]));
  }
  below.assign((size_t)P, 0);
  uint64_t prefix = 0, mask = 0, kor = 0, knor = 0;
  int64_t remaining = k;  // the wanted record's rank among the candidates
  std::vector<uint64_t> tab;
  std::vector<char> ran((size_t)P), packed((size_t)P);
  for (int shift = 56; shift >= 0;) {
    const bool first = c->sel_rounds == 0;
    // A rank compacts when at most half of what its source holds is still a
    // candidate: the ranges appended to B then sum to less than `here`.
    for (int r = 0; r < P; ++r) {
      ran[r] = cand[r] > 0;
      packed[r] = !first && cand[r] > 0 && cand[r] * 2 <= held[r];
    }
    for (size_t i = 0; i < c->ranks.size(); ++i) {
      Rank& r = c->ranks[i];
      if (!ran[r.rank]) continue;
      HIP_TRY(hipSetDevice(r.dev));
      HIP_TRY(hipMemsetAsync(r.sel_buf, 0, sizeof(uint64_t) * kSelWords, r.stream));
      Elem* dst = nullptr;
      if (packed[r.rank]) {
        if (src[i].used + cand[r.rank] > r.here) return fail(LSB_ERR_STATE, where, "the candidates outgrow B");
        dst = r.B + src[i].used;
      }
      HIP_TRY(lsb::launch_select_hist(src[i].at, held[r.rank], shift, prefix, mask, first, dst, cand[r.rank],
                                      r.sel_buf, r.stream));
      c->sel_read += held[r.rank];
      if (dst) {
        src[i].at = dst;
        src[i].used += cand[r.rank];
      }
    }
    LSB_TRY(gather_tables(c, ran, tab));
    c->sel_rounds += 1;
    // The words come from the device (and from other ranks): check them before
    // anything is derived from them.
    int64_t total[kSelHist] = {};
    for (int r = 0; r < P; ++r) {
      const uint64_t* w = &tab[(size_t)r * kSelWords];
      uint64_t sum = 0;
      for (int b = 0; b < kSelHist; ++b) {
        if (w[b] > (uint64_t)cand[r]) return fail(LSB_ERR_STATE, where, "a count above the rank's candidates");
        sum += w[b];
        total[b] += (int64_t)w[b];
      }
      if (sum != (uint64_t)cand[r]) return fail(LSB_ERR_STATE, where, "A changed during the select: the counts do not add up");
      if (packed[r] && (w[kSelHist] != (uint64_t)cand[r] || w[kSelHist + 1] != 0))
        return fail(LSB_ERR_STATE, where, "A changed during the select: the candidates are not those counted");
      if (packed[r]) held[r] = cand[r];
      if (first) {
        kor |= w[kSelHist];
        knor |= w[kSelHist + 1];
      }
    }
    int b = 0;
    int64_t before = 0;
    while (b < kSelHist - 1 && before + total[b] <= remaining) before += total[b++];
    if (before + total[b] <= remaining) return fail(LSB_ERR_STATE, where, "fewer candidates than the wanted rank");
    remaining -= before;
    for (int r = 0; r < P; ++r) {
      const uint64_t* w = &tab[(size_t)r * kSelWords];
      for (int j = 0; j < b; ++j) below[r] += (int64_t)w[j];
      cand[r] = (int64_t)w[b];
    }
    prefix |= (uint64_t)b << shift;
    mask |= 0xffull << shift;
    // A byte on which every key of the array agrees takes its bits from the span.
    const uint64_t varying = kor & knor;
    for (shift -= 8; shift >= 0 && ((varying >> shift) & 0xff) == 0; shift -= 8) {
      prefix |= kor & (0xffull << shift);
      mask |= 0xffull << shift;
    }
  }
  *pivot = prefix;
  equal = cand;
  return LSB_OK;
}

}  // namespace

extern "C" {

int lsb_plan_select(int64_t n_total, int num_ranks, int64_t count, const int64_t* below, const int64_t* equal,
                    int64_t* take, int64_t* bases) {
  const char* where = "lsb_plan_select";
  if (n_total < 0 || num_ranks < 1 || num_ranks > LSB_MAX_RANKS || !below || !equal || !take || !bases)
    return fail(LSB_ERR_INVALID, where, "arguments");
  const int P = num_ranks;
  int64_t sum_below = 0, sum_equal = 0;
  for (int r = 0; r < P; ++r) {
    const int64_t here = here_of(n_total, P, r);
    if (below[r] < 0 || equal[r] < 0) return fail(LSB_ERR_INVALID, where, "negative count");
    if (below[r] > here || equal[r] > here - below[r]) return fail(LSB_ERR_INVALID, where, "more keys than the rank holds");
    sum_below += below[r];
    sum_equal += equal[r];
  }
  if (!(sum_below < count && count <= sum_below + sum_equal))
    return fail(LSB_ERR_INVALID, where, "the counts do not bracket count");
  int64_t left = count - sum_below, acc = 0;  // equal keys still to take, in rank order
  for (int r = 0; r < P; ++r) {
    const int64_t e = equal[r] < left ? equal[r] : left;
    left -= e;
    take[r] = below[r] + e;
    bases[r] = acc;
    acc += take[r];
  }
  return LSB_OK;
}

int lsb_select(lsb_ctx_t* c, int64_t k, uint64_t* key, int64_t* below, int64_t* equal, int64_t* take,
               int64_t* bases) {
  const char* where = "lsb_select";
  LSB_TRY(check_ctx(c));
  if (k < 0 || k >= c->n) return fail(LSB_ERR_INVALID, where, "k outside [0, n)");
  if (c->broken)
    return fail(LSB_ERR_STATE, where, "an earlier sort failed and left packed records in A; load the input again");
  select_invalidate(c);
  c->sel_rounds = 0;
  c->sel_read = 0;
  const int P = c->P;
  LSB_TRY(select_rounds(c, k, &c->sel_pivot, c->sel_below, c->sel_equal));
  c->sel_take.assign((size_t)P, 0);
  c->sel_base.assign((size_t)P, 0);
  if (lsb_plan_select(c->n, P, k + 1, c->sel_below.data(), c->sel_equal.data(), c->sel_take.data(),
                      c->sel_base.data()) != LSB_OK)
    return fail(LSB_ERR_STATE, where, "the device's counts are inconsistent");
  c->select_valid = true;
  int64_t sum_below = 0, sum_equal = 0;
  for (int r = 0; r < P; ++r) {
    sum_below += c->sel_below[r];
    sum_equal += c->sel_equal[r];
    if (take) take[r] = c->sel_take[r];
    if (bases) bases[r] = c->sel_base[r];
  }
  if (key) *key = c->sel_pivot;
  if (below) *below = sum_below;
  if (equal) *equal = sum_equal;
  return LSB_OK;
}

int lsb_store_select(lsb_ctx_t* c, int rank, int64_t cap, void* keys_dev, int key_type, int flags, void* vals_dev,
                     int val_bytes, int64_t* count) {
  const char* where = "lsb_store_select";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || cap < 0) return fail(LSB_ERR_INVALID, where, "rank or cap");
  if (!lsb::key_form_valid(key_type, flags)) return fail(LSB_ERR_INVALID, where, "key type or flags");
  if (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) return fail(LSB_ERR_INVALID, where, "val_bytes");
  if ((val_bytes == 0) != (vals_dev == nullptr)) return fail(LSB_ERR_INVALID, where, "val_bytes and values disagree");
  if (!keys_dev && !vals_dev) return fail(LSB_ERR_INVALID, where, "no output column");
  if (!c->select_valid) return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_select after the last change of A");
  const int64_t mine = c->sel_take[rank];
  if (count) *count = mine;
  if (cap < mine) return fail(LSB_ERR_INVALID, where, "cap below the rank's part of the selection");
  if (mine == 0) return LSB_OK;  // nothing to write: the pointers are not looked at
  HIP_TRY(hipSetDevice(r->dev));
  if (keys_dev) LSB_TRY(check_column(*r, keys_dev, (size_t)lsb::key_bytes(key_type), cap, where));
  if (vals_dev) LSB_TRY(check_column(*r, vals_dev, (size_t)val_bytes, cap, where));
  LSB_TRY(ensure_store_scratch(*r));
  HIP_TRY(hipStreamSynchronize(r->stream));
  uint32_t* err = reinterpret_cast<uint32_t*>(r->sel_buf + kSelWords);
  const int64_t lt = c->sel_below[rank];
  uint32_t h = 0;
  LSB_TRY(guarded_launch(*r, err, &h, [&]() -> int {
    HIP_TRY(lsb::launch_select_count(r->A, r->here, c->sel_pivot, lt, c->sel_equal[rank], r->sel_cnt, r->sel_tbase,
                                     err, r->stream));
    HIP_TRY(lsb::launch_select_write(r->A, r->here, c->sel_pivot, mine - lt, mine, r->sel_cnt, r->sel_tbase, keys_dev,
                                     key_type, flags, vals_dev, val_bytes, err, r->stream));
    return LSB_OK;
  }));
  if (h) {
    select_invalidate(c);
    return fail(LSB_ERR_STATE, where, "A changed since lsb_select: the outputs are unspecified");
  }
  return LSB_OK;
}

int lsb_get_last_select(lsb_ctx_t* c, int* rounds, int64_t* records_read) {
  LSB_TRY(check_ctx(c));
  if (rounds) *rounds = c->sel_rounds;
  if (records_read) *records_read = c->sel_read;
  return LSB_OK;
}

}  // extern "C"
