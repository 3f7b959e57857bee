// Runs of equal keys (include/lsb.h): the host planner over
// the ranks' summary words, the collective count and the local store; and the
// reductions over the runs' values (§7.3): the host planner over the ranks'
// leading runs, the collective plan and the local store; and the run id of
// every record (§7.4): one local call over the run plan; and the scan within
// the runs (§7.6): the host planner over the ranks' trailing runs, the
// collective plan, the local store and the records form.
#include "lsb_keyform.h"
#include "lsb_rt.h"

using namespace lsb_rt;

namespace {

// The planner's four words of rank s.
enum { kFirst = 0, kLast = 1, kInner = 2, kLead = 3 };

// A summary no array gives is refused before anything is derived from it
// (lsb_plan_runs and lsb_plan_run_tails).
int check_summary(int64_t n_total, int P, const uint64_t* summary, const char* where) {
  for (int r = 0; r < P; ++r) {
    const int64_t here = here_of(n_total, P, r);
    if (here == 0) continue;
    const uint64_t* w = summary + (size_t)r * 4;
    const uint64_t h = (uint64_t)here;
    if (w[kLead] < 1 || w[kLead] > h) return fail(LSB_ERR_INVALID, where, "lead outside [1, here]");
    if (w[kInner] > h - 1) return fail(LSB_ERR_INVALID, where, "more heads than positions");
    if ((w[kInner] == 0) != (w[kLead] == h)) return fail(LSB_ERR_INVALID, where, "heads and leading run disagree");
    if (w[kInner] == 0 && w[kFirst] != w[kLast]) return fail(LSB_ERR_INVALID, where, "one run with two keys");
  }
  return LSB_OK;
}

// Each buffer once: a call that failed part-way leaves what it got to the next.
int ensure_run_scratch(Rank& r) {
  const size_t tiles = (size_t)lsb::run_tiles(r.here);
  if (!r.run_cnt) LSB_TRY(dev_alloc(&r.run_cnt, tiles));
  if (!r.run_tbase) LSB_TRY(dev_alloc(&r.run_tbase, tiles));
  if (!r.run_sum) LSB_TRY(dev_alloc(&r.run_sum, lsb::kRunSumWords));
  return LSB_OK;
}

// The reductions' scratch on top (lsb_plan_reduce), freed with the run scratch.
int ensure_reduce_scratch(Rank& r) {
  if (!r.run_lead) LSB_TRY(dev_alloc(&r.run_lead, (size_t)lsb::run_tiles(r.here)));
  if (!r.run_part) LSB_TRY(dev_alloc(&r.run_part, (size_t)lsb::kRunLeadParts + 1));
  return LSB_OK;
}

// The scan's scratch (lsb_plan_scan), freed with the run scratch: tile_open
// and tile_in, then the rank's trail word and the scan's own error word.
int ensure_scan_scratch(Rank& r) {
  if (!r.scan_buf) LSB_TRY(dev_alloc(&r.scan_buf, 2 * (size_t)lsb::run_tiles(r.here) + 2));
  return LSB_OK;
}
uint64_t* scan_open(const Rank& r) { return r.scan_buf; }
uint64_t* scan_in(const Rank& r) { return r.scan_buf + lsb::run_tiles(r.here); }
uint64_t* scan_trail(const Rank& r) { return r.scan_buf + 2 * lsb::run_tiles(r.here); }
uint32_t* scan_err(const Rank& r) { return reinterpret_cast<uint32_t*>(scan_trail(r) + 1); }

// The run kernels' error word (lsb_store_runs, lsb_store_reduce, lsb_label_runs).
uint32_t* run_err(const Rank& r) { return reinterpret_cast<uint32_t*>(r.run_sum + 4); }

// The OR of the non-empty local ranks' error words, after their streams are done.
template <typename ErrOf>
int read_guards(lsb_ctx* c, ErrOf err_of, uint32_t* any) {
  *any = 0;
  for (Rank& r : c->ranks) {
    if (r.here == 0) continue;
    HIP_TRY(hipSetDevice(r.dev));
    uint32_t h = 0;
    LSB_TRY(read_guard(r, err_of(r), &h));
    *any |= h;
  }
  return LSB_OK;
}

// lsb_label_runs' and lsb_scan_runs' work: every non-empty local rank's A -> B
// by launch_of(rank) on its own stream, then every rank's error word; the
// ranks swap only when none of them found A changed.
template <typename ErrOf, typename LaunchOf>
int ranks_a_to_b(lsb_ctx* c, const char* where, const char* text, ErrOf err_of, LaunchOf launch_of) {
  for (Rank& r : c->ranks) {
    if (r.here == 0) continue;
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(hipMemsetAsync(err_of(r), 0, sizeof(uint64_t), r.stream));
    LSB_TRY(launch_of(r));
  }
  uint32_t any = 0;
  LSB_TRY(read_guards(c, err_of, &any));
  if (any) return fail(LSB_ERR_STATE, where, text);
  for (Rank& r : c->ranks)
    if (r.here > 0) std::swap(r.A, r.B);
  return LSB_OK;
}

// The write kernel of rank r into out, with the plan's carry and the rank's
// first head from the run plan's summary.
hipError_t launch_scan_write(lsb_ctx* c, Rank& r, int sink, void* out) {
  const int head0 = c->run_head0[r.rank];
  const int64_t lead = head0 ? 0 : (int64_t)c->run_words[(size_t)r.rank * 4 + kLead];
  return lsb::launch_run_scan_write(r.A, r.here, (int64_t)r.rank * c->per, head0, lead, r.run_cnt, scan_in(r),
                                    c->scan_op, c->scan_type, c->run_carry[r.rank], sink, out, scan_err(r),
                                    r.stream);
}

int scan_ranks(lsb_ctx* c, int mode) {
  const int sink = mode == LSB_LABEL_KEEP ? lsb::kScanKeep : lsb::kScanByValue;
  return ranks_a_to_b(c, "lsb_scan_runs", "A changed since lsb_count_runs: no rank was written", scan_err,
                      [&](Rank& r) -> int {
                        HIP_TRY(launch_scan_write(c, r, sink, r.B));
                        return LSB_OK;
                      });
}

// Two outputs of cap elements (of ea and eb bytes) share a byte.
bool columns_overlap(const void* a, size_t ea, const void* b, size_t eb, int64_t cap) {
  if (!a || !b) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)cap * eb && pb < pa + (uintptr_t)cap * ea;
}

// The ranks' words of a plan on the host through r.gather (at least 4 P
// words): the four summary words, the leading-run word of the ranks that
// reduced one (sent[r] != 0), the scan's trail word.  Empty ranks give zeros.
int gather_summaries(lsb_ctx* c, std::vector<uint64_t>& sum) {
  return gather_words(c, 4, c->ranks[0].gather, [](const Rank& r) { return r.here > 0 ? r.run_sum : nullptr; }, sum);
}
int gather_leads(lsb_ctx* c, const std::vector<char>& sent, std::vector<uint64_t>& lead) {
  return gather_words(
      c, 1, c->ranks[0].gather,
      [&](const Rank& r) { return sent[r.rank] ? r.run_part + lsb::kRunLeadParts : nullptr; }, lead);
}
int gather_trails(lsb_ctx* c, std::vector<uint64_t>& trail) {
  return gather_words(c, 1, c->ranks[0].gather, [](const Rank& r) { return r.here > 0 ? scan_trail(r) : nullptr; },
                      trail);
}

int label_ranks(lsb_ctx* c, int mode) {
  return ranks_a_to_b(c, "lsb_label_runs", "A changed since lsb_count_runs: no rank was labelled", run_err,
                      [&](Rank& r) -> int {
                        HIP_TRY(lsb::launch_run_label(r.A, r.B, r.here, c->run_base[r.rank], c->run_head0[r.rank],
                                                      r.run_cnt, r.run_tbase, mode, run_err(r), r.stream));
                        return LSB_OK;
                      });
}

}  // namespace

extern "C" {

int lsb_plan_runs(int64_t n_total, int num_ranks, const uint64_t* summary, int* head0, int64_t* runs,
                  int64_t* bases, int64_t* ends, int64_t* total) {
  if (n_total < 0 || num_ranks < 1 || num_ranks > LSB_MAX_RANKS || !summary || !head0 || !runs || !bases || !ends ||
      !total)
    return fail(LSB_ERR_INVALID, "lsb_plan_runs", "arguments");
  const int P = num_ranks;
  const int64_t per = div_ceil(n_total, P);
  LSB_TRY(check_summary(n_total, P, summary, "lsb_plan_runs"));
  int64_t acc = 0;
  int prev = -1;  // the last non-empty rank before r
  for (int r = 0; r < P; ++r) {
    const int64_t here = here_of(n_total, P, r);
    head0[r] = 0;
    runs[r] = 0;
    bases[r] = acc;
    ends[r] = 0;
    if (here == 0) {
      bases[r] = 0;
      continue;
    }
    const uint64_t* w = summary + (size_t)r * 4;
    head0[r] = (prev < 0 || summary[(size_t)prev * 4 + kLast] != w[kFirst]) ? 1 : 0;
    runs[r] = (int64_t)w[kInner] + head0[r];
    acc += runs[r];
    // The rank's last run goes on through the leading runs of the ranks
    // after it for as long as they carry its key, whole ranks included.
    int64_t end = (int64_t)r * per + here;
    for (int s = r + 1; s < P; ++s) {
      const int64_t hs = here_of(n_total, P, s);
      if (hs == 0) continue;
      const uint64_t* v = summary + (size_t)s * 4;
      if (v[kFirst] != w[kLast]) break;
      end += (int64_t)v[kLead];
      if ((int64_t)v[kLead] < hs) break;
    }
    ends[r] = end;
    prev = r;
  }
  *total = acc;
  return LSB_OK;
}

int lsb_count_runs(lsb_ctx_t* c, int64_t* total, int64_t* runs, int64_t* bases) {
  LSB_TRY(check_ctx(c));
  if (!total) return fail(LSB_ERR_INVALID, "lsb_count_runs", "null total");
  if (c->broken)
    return fail(LSB_ERR_STATE, "lsb_count_runs", "an earlier sort failed and left packed records in A; load the input again");
  runs_invalidate(c);
  const int P = c->P;
  std::vector<uint64_t> sum((size_t)P * 4, 0);
  if (c->n > 0) {
    for (Rank& r : c->ranks) {
      if (r.here == 0) continue;
      HIP_TRY(hipSetDevice(r.dev));
      LSB_TRY(ensure_run_scratch(r));
      HIP_TRY(lsb::launch_run_count(r.A, r.here, r.run_cnt, r.run_tbase, r.run_sum, r.stream));
    }
    LSB_TRY(gather_summaries(c, sum));
  }
  c->run_head0.assign(P, 0);
  c->run_count.assign(P, 0);
  c->run_base.assign(P, 0);
  c->run_end.assign(P, 0);
  c->runs_total = 0;
  // The words come from the device (and from other ranks): the planner checks them.
  if (lsb_plan_runs(c->n, P, sum.data(), c->run_head0.data(), c->run_count.data(), c->run_base.data(),
                    c->run_end.data(), &c->runs_total) != LSB_OK)
    return fail(LSB_ERR_STATE, "lsb_count_runs", "the device's run summary is inconsistent");
  c->run_words = sum;  // lsb_plan_reduce walks the same chains
  c->runs_valid = true;
  *total = c->runs_total;
  for (int r = 0; r < P; ++r) {
    if (runs) runs[r] = c->run_count[r];
    if (bases) bases[r] = c->run_base[r];
  }
  return LSB_OK;
}

int lsb_store_runs(lsb_ctx_t* c, int rank, int64_t cap, void* keys_dev, int key_type, int flags,
                   int64_t* starts_dev, int64_t* counts_dev, void* firsts_dev, int val_bytes, int64_t* runs) {
  const char* where = "lsb_store_runs";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || cap < 0) return fail(LSB_ERR_INVALID, where, "rank or cap");
  if (!lsb::key_form_valid(key_type, flags)) return fail(LSB_ERR_INVALID, where, "key type or flags");
  if (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) return fail(LSB_ERR_INVALID, where, "val_bytes");
  if ((val_bytes == 0) != (firsts_dev == nullptr)) return fail(LSB_ERR_INVALID, where, "val_bytes and firsts disagree");
  if (!keys_dev && !starts_dev && !firsts_dev) return fail(LSB_ERR_INVALID, where, "no output");
  if (counts_dev && !starts_dev) return fail(LSB_ERR_INVALID, where, "counts need starts");
  if (!c->runs_valid) return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs after the last change of A");
  const int64_t mine = c->run_count[rank];
  if (runs) *runs = mine;
  if (cap < mine) return fail(LSB_ERR_INVALID, where, "cap below the rank's runs");
  if (mine == 0) return LSB_OK;  // nothing to write: the pointers are not looked at
  HIP_TRY(hipSetDevice(r->dev));
  if (keys_dev) LSB_TRY(check_column(*r, keys_dev, (size_t)lsb::key_bytes(key_type), cap, where));
  if (starts_dev) LSB_TRY(check_column(*r, starts_dev, 8, cap, where));
  if (counts_dev) LSB_TRY(check_column(*r, counts_dev, 8, cap, where));
  if (firsts_dev) LSB_TRY(check_column(*r, firsts_dev, (size_t)val_bytes, cap, where));
  // Every range lies inside an allocation now, so the sums below cannot wrap.
  const void* out[4] = {keys_dev, starts_dev, counts_dev, firsts_dev};
  const size_t elem[4] = {(size_t)lsb::key_bytes(key_type), 8, 8, (size_t)val_bytes};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (columns_overlap(out[i], elem[i], out[j], elem[j], cap))
        return fail(LSB_ERR_INVALID, where, "outputs overlap");
  HIP_TRY(hipStreamSynchronize(r->stream));
  uint32_t h = 0;
  LSB_TRY(guarded_launch(*r, run_err(*r), &h, [&]() -> int {
    HIP_TRY(lsb::launch_run_write(r->A, r->here, (int64_t)r->rank * c->per, c->run_head0[rank], r->run_cnt,
                                  r->run_tbase, keys_dev, key_type, flags, starts_dev, counts_dev, firsts_dev,
                                  val_bytes, mine, c->run_end[rank], run_err(*r), r->stream));
    return LSB_OK;
  }));
  if (h) {
    runs_invalidate(c);
    return fail(LSB_ERR_STATE, where, "A changed since lsb_count_runs: the outputs are unspecified");
  }
  return LSB_OK;
}

int lsb_label_runs(lsb_ctx_t* c, int mode) {
  const char* where = "lsb_label_runs";
  LSB_TRY(check_ctx(c));
  if (mode != LSB_LABEL_KEEP && mode != LSB_LABEL_BY_VALUE) return fail(LSB_ERR_INVALID, where, "mode");
  if (!c->runs_valid) return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs after the last change of A");
  // The records change (or a rank found them changed already): the plans end here either way.
  const int rc = c->n > 0 ? label_ranks(c, mode) : LSB_OK;
  runs_invalidate(c);
  select_invalidate(c);
  search_invalidate(c);
  return rc;
}

int lsb_plan_run_tails(int64_t n_total, int num_ranks, const uint64_t* summary, int op, int val_type,
                       const uint64_t* lead, uint64_t* tail) {
  const char* where = "lsb_plan_run_tails";
  if (n_total < 0 || num_ranks < 1 || num_ranks > LSB_MAX_RANKS || !summary || !lead || !tail ||
      !lsb::reduce_valid(op, val_type))
    return fail(LSB_ERR_INVALID, where, "arguments");
  const int P = num_ranks;
  LSB_TRY(check_summary(n_total, P, summary, where));
  const int F = lsb::red_form(op, val_type);
  const lsb::KeyForm form = lsb::key_form(val_type, 0);
  for (int r = 0; r < P; ++r) {
    uint64_t acc = lsb::red_identity(F);
    if (here_of(n_total, P, r) > 0) {
      // lsb_plan_runs' walk for ends[r]: the leading runs of the ranks after r
      // for as long as they carry its last key, whole ranks included.
      const uint64_t* w = summary + (size_t)r * 4;
      for (int s = r + 1; s < P; ++s) {
        const int64_t hs = here_of(n_total, P, s);
        if (hs == 0) continue;
        const uint64_t* v = summary + (size_t)s * 4;
        if (v[kFirst] != w[kLast]) break;
        acc = lsb::red(F, acc, lsb::red_load(F, lead[s], form));
        if ((int64_t)v[kLead] < hs) break;
      }
    }
    tail[r] = lsb::red_store(F, acc, form);
  }
  return LSB_OK;
}

int lsb_plan_reduce(lsb_ctx_t* c, int op, int val_type) {
  const char* where = "lsb_plan_reduce";
  LSB_TRY(check_ctx(c));
  if (!lsb::reduce_valid(op, val_type)) return fail(LSB_ERR_INVALID, where, "op or value type");
  if (!c->runs_valid) return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs after the last change of A");
  c->reduce_valid = false;
  const int P = c->P;
  std::vector<uint64_t> lead((size_t)P, 0);
  if (c->n > 0) {
    // Ranks whose first slot goes on with an earlier rank's run reduce their leading run.
    std::vector<char> sent((size_t)P, 0);
    for (Rank& r : c->ranks) {
      if (r.here == 0) continue;
      HIP_TRY(hipSetDevice(r.dev));
      LSB_TRY(ensure_reduce_scratch(r));
      if (c->run_head0[r.rank]) continue;
      HIP_TRY(lsb::launch_run_lead(r.A, (int64_t)c->run_words[(size_t)r.rank * 4 + kLead], op, val_type, r.run_part,
                                   r.run_part + lsb::kRunLeadParts, r.stream));
      sent[r.rank] = 1;
    }
    LSB_TRY(gather_leads(c, sent, lead));
  }
  c->run_tail.assign((size_t)P, 0);
  if (lsb_plan_run_tails(c->n, P, c->run_words.data(), op, val_type, lead.data(), c->run_tail.data()) != LSB_OK)
    return fail(LSB_ERR_STATE, where, "the run plan's summary is inconsistent");
  c->reduce_op = op;
  c->reduce_type = val_type;
  c->reduce_valid = true;
  return LSB_OK;
}

int lsb_store_reduce(lsb_ctx_t* c, int rank, int64_t cap, void* out_dev, int64_t* runs) {
  const char* where = "lsb_store_reduce";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || cap < 0) return fail(LSB_ERR_INVALID, where, "rank or cap");
  if (!c->runs_valid || !c->reduce_valid)
    return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs and lsb_plan_reduce after the last change of A");
  const int64_t mine = c->run_count[rank];
  if (runs) *runs = mine;
  if (cap < mine) return fail(LSB_ERR_INVALID, where, "cap below the rank's runs");
  if (mine == 0) return LSB_OK;  // nothing to write: the pointer is not looked at
  if (!out_dev) return fail(LSB_ERR_INVALID, where, "null output");
  HIP_TRY(hipSetDevice(r->dev));
  LSB_TRY(check_column(*r, out_dev, 8, cap, where));
  LSB_TRY(ensure_reduce_scratch(*r));
  HIP_TRY(hipStreamSynchronize(r->stream));
  uint32_t h = 0;
  LSB_TRY(guarded_launch(*r, run_err(*r), &h, [&]() -> int {
    HIP_TRY(lsb::launch_run_reduce(r->A, r->here, c->run_head0[rank], r->run_cnt, r->run_tbase, c->reduce_op,
                                   c->reduce_type, c->run_tail[rank], r->run_lead, static_cast<uint64_t*>(out_dev),
                                   mine, run_err(*r), r->stream));
    return LSB_OK;
  }));
  if (h) {
    runs_invalidate(c);
    return fail(LSB_ERR_STATE, where, "A changed since lsb_count_runs: the outputs are unspecified");
  }
  return LSB_OK;
}

int lsb_plan_run_carries(int64_t n_total, int num_ranks, const uint64_t* summary, int op, int val_type,
                         const uint64_t* trail, uint64_t* carry) {
  const char* where = "lsb_plan_run_carries";
  if (n_total < 0 || num_ranks < 1 || num_ranks > LSB_MAX_RANKS || !summary || !trail || !carry ||
      !lsb::scan_valid(op, val_type))
    return fail(LSB_ERR_INVALID, where, "arguments");
  const int P = num_ranks;
  LSB_TRY(check_summary(n_total, P, summary, where));
  const int F = lsb::scan_form(op, val_type);
  const lsb::KeyForm form = lsb::key_form(val_type, 0);
  // own[s]: rank s has a head of its own (an inner one, or a run starts at its slot 0: lsb_plan_runs' head0).
  bool own[LSB_MAX_RANKS] = {};
  for (int r = 0, prev = -1; r < P; ++r) {
    if (here_of(n_total, P, r) == 0) continue;
    const uint64_t* w = summary + (size_t)r * 4;
    own[r] = w[kInner] > 0 || prev < 0 || summary[(size_t)prev * 4 + kLast] != w[kFirst];
    prev = r;
  }
  for (int r = 0; r < P; ++r) {
    uint64_t acc = lsb::red_identity(F);
    if (here_of(n_total, P, r) > 0) {
      // lsb_plan_run_tails' walk the other way: down from r - 1 through the
      // ranks whose last run is r's leading run, to the one that holds its head.
      const uint64_t* w = summary + (size_t)r * 4;
      int chain[LSB_MAX_RANKS], len = 0;
      for (int s = r - 1; s >= 0; --s) {
        if (here_of(n_total, P, s) == 0) continue;
        if (summary[(size_t)s * 4 + kLast] != w[kFirst]) break;
        chain[len++] = s;
        if (own[s]) break;
      }
      // the fold is a left one in increasing rank order
      while (len > 0) acc = lsb::red(F, acc, lsb::red_load(F, trail[chain[--len]], form));
    }
    carry[r] = lsb::red_store(F, acc, form);
  }
  return LSB_OK;
}

int lsb_plan_scan(lsb_ctx_t* c, int op, int val_type) {
  const char* where = "lsb_plan_scan";
  LSB_TRY(check_ctx(c));
  if (!lsb::scan_valid(op, val_type)) return fail(LSB_ERR_INVALID, where, "op or value type");
  if (!c->runs_valid) return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs after the last change of A");
  c->scan_valid = false;
  const int P = c->P;
  std::vector<uint64_t> trail((size_t)P, 0);
  if (c->n > 0) {
    for (Rank& r : c->ranks) {
      if (r.here == 0) continue;
      HIP_TRY(hipSetDevice(r.dev));
      LSB_TRY(ensure_scan_scratch(r));
      HIP_TRY(hipMemsetAsync(scan_err(r), 0, sizeof(uint64_t), r.stream));
      HIP_TRY(lsb::launch_run_scan_plan(r.A, r.here, c->run_head0[r.rank], r.run_cnt, op, val_type, scan_open(r),
                                        scan_in(r), scan_trail(r), scan_err(r), r.stream));
    }
    // The gather comes first: a rank whose guard fired still takes part in the collective.
    LSB_TRY(gather_trails(c, trail));
    uint32_t any = 0;
    LSB_TRY(read_guards(c, scan_err, &any));
    if (any) {
      runs_invalidate(c);
      return fail(LSB_ERR_STATE, where, "A changed since lsb_count_runs");
    }
  }
  c->run_carry.assign((size_t)P, 0);
  if (lsb_plan_run_carries(c->n, P, c->run_words.data(), op, val_type, trail.data(), c->run_carry.data()) != LSB_OK)
    return fail(LSB_ERR_STATE, where, "the run plan's summary is inconsistent");
  c->scan_op = op;
  c->scan_type = val_type;
  c->scan_valid = true;
  return LSB_OK;
}

int lsb_store_scan(lsb_ctx_t* c, int rank, int64_t cap, void* out_dev, int64_t* count) {
  const char* where = "lsb_store_scan";
  LSB_TRY(check_ctx(c));
  Rank* r = local_rank(c, rank);
  if (!r || cap < 0) return fail(LSB_ERR_INVALID, where, "rank or cap");
  if (!c->runs_valid || !c->scan_valid)
    return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs and lsb_plan_scan after the last change of A");
  const int64_t mine = r->here;
  if (count) *count = mine;
  if (cap < mine) return fail(LSB_ERR_INVALID, where, "cap below the rank's records");
  if (mine == 0) return LSB_OK;  // nothing to write: the pointer is not looked at
  if (!out_dev) return fail(LSB_ERR_INVALID, where, "null output");
  HIP_TRY(hipSetDevice(r->dev));
  LSB_TRY(check_column(*r, out_dev, 8, cap, where));
  HIP_TRY(hipStreamSynchronize(r->stream));
  uint32_t h = 0;
  LSB_TRY(guarded_launch(*r, scan_err(*r), &h, [&]() -> int {
    HIP_TRY(launch_scan_write(c, *r, lsb::kScanColumn, out_dev));
    return LSB_OK;
  }));
  if (h) {
    runs_invalidate(c);
    return fail(LSB_ERR_STATE, where, "A changed since lsb_count_runs: the output is unspecified");
  }
  return LSB_OK;
}

int lsb_scan_runs(lsb_ctx_t* c, int mode) {
  const char* where = "lsb_scan_runs";
  LSB_TRY(check_ctx(c));
  if (mode != LSB_LABEL_KEEP && mode != LSB_LABEL_BY_VALUE) return fail(LSB_ERR_INVALID, where, "mode");
  if (!c->runs_valid || !c->scan_valid)
    return fail(LSB_ERR_STATE, where, "no valid plan: call lsb_count_runs and lsb_plan_scan after the last change of A");
  // The records change (or a rank found them changed already): the plans end here either way.
  const int rc = c->n > 0 ? scan_ranks(c, mode) : LSB_OK;
  runs_invalidate(c);
  select_invalidate(c);
  search_invalidate(c);
  return rc;
}

}  // extern "C"
