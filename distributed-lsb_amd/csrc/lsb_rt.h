// Internal header of the runtime behind include/lsb.h: the context and rank
// state, error and timing helpers, and every function the runtime's
// translation units share.  Not part of the C ABI.
//
//   lsb_alloc.cpp     record buffers (VMM pieces) and the optional placement probe
//   lsb_context.cpp   context / rank buffers, timing, host collectives
//   lsb_passes.cpp    the local pass driver: reduce-then-scan passes,
//                     single-read passes (k_subhist + k_onesweep), the hybrid
//   lsb_exchange.cpp  the per-digit exchange (plan, all-to-all, placement,
//                     gathered passes; loopback, RCCL / host ops, peer stores)
//   lsb_wholekey.cpp  the whole-key exchange (splitter search, one all-to-all,
//                     merge of the P runs)
//   lsb_runs.cpp      runs of equal keys (lsb_plan_runs, lsb_count_runs,
//                     lsb_store_runs, lsb_plan_reduce, lsb_store_reduce,
//                     lsb_label_runs)
//   lsb_select.cpp    the k-th key and the first k + 1 records without a sort
//                     (lsb_plan_select, lsb_select, lsb_store_select)
//   lsb_search.cpp    a column of queries against a rank's sorted records
//                     (lsb_search) and the fence table the searches share
//   lsb_join.cpp      the matches themselves: the first match's value per
//                     query and the matched pairs (lsb_lookup, lsb_join_count,
//                     lsb_store_join)
//   lsb_abi.cpp       the extern "C" entry points and the host planners
//   lsb_xgeom.h       host-only exchange geometry (checked plan, waves); no
//                     device header, so host tools can include it alone
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/lsb.h"
#include "lsb_kernels.h"
#include "lsb_xgeom.h"

namespace lsb_rt {

using lsb::Elem;

// kLoopback: all ranks in this process (lsb_create); kRccl: this process is
// one rank, RCCL collectives (lsb_create_rank); kOps: one rank, the caller's
// host collectives (lsb_create_rank_ops).
enum class Mode { kLoopback, kRccl, kOps };

struct PendingEvent {
  int kid;
  int dev;
  int pass;  // local pass the launch is filed under (lsb_get_pass_stats), -1: none
  hipEvent_t start, stop;
};

struct Rank {
  int rank = 0;
  int dev = 0;
  hipStream_t stream = nullptr;
  hipStream_t pstream = nullptr;        // placement stream (overlaps the exchange)
  hipEvent_t pevent = nullptr;          // stream -> pstream handoff
  hipEvent_t pdone = nullptr;           // pstream -> stream: placement finished
  int64_t here = 0;
  Elem* A = nullptr;  // per slots: input / output (DistributedArray A)
  Elem* B = nullptr;  // per slots: ping-pong partner
  Elem* R = nullptr;  // per slots: receive buffer (P > 1 only)
  // A and B were chosen among placement_k candidate buffers (alloc_records;
  // 0: allocated as they came): ms of the probe copy, mean of both
  // directions, of the chosen pair, of the first two allocated, of the worst.
  int placement_k = 0;
  double placement_ms[3] = {0.0, 0.0, 0.0};
  uint32_t* chunk_hist = nullptr;       // [256][num_chunks]
  uint64_t* chunk_off = nullptr;        // [256][num_chunks]
  uint64_t* totals = nullptr;           // [256] local counts of the current 8-bit digit
  uint64_t* totals16 = nullptr;         // [65536] local counts of a 16-bit digit (bits = 16, P > 1)
  int64_t* first16 = nullptr;           // [65536] scratch of the 16-bit count
  bool starts_fused = false;            // first16 holds this digit's starts (marked by k_scatter)
  uint64_t* gather = nullptr;           // [P][nb] all-gathered counts
  int64_t* place = nullptr;             // [P][nb] place_off, then [P] rend (device plan)
  int64_t* plan_work = nullptr;         // [P][nb] device-plan scratch
  int64_t* plan_total = nullptr;        // [nb]    device-plan scratch
  int64_t* plan_counts = nullptr;       // [2P] send counts, recv counts
  unsigned long long* check = nullptr;  // [4] verify / check_sorted scratch; [2]: lsb_rekey_columns' error word
  uint64_t* span = nullptr;             // [2] OR of keys, OR of ~keys (first pass of lsb_sort)
  uint64_t* span_gather = nullptr;      // [2P] all-gathered spans (RCCL)
  uint64_t* span_h = nullptr;           // [2P] pinned host mirror
  int64_t* counts_h = nullptr;          // pinned host mirror of plan_counts
  lsb::Chunking chunking;
  // Peer-store exchange (LSB_OPT_EXCHANGE_PEER): the two physical record
  // buffers (A and B swap between them), every rank's two buffers as this
  // process sees them (IPC-opened for other processes), and the base table.
  Elem* buf[2] = {nullptr, nullptr};
  std::vector<Elem*> peer0, peer1;
  std::vector<void*> ipc_opened;
  int64_t* peer_base = nullptr;         // [nb]
  // Single-read passes (LSB_OPT_ONESWEEP, P == 1), allocated on first use.
  uint32_t* os_status = nullptr;        // [tiles][256] look-back granules (self-tagged u32)
  uint32_t* os_hist = nullptr;          // [2][8][256] sub-array histograms (ping-pong)
  uint32_t* os_ctr = nullptr;           // [8] tile counters, [8] look-back error word
  uint32_t* os_err_h = nullptr;         // pinned mirror of the error word
  uint32_t* os_hist_h = nullptr;        // pinned mirror of a sub-array histogram
  int os_halves = 1;                    // this sort's k_onesweep stage split (1 or 2)
  uint32_t os_epoch = 0;                // last look-back epoch
  int64_t os_rows = 0;                  // os_status rows the last launch wrote (lsb::status_fill)
  bool os_dirty = false;                // a launch failed: zero os_status before the next
  int64_t* seg_base = nullptr;          // [kOnesweepSubs][256] the hybrid's bucket bases (k_segfix)
  int os_grid = 0;                      // persistent grid (2 workgroups per CU)
  // The regional first pass (LSB_OPT_REGION_FIRST), allocated on first use:
  // the look-back rows of the pass that reads the regional layout (a track
  // of their own: that pass has more tiles than the others; launches of
  // different tile counts on one track refill rows), its epoch,
  // and rg_buf: region counts, the sample's histogram and span, the overflow
  // word (kRg* offsets, lsb_passes.cpp), rg_h its pinned mirror.
  int64_t cap = 0;                      // records A and B hold (>= here)
  int64_t rg_cap = 0;                   // slots per region (0: no regional first pass)
  uint32_t* os_status2 = nullptr;
  uint32_t os_epoch2 = 0;
  int64_t os_rows2 = 0;                 // os_status2 rows the last launch wrote (as os_rows)
  uint32_t* rg_buf = nullptr;
  uint32_t* rg_h = nullptr;
  // Per-digit exchange with single-read local passes (sort_exchange_onesweep):
  // os_hist[os_cur] is A's sub-array histogram of the byte at os_valid (-1:
  // none; the next pass reads A once with k_subhist).  The exchange's
  // placements count the byte at place_next into place_hist as they write.
  int os_cur = 0;
  int os_valid = -1;
  int place_next = -1;
  uint32_t* place_hist = nullptr;
  bool counts_ready = false;            // totals16 = this exchange digit's counts (k_onesweep C16)
  // Gathered passes (LSB_OPT_EXCHANGE_GATHER): an exchange whose placement
  // only counts leaves the peers' records in R and the rank's own in A; the
  // next local pass reads them there through gsrc (piece starts in gstart,
  // one descriptor per onesweep tile in gdesc), allocated on first use.
  bool gather_next = false;             // this exchange counts only
  bool gather_pending = false;          // the next local pass gathers
  int64_t* gstart = nullptr;            // [nb][P] piece starts in the placed order
  lsb::TileDesc* gdesc = nullptr;       // [tiles]
  lsb::GatherSrc gsrc;
  // The per-digit exchange in chunks (LSB_OPT_EXCHANGE_CHUNKS, lsb_exchange.cpp
  // exchange_chunked), allocated on first use: the wire stream, chunk k's
  // events (its high-byte pass done on `stream`, its records received on
  // xstream), the count kernel's per-chunk histograms and the plan's
  // per-chunk counts (device, pinned mirror), the low byte's histogram mirror.
  hipStream_t xstream = nullptr;
  hipEvent_t ck_hi[lsb::kMaxExchangeChunks] = {};
  hipEvent_t ck_wire[lsb::kMaxExchangeChunks] = {};
  hipEvent_t xdone = nullptr;
  uint32_t* ck_hist = nullptr;          // [C][8][256]
  int64_t* ck_counts = nullptr;         // [2][P][C]: send per (owner, chunk), recv per (source, chunk)
  int64_t* ck_counts_h = nullptr;
  uint32_t* lo_hist_h = nullptr;        // [8][256]
  // Whole-key exchange (radix_bits = 64), allocated on first use.
  uint64_t* split_state = nullptr;      // [Q][2] key interval per target
  int64_t* split_targets = nullptr;     // [Q] global positions q * per
  uint64_t* split_cnt = nullptr;        // [Q][kSplitCands] counts below the candidates
  uint64_t* split_gather = nullptr;     // [P][Q][kSplitCands] all-gathered
  uint64_t* split_fin = nullptr;        // [Q][2] #keys < k*, #keys <= k*
  uint64_t* split_fin_gather = nullptr; // [P][Q][2]
  uint64_t* split_h = nullptr;          // pinned mirror of split_fin_gather
  int64_t* merge_path = nullptr;        // merge-path tile boundaries
  int split_q = 0, split_S = 0;         // geometry the split buffers were sized for
  std::vector<int64_t> mcut;            // [P][P * S + 1] cuts of every source (host)
  // Runs of equal keys (lsb_runs.cpp), allocated on first use.
  uint32_t* run_cnt = nullptr;          // [run_tiles(here)] heads per tile (k_run_count)
  int64_t* run_tbase = nullptr;         // [run_tiles(here)] heads of the tiles before (k_run_scan)
  uint64_t* run_sum = nullptr;          // [kRunSumWords] summary words, k_run_write's error word
  uint64_t* run_lead = nullptr;         // [run_tiles(here)] k_run_reduce's tile leads (lsb_plan_reduce)
  uint64_t* run_part = nullptr;         // [kRunLeadParts + 1] k_run_lead's partials, then the leading run's word
  uint64_t* scan_buf = nullptr;         // [2 run_tiles(here) + 2] tile_open, tile_in, the trail word, the scan's error word (lsb_plan_scan)
  // The select (lsb_select.cpp), allocated on first use.
  uint64_t* sel_buf = nullptr;          // [kSelBufWords] a round's table, then lsb_store_select's error word
  uint64_t* sel_gather = nullptr;       // [P][kSelWords] all-gathered tables (one rank per process)
  uint32_t* sel_cnt = nullptr;          // [run_tiles(here)] keys below and equal to the pivot per tile (k_sel_count)
  int64_t* sel_tbase = nullptr;         // [run_tiles(here)][2] those of the tiles before (k_sel_scan)
  // The search (lsb_search.cpp), allocated on first use.
  uint64_t* search_fence = nullptr;     // [run_tiles(here)] the key of every tile's first record (k_search_fence)
  // The join plan (lsb_join.cpp), allocated at the first lsb_join_count and
  // regrown when a later one has more queries.
  int64_t* join_lower = nullptr;        // [join_cap] the records below every query
  int64_t* join_off = nullptr;          // [join_cap] the matches of the queries in front of every query
  int64_t* join_tile = nullptr;         // [join_qtiles(join_cap) + 1] tile bases of the scan, then the total
  int64_t join_cap = 0;                 // queries the three hold
  int64_t join_m = 0, join_total = 0;   // the plan: its queries and its pairs
  std::vector<int64_t> send_counts, send_displs, recv_counts, recv_displs;
};

}  // namespace lsb_rt

struct lsb_ctx {
  lsb_rt::Mode mode = lsb_rt::Mode::kLoopback;
  int64_t n = 0;
  int64_t per = 0;
  int P = 1;
  int bits = 8;      // exchange digit width: 8, 16, or 64 (the whole key: one exchange)
  int nb = 256;      // 1 << bits (256 for bits = 64: the buckets of the local passes)
  int first_rank = 0;
  std::vector<lsb_rt::Rank> ranks;  // local ranks
  ncclComm_t comm = nullptr;
  lsb_comm_ops_t ops = {};  // Mode::kOps
  bool timing = false;
  bool shared_device = false;  // two local ranks on one device (no placement probe)
  std::vector<int> access_devs;  // loopback: every device of the ranks (VMM record buffers map on all)
  bool force_exchange = false;
  bool skip_constant = true;  // lsb_sort skips digits on which all keys agree
  int slices = 0;             // exchange slices (placement overlaps the next slice); 0 = default
  int xchunks = 0;            // LSB_OPT_EXCHANGE_CHUNKS: 16-bit exchange digits in C chunks (0: off)
  int xchunk_reserve = 0;     // LSB_XCHUNK_RESERVE: workgroups the chunk passes leave to the wire
  bool p2p = false;           // RCCL exchange as grouped ncclSend/ncclRecv, not ncclAllToAllv
  bool peer = false;          // exchange by direct stores into the owners' buffers
  bool peer_ready = false;    // peer tables set up
  bool onesweep = true;       // P == 1: single-read passes (k_subhist + k_onesweep)
  bool region = true;         // LSB_OPT_REGION_FIRST: P == 1 LSD sorts start with the regional pass
  bool self_coll = false;     // the self segment also goes through the collective
  bool gather = true;         // LSB_OPT_EXCHANGE_GATHER: count-only placement + gathered pass
  int os_split = 0;           // LSB_OPT_ONESWEEP_SPLIT: 0 auto, 1 never, 2 always
  int fail_onesweep = 0;      // LSB_OPT_FAIL_ONESWEEP: the n-th k_onesweep launch fails (tests)
  int pack_values = 1;        // LSB_OPT_PACK_VALUES: 0 never, 1 when the values fit 32 bits, 2 always try
  int packed_tile = lsb::kOsTile10;  // LSB_PACKED_TILE: records per tile of a packed sort's middle passes
  unsigned edge_tiles = lsb::kOsEdgeAll;  // LSB_EDGE_TILES: the edge passes that may take the large tile too
  bool pack_wide = false;     // a packing first pass of this context met a value over 32 bits
  bool broken = false;        // a failed packed sort could not restore whole records: no more sorts
  int hybrid = 0;             // LSB_OPT_HYBRID: 0 off, 1 k byte passes (the last one
                              // ordering segments, + k_segfix), 2 the same + a k_segsort pass
  int64_t coll_calls = 0, coll_bytes = 0, coll_max = 0;  // element payload handed to the collective
  // What the last lsb_sort ran (lsb_get_last_sort).
  int last_local_passes = 0;
  int last_exchanges = 0;
  uint64_t last_varying = 0;
  int last_first = 0;  // the first pass's form (lsb_get_first_pass)
  int last_records = 0;  // the records between the passes (lsb_get_last_records)
  int last_packed_tile = 0;  // records per tile of the packed middle passes (lsb_get_last_packed_tile)
  int pass_tile[LSB_MAX_PASSES] = {};  // records per tile of each local pass (lsb_get_last_pass_tiles; 0: no k_onesweep)
  // The plan of the last lsb_count_runs (lsb_plan_runs over every rank's
  // summary), valid until an entry point that can change A (runs_invalidate).
  bool runs_valid = false;
  int64_t runs_total = 0;
  std::vector<int> run_head0;                         // [P]
  std::vector<int64_t> run_count, run_base, run_end;  // [P]
  std::vector<uint64_t> run_words;                    // [P][4] the gathered summary words
  // The plan of the last lsb_plan_reduce (lsb_plan_run_tails over every
  // rank's leading run); it dies with the run plan.
  bool reduce_valid = false;
  int reduce_op = 0, reduce_type = 0;
  std::vector<uint64_t> run_tail;                     // [P]
  // The plan of the last lsb_plan_scan (lsb_plan_run_carries over every
  // rank's trailing word), beside the reduce plan; it dies with the run plan.
  bool scan_valid = false;
  int scan_op = 0, scan_type = 0;
  std::vector<uint64_t> run_carry;                    // [P]
  // The plan of the last lsb_select (lsb_plan_select over every rank's
  // counts), valid until an entry point that can change A (select_invalidate);
  // the run plan and this one do not end each other.  What that call ran
  // outlives the plan (lsb_get_last_select).
  bool select_valid = false;
  uint64_t sel_pivot = 0;
  std::vector<int64_t> sel_below, sel_equal, sel_take, sel_base;  // [P]
  int sel_rounds = 0;
  int64_t sel_read = 0;
  // Bit r: rank r's search_fence is that of its A (lsb_search builds it),
  // until an entry point that can change A (search_invalidate).  lsb_select
  // leaves A bit for bit and writes B only, so it keeps the fences.
  uint64_t search_valid = 0;
  // Bit r: rank r's join plan (join_lower, join_off, join_m, join_total) is
  // that of its A (lsb_join_count), for as long as its fence table would be.
  uint64_t join_valid = 0;
  lsb::KeyGen keygen;
  std::vector<lsb_rt::PendingEvent> pending;
  std::vector<std::pair<int, hipEvent_t>> event_pool;  // (device, event) of finished timings
  int64_t launches[LSB_K_COUNT] = {};
  double total_ms[LSB_K_COUNT] = {};
  int64_t scatter_elems = 0;
  // Per local pass (lsb_get_pass_stats): the pass the next timed launch is
  // filed under (pass_cursor counts the local passes of the current sort).
  int cur_pass = 0;
  int pass_cursor = 0;
  int pass_shift[LSB_MAX_PASSES] = {};
  int64_t pass_launches[LSB_MAX_PASSES][LSB_K_COUNT] = {};
  double pass_ms[LSB_MAX_PASSES][LSB_K_COUNT] = {};
  int64_t pass_elems[LSB_MAX_PASSES] = {};
  // Exchange steps since the last reset (lsb_get_exchange_stats).
  int64_t xs_exchanges = 0, xs_calls = 0;
  int64_t xs_sent[LSB_MAX_RANKS] = {}, xs_recv[LSB_MAX_RANKS] = {};
  int64_t xs_place_bytes = 0, xs_placed = 0, xs_counted = 0;
  int64_t pass_xbytes[LSB_MAX_PASSES] = {};
};

#define HIP_TRY(expr)                                                    \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) return fail(LSB_ERR_HIP, #expr, hipGetErrorString(_e)); \
  } while (0)

#define RCCL_TRY(expr)                                                   \
  do {                                                                   \
    ncclResult_t _r = (expr);                                            \
    if (_r != ncclSuccess) return fail(LSB_ERR_RCCL, #expr, ncclGetErrorString(_r)); \
  } while (0)

#define LSB_TRY(expr)              \
  do {                             \
    int _c = (expr);               \
    if (_c != LSB_OK) return _c;   \
  } while (0)

namespace lsb_rt {

// ---- errors (lsb_context.cpp) ------------------------------------------------
// fail(code, what, detail) is declared in lsb_xgeom.h.
const std::string& last_error();

inline int64_t div_ceil(int64_t x, int64_t y) { return (x + y - 1) / y; }

inline int64_t here_of(int64_t n, int P, int r) {
  const int64_t per = P > 0 ? div_ceil(n, P) : 0;
  int64_t h = per;
  if (per * r + h > n) h = n - per * r;
  return h < 0 ? 0 : h;
}

inline bool exchanging(const lsb_ctx* c) { return c->P > 1 || c->force_exchange; }

// ---- timing (lsb_context.cpp) ----------------------------------------------
hipEvent_t take_event(lsb_ctx* c);

struct Timer {
  lsb_ctx* c;
  Rank* r;
  int kid;
  int pass;
  hipStream_t stream;
  hipEvent_t start = nullptr;
  Timer(lsb_ctx* c_, Rank* r_, int kid_, hipStream_t s = nullptr)
      : c(c_), r(r_), kid(kid_), pass(kid_ == LSB_K_SORT ? -1 : c_->cur_pass),
        stream(s ? s : r_->stream) {
    if (!c->timing) return;
    start = take_event(c);
    if (start) (void)hipEventRecord(start, stream);
  }
  void stop() {
    if (!start) return;
    hipEvent_t e = take_event(c);
    if (!e) return;
    (void)hipEventRecord(e, stream);
    c->pending.push_back({kid, r->dev, pass, start, e});
    start = nullptr;
  }
  ~Timer() { stop(); }
};

void begin_pass(lsb_ctx* c, int shift);
void count_pass_elems(lsb_ctx* c, int64_t m, bool scatter = true);
int resolve_timing(lsb_ctx* c);

// ---- allocation -----------------------------------------------------------
template <typename T>
int dev_alloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
  if (e != hipSuccess) return fail(LSB_ERR_NOMEM, "hipMalloc", hipGetErrorString(e));
  return LSB_OK;
}

template <typename T>
int host_alloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipHostMalloc(reinterpret_cast<void**>(p), count * sizeof(T), 0);
  if (e != hipSuccess) return fail(LSB_ERR_NOMEM, "hipHostMalloc", hipGetErrorString(e));
  return LSB_OK;
}

// ---- record buffers (lsb_alloc.cpp) and rank buffers (lsb_context.cpp) ---------
// Record buffers (A, B, R, candidates): VMM-backed in 1 GiB pieces when at
// least one piece long, else hipMalloc; rec_free frees either kind.
int rec_alloc(const lsb_ctx* c, Elem** p, size_t count);
int rec_alloc_group(const lsb_ctx* c, Elem** const* outs, int k, size_t count);
size_t rec_bytes(size_t count);  // device bytes rec_alloc takes for count records
void rec_free(void* p);
bool rec_is_vmm(const void* p);
// A VMM record buffer that RCCL has seen is being released (an RCCL
// context's A, B or R): later RCCL contexts of this process take hipMalloc'd
// record buffers (lsb_alloc.cpp, "RCCL and VMM address reuse").
void mark_rccl_vmm_released();
int max_chunks_for_device(int dev);
// Records A and B are allocated for: the block, or the regional first
// pass's slots when a P == 1 context's sorts may start with it (blocks of at
// least region_min() records: lsb::kRegionMin, or LSB_REGION_MIN >= 2^16).
int64_t region_min();
int64_t region_cap_for(int64_t per, int P);
int64_t record_capacity(int64_t per, int P);
// The placement probe's request for record buffers of `bytes`, before the
// free-memory cap: candidates K (<= 2: no probe) and the share of the free
// memory the K buffers may take.  LSB_PLACEMENT_CANDIDATES = K sets it (at
// most 8, 90 %); unset, buffers of at least kProbeMinBytes get
// kDefaultCandidates within half the free memory.
constexpr int kDefaultCandidates = 4;
constexpr double kProbeMinBytes = double(int64_t(4) << 30);
int placement_request(double bytes, double* free_share);
int alloc_records(lsb_ctx* c, Rank& r);  // A and B (placement-calibrated)
int alloc_third(lsb_ctx* c, Rank& r);    // R, placed against A and B
int init_rank(lsb_ctx* c, Rank& r, int rank, int dev);
// Frees r's buffers once r's streams are idle.  c (LSB_DEBUG builds): check
// first that every rank's streams of c are idle (teardown_check).
void free_rank(Rank& r, const lsb_ctx* c = nullptr);
// Debug builds: every rank's stream and placement stream must be idle before
// any record buffer of the context is unmapped (VMM unmapping does not wait
// for the device).  Reports each busy stream on stderr; returns how many.
int teardown_check(const lsb_ctx* c, const Rank& freeing);
Rank* local_rank(lsb_ctx* c, int rank);
int check_ctx(const lsb_ctx* c);
// A is about to change: lsb_store_runs and lsb_label_runs need a new
// lsb_count_runs, lsb_store_reduce a new lsb_plan_reduce after it.
inline void runs_invalidate(lsb_ctx* c) { c->runs_valid = c->reduce_valid = c->scan_valid = false; }
// A is about to change: lsb_store_select needs a new lsb_select.
inline void select_invalidate(lsb_ctx* c) { c->select_valid = false; }
// A is about to change: the searches build a rank's fence table again, and
// lsb_store_join needs a new lsb_join_count.
inline void search_invalidate(lsb_ctx* c) { c->search_valid = c->join_valid = 0; }
// r's fence table, allocated and built when search_valid says so
// (lsb_search.cpp); r.here > 0, r's device current, r's stream idle or ahead.
int ensure_search_fence(lsb_ctx* c, Rank& r);
// A caller's column of cnt elements of `elem` bytes at p, before a kernel may
// touch it (lsb_context.cpp): LSB_ERR_INVALID unless it is aligned to its element,
// device (or managed) memory of the rank's device and inside its allocation.
int check_column(const Rank& r, const void* p, size_t elem, int64_t cnt, const char* where);
lsb_ctx* new_ctx(int64_t n_total, int num_ranks, int radix_bits);

// ---- collectives (lsb_context.cpp) ------------------------------------------
int ops_fail(const char* what);
int coll_allgather_u64(lsb_ctx* c, Rank& r, const uint64_t* send, uint64_t* recv, size_t count);
// RCCL calls carry at most this many u64 (1 GiB) per peer (coll_alltoallv_u64).
constexpr size_t kMaxCallU64 = (size_t)1 << 27;
// The bound in force: kMaxCallU64, or LSB_RCCL_CALL_U64 (tests: a small bound
// makes small multi-rank sorts take the cut path, advisor r05).
size_t max_call_u64();
int coll_alltoallv_u64(lsb_ctx* c, Rank& r, const uint64_t* send, const size_t* sc,
                       const size_t* sd, uint64_t* recv, const size_t* rc, const size_t* rd,
                       size_t bound, hipStream_t stream = nullptr);
int gather_boundaries(lsb_ctx* c, std::vector<uint64_t>& bnd);
// out[r * W ..] = rank r's W words on the host, read from the device pointer
// src_of(rank) of the process that holds the rank; a null pointer gives zeros.
// Loopback reads each rank's own once its stream is done; a one-rank-per-
// process context all-gathers them in place through `area`, P * W words of
// device memory on ranks[0] (not looked at in loopback).
int gather_words(lsb_ctx* c, size_t W, uint64_t* area, const std::function<const uint64_t*(const Rank&)>& src_of,
                 std::vector<uint64_t>& out);
int allreduce_min_i64(lsb_ctx* c, int64_t* v);
int gather_span(lsb_ctx* c, uint64_t* kor, uint64_t* knor);

// ---- guarded launches ---------------------------------------------------------
// A kernel that writes from a plan recounts what the plan counted and sets its
// error word when A has changed since (lsb_tile.h's recount guard).  *h = the
// word of r at err, once r's stream is done.
inline int read_guard(Rank& r, const uint32_t* err, uint32_t* h) {
  *h = 0;
  HIP_TRY(hipMemcpyAsync(h, err, sizeof *h, hipMemcpyDeviceToHost, r.stream));
  HIP_TRY(hipStreamSynchronize(r.stream));
  return LSB_OK;
}
// The word zeroed, launch() (-> an LSB code) on r's stream, and the word read.
// What a set word means is the caller's: its text, and the plan it drops.
template <typename Launch>
int guarded_launch(Rank& r, uint32_t* err, uint32_t* h, Launch&& launch) {
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(uint64_t), r.stream));
  LSB_TRY(launch());
  return read_guard(r, err, h);
}

// recv[s * count ..] = send of rank s, for every local rank (loopback: device
// copies once every rank's stream is done; otherwise the collective).
template <typename SendOf, typename RecvOf>
int gather_ranks(lsb_ctx* c, size_t count, SendOf send_of, RecvOf recv_of) {
  if (c->mode != Mode::kLoopback) {
    Rank& r = c->ranks[0];
    HIP_TRY(hipSetDevice(r.dev));
    return coll_allgather_u64(c, r, send_of(r), recv_of(r), count);
  }
  for (Rank& r : c->ranks) {
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(hipStreamSynchronize(r.stream));
  }
  for (Rank& q : c->ranks) {
    HIP_TRY(hipSetDevice(q.dev));
    for (Rank& s : c->ranks)
      HIP_TRY(hipMemcpyAsync(recv_of(q) + (size_t)s.rank * count, send_of(s), count * 8,
                             hipMemcpyDefault, q.stream));
  }
  return LSB_OK;
}

// ---- local passes (lsb_passes.cpp) ------------------------------------------
int local_pass(lsb_ctx* c, Rank& r, int shift, bool want_span = false, bool starts16 = false);
int do_pass(lsb_ctx* c, int digit, uint64_t varying = ~0ull, bool want_span = false);
bool onesweep_applies(const lsb_ctx* c);
int onesweep_ensure(Rank& r);
int onesweep_launch(lsb_ctx* c, Rank& r, int shift, int next, const uint32_t* hist,
                    uint32_t* next_hist, lsb::OnesweepExtra x);
int queue_halves(lsb_ctx* c, Rank& r, const uint32_t* hist);
int choose_halves(lsb_ctx* c, Rank& r, bool synced);
int sort_onesweep(lsb_ctx* c);
int sort_local_rank(lsb_ctx* c, Rank& r, int* passes, uint64_t* varying);
int sort_local_ranks(lsb_ctx* c);  // every rank, step by step across ranks
int onesweep_check(Rank& r);
#ifdef LSB_OS_PROFILE
void os_profile_report();
#endif

// ---- per-digit exchange (lsb_exchange.cpp) ------------------------------------

// ---- placement, overlapped with the exchange ------------------------------
// Part j of n records cut into `slices` equal parts: [part(n, j), part(n, j + 1))
// (the whole-key exchange's owner slices).
inline int64_t part(int64_t n, int j, int slices) { return n * j / slices; }

// Slices of an exchange: the option, else 5 halving slices per exchange digit,
// or 8 equal slices for the whole-key exchange, whose one all-to-all carries
// every record: its last slice's merge (ceil(log2 P) levels) is the tail
// after the wire goes quiet.
inline int slices_of(const lsb_ctx* c) { return c->slices > 0 ? c->slices : (c->bits == 64 ? 8 : 5); }

// Records of slice j of any peer segment of a rank block of `per` records, at
// most: a slice of a segment of n records holds ceil(floor(n / 2^j) / 2) (the
// last: floor(n / 2^(S-1))), non-decreasing in n, and n <= per.
inline int64_t slice_bound(int64_t per, int j, int slices) {
  return slice_part(per, j + 1, slices) - slice_part(per, j, slices);
}
int ensure_recv(lsb_ctx* c, Rank& r);
int join_place(Rank& r);
int join_place_timed(lsb_ctx* c, Rank& r);
int exchange_digit(lsb_ctx* c, int digit);
// A loopback exchange's device copy of cnt records src (a record buffer of
// src_rank) -> dst (one of dst_rank's), checked against the buffers first.
bool in_buffers(const Rank& q, const Elem* p, int64_t cnt);
int copy_range(const lsb_ctx* c, Rank& dst_rank, Elem* dst, const Rank& src_rank, const Elem* src, int64_t cnt,
               hipStream_t s);
// One all-to-all-v step of every exchange: every local rank's wave w[i] moves
// out of its src[i] into its R on its stream `st` (Rank::stream or
// Rank::xstream), timed as LSB_K_WIRE.  Loopback: one copy_range per pair;
// one rank per process: one coll_alltoallv_u64, cut by `bound` records.
int wire_step(lsb_ctx* c, const std::vector<Wave>& w, const std::vector<Elem*>& src, int64_t bound,
              hipStream_t Rank::*st);
// The per-digit exchange in chunks: digit `digit` (16 bits) whose low-byte
// pass has run (A sorted by the low byte; lo_hist its input's sub-array
// histogram on each rank), high-byte passes chunk by chunk, each chunk's
// records on the wire while the next chunk's pass runs.
bool chunked_applies(const lsb_ctx* c, uint64_t varying, int digit);
int exchange_chunked(lsb_ctx* c, int digit, const std::vector<const uint32_t*>& lo_hist);
bool exchange_onesweep_applies(const lsb_ctx* c);
int sort_exchange_onesweep(lsb_ctx* c);

// ---- whole-key exchange (lsb_wholekey.cpp) ------------------------------------

// The cut geometry (MergeGeom, merge_geometry, merge_cuts, merge_owner_counts)
// is declared in lsb_xgeom.h.
int merge_sort(lsb_ctx* c);

}  // namespace lsb_rt
