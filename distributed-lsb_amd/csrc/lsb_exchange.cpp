// The per-digit exchange (radix_bits 8 / 16, P > 1 or forced): the reference's
// globalShuffle after its localShuffle (mpi/mpi_lsbsort.cpp:481-577).
//
// Per pass on digit d of `bits` bits (64 / bits passes, least significant
// first, mpi/mpi_lsbsort.cpp:580-585), for every rank r:
//   1. local stable pass(es) A -> B, then swap (localShuffle,
//      mpi/mpi_lsbsort.cpp:213-247): one 8-bit pass for bits = 8, two stable
//      8-bit sub-passes (low byte, high byte) for bits = 16.  A is then
//      ordered by digit d.
//   P == 1: done.
//   P  > 1:
//   2. the rank's bucket counts of digit d (k_scan totals for 8 bits,
//      run lengths of the sorted 16-bit digits for 16 bits), all-gathered
//      (replaces copyCountsToGlobalCounts + MPI_Exscan +
//      copyStartsFromGlobalStarts, mpi/mpi_lsbsort.cpp:327-479: every rank
//      scans the P x nbuckets matrix in digit-major, rank-minor order itself)
//   3. device plan (k_plan_*, same rule as lsb_plan_exchange): placement
//      table on the device, the 2P send/recv counts to the host
//   4. all-to-all-v of 16-byte records out of A into R (MPI_Alltoallv of
//      24-byte ShuffleBufSortElement at mpi/mpi_lsbsort.cpp:563; no
//      destination index travels: the receiver derives it from the counts),
//      cut into `slices` groups: slice j carries part j of every peer segment
//   5. k_place -> B on a second stream (mpi/mpi_lsbsort.cpp:568-575): the
//      self segment straight out of A at once, slice j of R as soon as it has
//      arrived, overlapping slice j+1 on the wire; then swap
//
// Three transports: in-process loopback (device copies standing in for the
// collectives), one rank per process (RCCL, or the caller's host callbacks),
// and the opt-in peer stores (shmem_putmem / MPI_Put form, exchange_peer).
// The first two differ in two places only, gather_ranks (step 2) and
// wire_step (step 4); the drivers around them are shared: exchange_sliced
// (steps 2-5 as above), exchange_chunked (the high-byte pass chunk by chunk
// under the wire) and lsb_wholekey.cpp's exchange_merge.  Every driver moves
// records by a plan checked on the host (plan_fetch, lsb_xgeom.h), one wave
// (lsb_xgeom.h) per step.  sort_exchange_onesweep is lsb_sort of these forms
// with single-read local passes and gathered passes after count-only
// placements.
#include "lsb_rt.h"

namespace lsb_rt {

// Device counts of the exchange digit for rank r (A is ordered by it).
int digit_counts(lsb_ctx* c, Rank& r, int digit, const uint64_t** counts) {
  if (c->bits == 8) {
    *counts = r.totals;  // k_scan totals of the (only) sub-pass
    return LSB_OK;
  }
  if (r.counts_ready) {  // counted by the high-byte k_onesweep
    *counts = r.totals16;
    return LSB_OK;
  }
  HIP_TRY(hipSetDevice(r.dev));
  {
    Timer t(c, &r, LSB_K_UPSWEEP);
    if (r.starts_fused)  // the high-byte scatter marked the starts
      HIP_TRY(lsb::launch_starts_to_counts(r.first16, r.here, r.totals16, r.stream));
    else  // high byte constant (skipped) or lsb_pass: read A once more
      HIP_TRY(lsb::launch_digit16_counts(r.A, r.here, digit * 16, r.first16, r.totals16,
                                         r.stream));
  }
  *counts = r.totals16;
  return LSB_OK;
}

// counts[i] (nb device words) of every rank into every local rank's gather
// matrix; the collective (not its loopback stand-in) is timed.
int gather_counts(lsb_ctx* c, const std::vector<const uint64_t*>& counts) {
  auto send = [&](Rank& r) { return counts[&r - c->ranks.data()]; };
  auto recv = [](Rank& r) { return r.gather; };
  if (c->mode == Mode::kLoopback) return gather_ranks(c, (size_t)c->nb, send, recv);
  HIP_TRY(hipSetDevice(c->ranks[0].dev));
  Timer t(c, &c->ranks[0], LSB_K_EXCHANGE);
  return gather_ranks(c, (size_t)c->nb, send, recv);
}

// Device plan of rank r from its gathered count matrix (r.gather): the
// placement table stays on the device; only the 2P send/recv counts come
// back (RCCL takes host counts).  cshift < 8 (exchange_chunked): the plan in
// chunk order, and its per-chunk counts come back too.  Call plan_fetch after
// a stream sync.
int plan_launch(lsb_ctx* c, Rank& r, int cshift = 8) {
  HIP_TRY(hipSetDevice(r.dev));
  if (r.gather_next && !r.gstart) {
    LSB_TRY(dev_alloc(&r.gstart, (size_t)2 * c->P * c->nb));  // gstart, then gadj
    LSB_TRY(dev_alloc(&r.gdesc, (size_t)lsb::onesweep_tiles(r.here)));
  }
  {
    Timer t(c, &r, LSB_K_EXCHANGE);
    HIP_TRY(lsb::launch_plan(r.gather, c->P, c->nb, r.rank, c->n, r.plan_work, r.plan_total, r.place,
                             r.plan_counts, r.stream, r.gather_next ? r.gstart : nullptr, cshift,
                             cshift < 8 ? r.ck_counts : nullptr));
  }
  HIP_TRY(hipMemcpyAsync(r.counts_h, r.plan_counts, sizeof(int64_t) * 2 * c->P,
                         hipMemcpyDeviceToHost, r.stream));
  if (cshift < 8)
    HIP_TRY(hipMemcpyAsync(r.ck_counts_h, r.ck_counts, sizeof(int64_t) * 2 * c->P * (lsb::kBuckets >> cshift),
                           hipMemcpyDeviceToHost, r.stream));
  return LSB_OK;
}

// The plan on the host, checked (checked_plan): no record moves by a plan
// whose counts do not add up to the block.
int plan_fetch(lsb_ctx* c, Rank& r) {
  return checked_plan(r.counts_h, c->P, r.here, r.send_counts.data(), r.send_displs.data(),
                      r.recv_counts.data(), r.recv_displs.data());
}


// After an exchange's placements: B holds the placed block and becomes A, or
// (count-only placement) the next pass gathers from R and A.
void end_placement(Rank& r) {
  if (r.gather_next) r.gather_pending = true;
  else std::swap(r.A, r.B);
}

// Everything after this on r.stream waits for r.pstream's work so far.
int join_place(Rank& r) {
  HIP_TRY(hipEventRecord(r.pdone, r.pstream));
  HIP_TRY(hipStreamWaitEvent(r.stream, r.pdone, 0));
  return LSB_OK;
}

// join_place after the last slice of an exchange, timed (LSB_K_PLACE_TAIL):
// from the moment the rank's stream has issued its last transfer to the end
// of the placement, i.e. the placement work not overlapped with the wire.
int join_place_timed(lsb_ctx* c, Rank& r) {
  Timer t(c, &r, LSB_K_PLACE_TAIL);
  return join_place(r);
}

// [p, p + cnt) lies inside one of rank q's record buffers.  Every device
// copy and placement of the exchange checks its ranges on the host first, so
// a plan gone wrong fails the sort instead of faulting the device.
bool in_buffers(const Rank& q, const Elem* p, int64_t cnt) {
  for (const Elem* b : {q.A, q.B, q.R})
    if (b && cnt >= 0 && p >= b && p + cnt <= b + q.cap) return true;
  return false;
}

int copy_range(const lsb_ctx*, Rank& dst_rank, Elem* dst, const Rank& src_rank, const Elem* src, int64_t cnt,
               hipStream_t s) {
  if (cnt <= 0) return LSB_OK;
  if (!in_buffers(dst_rank, dst, cnt) || !in_buffers(src_rank, src, cnt))
    return fail(LSB_ERR_STATE, "exchange copy", "range outside the record buffers");
  if (dst_rank.dev == src_rank.dev) {
    // One device: a copy kernel (addresses through the page tables only).
    HIP_TRY(lsb::launch_copy_records(dst, src, cnt, s));
  } else {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)cnt * sizeof(Elem), hipMemcpyDefault, s));
  }
  return LSB_OK;
}

// Place one source's received range [k0, k0 + cnt) (records at src) into B.
int place_range(lsb_ctx* c, Rank& r, int shift, int src_rank, const Elem* src, int64_t k0,
                int64_t cnt) {
  if (cnt <= 0) return LSB_OK;
  if (!in_buffers(r, src, cnt) || k0 < 0 || k0 + cnt > r.cap)
    return fail(LSB_ERR_STATE, "exchange placement", "range outside the record buffers");
  // 32 algorithmic bytes per placed record, 16 per record only counted
  c->xs_place_bytes += cnt * (r.gather_next ? 16 : 32);
  (r.gather_next ? c->xs_counted : c->xs_placed) += cnt;
  Timer t(c, &r, LSB_K_PLACE, r.pstream);
  HIP_TRY(lsb::launch_place(src, r.B, r.here, k0, cnt, shift, c->nb,
                            r.place + (size_t)src_rank * c->nb, r.pstream, r.place_next,
                            r.place_hist, !r.gather_next, r.os_halves == 2));
  return LSB_OK;
}

// The receive buffer, allocated at the first all-to-all of the context.
int ensure_recv(lsb_ctx* c, Rank& r) {
  if (r.R) return LSB_OK;
  HIP_TRY(hipSetDevice(r.dev));
  return alloc_third(c, r);
}

// The self segment stays where it is unless LSB_OPT_EXCHANGE_SELF sends it
// through the collective like every other source's.
bool self_in_r(const lsb_ctx* c) { return c->self_coll && c->mode != Mode::kLoopback; }

// Where the next (gathered) pass will find each tile's records: peers'
// pieces in R, the rank's own in `own`, chunk k's self_adj[k] records further
// on than in R (chunk_shift 8: one chunk).
int gather_desc(lsb_ctx* c, Rank& r, const Elem* own, const int64_t (&self_adj)[lsb::kMaxExchangeChunks],
                int chunk_shift) {
  lsb::GatherSrc& g = r.gsrc;
  g.R = r.R;
  g.A = own;
  std::copy(std::begin(self_adj), std::end(self_adj), g.self_adj);
  g.chunk_shift = chunk_shift;
  g.place = r.place;
  g.gstart = r.gstart;
  g.gadj = r.gstart + (size_t)c->P * c->nb;
  g.desc = r.gdesc;
  g.P = c->P;
  g.nb = c->nb;
  g.me = r.rank;
  g.self_in_a = !self_in_r(c);
  g.a_len = g.r_len = r.cap;
  HIP_TRY(hipSetDevice(r.dev));
  Timer t(c, &r, LSB_K_EXCHANGE);
  HIP_TRY(lsb::launch_gather_desc(g, r.here, r.gdesc, r.stream));
  return LSB_OK;
}

// The self segment needs no transfer: place it straight out of A as soon as
// the plan is on the device (call after the host has the plan).  With
// LSB_OPT_EXCHANGE_SELF it travels through the collective instead and is
// placed from R by place_wave like every other source.
int place_self(lsb_ctx* c, Rank& r, int shift) {
  const int me = r.rank;
  if (r.send_counts[me] != r.recv_counts[me])
    return fail(LSB_ERR_STATE, "exchange", "self count mismatch");
  LSB_TRY(ensure_recv(c, r));
  if (r.gather_next) {
    int64_t adj[lsb::kMaxExchangeChunks];
    std::fill(std::begin(adj), std::end(adj), r.send_displs[me] - r.recv_displs[me]);
    LSB_TRY(gather_desc(c, r, r.A, adj, 8));
  }
  if (self_in_r(c)) return LSB_OK;
  HIP_TRY(hipSetDevice(r.dev));
  HIP_TRY(hipEventRecord(r.pevent, r.stream));  // plan kernels done
  HIP_TRY(hipStreamWaitEvent(r.pstream, r.pevent, 0));
  return place_range(c, r, shift, me, r.A + r.send_displs[me], r.recv_displs[me],
                     r.recv_counts[me]);
}

// Place a received wave on r.pstream: every source's range of R, and the
// rank's own records (unless they came through the collective) out of `own`
// where the wave sends them from; own == nullptr: placed already (place_self).
int place_wave(lsb_ctx* c, Rank& r, int shift, const Wave& w, const Elem* own) {
  for (int s = 0; s < c->P; ++s) {
    const Elem* src = r.R + w.roff[s];
    if (s == r.rank && !self_in_r(c)) {
      if (!own) continue;
      src = own + w.soff[s];
    }
    LSB_TRY(place_range(c, r, shift, s, src, w.roff[s], w.rcnt[s]));
  }
  return LSB_OK;
}

// One all-to-all-v step (lsb_rt.h).  Loopback: part q of rank s's source ->
// rank q's R, after the check the collective's two ends cannot make: that
// sender and receiver agree on the count.  One rank per process: the
// collective in uint64 units (ncclAllToAllv; the reference's MPI_Alltoallv,
// mpi/mpi_lsbsort.cpp:316-324); the own entry is 0 because the own records
// are used where they lie (unless LSB_OPT_EXCHANGE_SELF sends them too).
int wire_step(lsb_ctx* c, const std::vector<Wave>& w, const std::vector<Elem*>& src, int64_t bound,
              hipStream_t Rank::*st) {
  const int P = c->P;
  if (c->mode == Mode::kLoopback) {
    for (int q = 0; q < P; ++q) {
      Rank& rq = c->ranks[q];
      HIP_TRY(hipSetDevice(rq.dev));
      Timer t(c, &rq, LSB_K_WIRE, rq.*st);
      for (int s = 0; s < P; ++s) {
        if (s == q) continue;
        if (w[s].scnt[q] != w[q].rcnt[s]) return fail(LSB_ERR_STATE, "exchange", "send/recv count mismatch");
        LSB_TRY(copy_range(c, rq, rq.R + w[q].roff[s], c->ranks[s], src[s] + w[s].soff[q], w[q].rcnt[s], rq.*st));
      }
    }
    return LSB_OK;
  }
  Rank& r = c->ranks[0];
  HIP_TRY(hipSetDevice(r.dev));
  std::vector<size_t> sc(P), sd(P), rc(P), rd(P);
  for (int q = 0; q < P; ++q) {
    const bool skip = q == r.rank && !c->self_coll;
    sc[q] = skip ? 0 : (size_t)w[0].scnt[q] * 2;
    rc[q] = skip ? 0 : (size_t)w[0].rcnt[q] * 2;
    sd[q] = (size_t)w[0].soff[q] * 2;
    rd[q] = (size_t)w[0].roff[q] * 2;
  }
  Timer t(c, &r, LSB_K_WIRE, r.*st);
  return coll_alltoallv_u64(c, r, reinterpret_cast<const uint64_t*>(src[0]), sc.data(), sd.data(),
                            reinterpret_cast<uint64_t*>(r.R), rc.data(), rd.data(), (size_t)bound * 2, r.*st);
}

// How RCCL calls of more than 1 GiB per peer are cut (coll_alltoallv_u64),
// alike on every rank: by the largest segment of this exchange on any rank
// (the local ones: send, recv [q * C + k]), one all-reduce of one word, asked
// only when a block could exceed the bound at all (may_exceed); else by the
// rank block.
int call_bound(lsb_ctx* c, const int64_t* send, const int64_t* recv, int C, bool may_exceed, int64_t* seg) {
  *seg = c->per;
  if (c->mode != Mode::kRccl || !may_exceed) return LSB_OK;
  int64_t neg = -max_segment(send, recv, c->P, C, c->self_coll ? -1 : c->ranks[0].rank);
  LSB_TRY(allreduce_min_i64(c, &neg));
  *seg = -neg;
  return LSB_OK;
}

// Every local rank's counts of the exchange digit into every local rank's
// gather matrix.
int gather_digit_counts(lsb_ctx* c, int digit) {
  std::vector<const uint64_t*> counts(c->ranks.size(), nullptr);
  for (size_t i = 0; i < c->ranks.size(); ++i) LSB_TRY(digit_counts(c, c->ranks[i], digit, &counts[i]));
  return gather_counts(c, counts);
}

// ---- exchange: in slices (loopback, RCCL, the caller's collectives) --------
int exchange_sliced(lsb_ctx* c, int digit) {
  const int shift = digit * c->bits, S = slices_of(c);
  const size_t nr = c->ranks.size();
  LSB_TRY(gather_digit_counts(c, digit));
  for (Rank& r : c->ranks) LSB_TRY(plan_launch(c, r));
  for (Rank& r : c->ranks) {
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(hipStreamSynchronize(r.stream));
    LSB_TRY(plan_fetch(c, r));
  }
  for (Rank& r : c->ranks) LSB_TRY(place_self(c, r, shift));
  const Rank& r0 = c->ranks[0];
  int64_t seg = 0;
  LSB_TRY(call_bound(c, r0.send_counts.data(), r0.recv_counts.data(), 1,
                     (size_t)slice_bound(c->per, 0, S) * 2 > max_call_u64(), &seg));
  // all-to-all-v out of the digit-ordered A, slice by slice; slice j is
  // placed on r.pstream while r.stream carries slice j + 1.
  std::vector<Wave> w(nr);
  std::vector<Elem*> src(nr);
  for (size_t i = 0; i < nr; ++i) src[i] = c->ranks[i].A;
  for (int j = 0; j < S; ++j) {
    for (size_t i = 0; i < nr; ++i) {
      const Rank& r = c->ranks[i];
      slice_wave(c->P, r.send_counts.data(), r.send_displs.data(), r.recv_counts.data(), r.recv_displs.data(), j, S,
                 w[i]);
    }
    LSB_TRY(wire_step(c, w, src, slice_bound(seg, j, S), &Rank::stream));
    for (size_t i = 0; i < nr; ++i) {
      Rank& r = c->ranks[i];
      HIP_TRY(hipSetDevice(r.dev));
      HIP_TRY(hipEventRecord(r.pevent, r.stream));
      HIP_TRY(hipStreamWaitEvent(r.pstream, r.pevent, 0));
      LSB_TRY(place_wave(c, r, shift, w[i], nullptr));
    }
  }
  // Loopback: every rank's copies out of A must be done before any rank's
  // next pass rewrites that A (it becomes B after the swap).
  for (Rank& r : c->ranks) {
    LSB_TRY(join_place_timed(c, r));
    if (c->mode == Mode::kLoopback) HIP_TRY(hipStreamSynchronize(r.stream));
    end_placement(r);
  }
  return LSB_OK;
}

// ---- exchange: peer stores (opt-in, LSB_OPT_EXCHANGE_PEER) ----------------
// Each rank writes its records straight into its owners' receiving buffers
// (shmem_putmem / MPI_Put in the reference, shmem/shmem_lsbsort.cpp:441-456,
// mpi/mpi_lsbsort_onesided.cpp:487-509): no R buffer, no all-to-all, no
// placement pass.  Ordering: the counts all-gather cannot complete before
// every rank's local pass has (stream order), so no store lands in a buffer
// still being read; a barrier after the stores orders them before any
// rank's next pass.  Visibility across GPUs is made explicit rather than left
// to kernel boundaries: k_peer_scatter ends every workgroup with a
// system-scope release (L2 write-back of the XCD), and after the barrier the
// owner runs a system-scope acquire on every XCD (L2 invalidate) before its
// next pass reads the buffer.

// Every rank's two physical buffers as this process sees them.
int peer_setup(lsb_ctx* c) {
  if (c->peer_ready) return LSB_OK;
  const int P = c->P;
  if (c->mode == Mode::kLoopback) {
    for (Rank& r : c->ranks) {
      r.peer0.assign(P, nullptr);
      r.peer1.assign(P, nullptr);
      HIP_TRY(hipSetDevice(r.dev));
      for (Rank& q : c->ranks) {
        r.peer0[q.rank] = q.buf[0];
        r.peer1[q.rank] = q.buf[1];
        if (q.dev != r.dev) {
          hipError_t e = hipDeviceEnablePeerAccess(q.dev, 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            return fail(LSB_ERR_HIP, "hipDeviceEnablePeerAccess", hipGetErrorString(e));
          (void)hipGetLastError();
        }
      }
    }
    c->peer_ready = true;
    return LSB_OK;
  }
  // One rank per process: IPC handles of both buffers, all-gathered.
  Rank& r = c->ranks[0];
  HIP_TRY(hipSetDevice(r.dev));
  // IPC handles name hipMalloc memory only: a record buffer built from VMM
  // pieces (rec_alloc) is replaced by a hipMalloc'd one holding its records,
  // of the same capacity: a later sort with the exchange off may start with
  // the regional first pass, which writes r.cap slots (advisor r05).
  for (int k = 0; k < 2; ++k) {
    Elem* old = r.buf[k];
    if (!rec_is_vmm(old)) continue;
    Elem* nu = nullptr;
    LSB_TRY(dev_alloc(&nu, (size_t)std::max(r.cap, c->per)));
    HIP_TRY(hipMemcpyAsync(nu, old, sizeof(Elem) * (size_t)c->per, hipMemcpyDeviceToDevice, r.stream));
    HIP_TRY(hipStreamSynchronize(r.stream));
    for (Elem** p : {&r.A, &r.B, &r.R})
      if (*p == old) *p = nu;
    r.buf[k] = nu;
    if (c->mode == Mode::kRccl) mark_rccl_vmm_released();
    rec_free(old);
  }
  static_assert(sizeof(hipIpcMemHandle_t) % 8 == 0, "handle in u64 words");
  constexpr size_t kW = sizeof(hipIpcMemHandle_t) / 8;  // words per handle
  std::vector<uint64_t> mine(2 * kW), all((size_t)P * 2 * kW);
  HIP_TRY(hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(mine.data()), r.buf[0]));
  HIP_TRY(hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(mine.data() + kW), r.buf[1]));
  uint64_t* d = r.gather;  // >= P * 2 * kW words (P * nb, nb >= 256)
  HIP_TRY(hipMemcpyAsync(d + (size_t)r.rank * 2 * kW, mine.data(), 2 * kW * 8,
                         hipMemcpyHostToDevice, r.stream));
  LSB_TRY(coll_allgather_u64(c, r, d + (size_t)r.rank * 2 * kW, d, 2 * kW));
  HIP_TRY(hipMemcpyAsync(all.data(), d, all.size() * 8, hipMemcpyDeviceToHost, r.stream));
  HIP_TRY(hipStreamSynchronize(r.stream));
  r.peer0.assign(P, nullptr);
  r.peer1.assign(P, nullptr);
  for (int q = 0; q < P; ++q) {
    if (q == r.rank) {
      r.peer0[q] = r.buf[0];
      r.peer1[q] = r.buf[1];
      continue;
    }
    for (int k = 0; k < 2; ++k) {
      hipIpcMemHandle_t h;
      memcpy(&h, all.data() + ((size_t)q * 2 + k) * kW, sizeof h);
      void* p = nullptr;
      HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
      r.ipc_opened.push_back(p);
      (k == 0 ? r.peer0 : r.peer1)[q] = static_cast<Elem*>(p);
    }
  }
  c->peer_ready = true;
  return LSB_OK;
}

// All ranks' stores are done: loopback waits for every stream, one rank per
// process runs a barrier collective after its own stores.
int peer_barrier(lsb_ctx* c) {
  if (c->mode == Mode::kLoopback) {
    for (Rank& r : c->ranks) {
      HIP_TRY(hipSetDevice(r.dev));
      HIP_TRY(hipStreamSynchronize(r.stream));
    }
    return LSB_OK;
  }
  Rank& r = c->ranks[0];
  HIP_TRY(hipSetDevice(r.dev));
  if (c->mode == Mode::kRccl) {
    RCCL_TRY(ncclAllReduce(r.check, r.check, 1, ncclUint64, ncclSum, c->comm, r.stream));
    return LSB_OK;
  }
  HIP_TRY(hipStreamSynchronize(r.stream));
  return c->ops.barrier(c->ops.user) == 0 ? LSB_OK : ops_fail("barrier");
}

int exchange_peer(lsb_ctx* c, int digit) {
  const int shift = digit * c->bits;
  const size_t nb = (size_t)c->nb;
  LSB_TRY(peer_setup(c));
  LSB_TRY(gather_digit_counts(c, digit));
  for (Rank& r : c->ranks) {
    HIP_TRY(hipSetDevice(r.dev));
    if (!r.peer_base) {
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r.peer_base), sizeof(int64_t) * nb));
    }
    // Every rank swaps alike, so B is the same physical buffer index everywhere.
    const bool free1 = r.B == r.buf[1];
    Timer t(c, &r, LSB_K_WIRE);  // the stores are the transfer (no payload counted)
    HIP_TRY(lsb::launch_peer_exchange(r.A, r.here, shift, c->nb, r.gather, c->P, r.rank, c->per,
                                      (free1 ? r.peer1 : r.peer0).data(), r.peer_base,
                                      r.stream));
  }
  LSB_TRY(peer_barrier(c));
  for (Rank& r : c->ranks) {
    // Acquire what the peers released (k_peer_scatter's system-scope fence).
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(lsb::launch_system_acquire(r.stream));
    std::swap(r.A, r.B);
  }
  return LSB_OK;
}

int exchange_digit(lsb_ctx* c, int digit) {
  ++c->xs_exchanges;
  if (c->peer) return exchange_peer(c, digit);
  return exchange_sliced(c, digit);
}

// ---- the per-digit exchange in chunks (LSB_OPT_EXCHANGE_CHUNKS) -------------
// the exchange of chunk k overlaps the local
// work of chunk k + 1.  The reference runs localShuffle to the end and only
// then the whole exchange (mpi/mpi_lsbsort.cpp:481-577), and so does
// exchange_digit: the high-byte pass, then the wire.  Here, for a 16-bit
// digit d whose low-byte pass has run (A sorted by the low byte l):
//   1. one read of A (launch_count16_chunks) counts the digit's 65536 values
//      and, per chunk k (the records with l in [k 256 / C, (k + 1) 256 / C):
//      a contiguous range of A), the high byte's sub-array histogram;
//   2. the counts are all-gathered and planned as before, except that a
//      source's pieces lie in R in chunk order (launch_plan with cshift);
//   3. chunk by chunk: chunk k's high-byte pass (one k_onesweep over its range
//      of A, into the same range of B) on the rank's stream, then chunk k's
//      all-to-all on the wire stream while chunk k + 1's pass runs, then its
//      count-only placement (or, the last exchange, its placement once every
//      pass is done) on the placement stream.
// Inside chunk k the records end up ordered by (h, l), so every owner's
// share is one contiguous range, and a digit's records all lie in one chunk:
// the placed order, (digit, source), is the reference's, and the output is
// the same bit for bit.  The price is step 1's read (16 B per record); what it
// buys is the high-byte pass under the wire.
constexpr int64_t kChunkMinPer = int64_t(1) << 16;

bool chunked_applies(const lsb_ctx* c, uint64_t varying, int digit) {
  if (c->xchunks < 2 || c->bits != 16 || c->peer || c->mode == Mode::kOps || !exchanging(c)) return false;
  const int lo = digit * 16;
  if (((varying >> lo) & 0xFF) == 0 || ((varying >> (lo + 8)) & 0xFF) == 0) return false;
  return c->per >= kChunkMinPer;
}

namespace {

int cshift_of(int C) { return C >= 8 ? 5 : C == 4 ? 6 : 7; }

int chunk_ensure(lsb_ctx* c, Rank& r) {
  if (r.xstream) return LSB_OK;
  HIP_TRY(hipSetDevice(r.dev));
  if (!r.ck_hist) LSB_TRY(dev_alloc(&r.ck_hist, (size_t)lsb::kMaxExchangeChunks * lsb::kOnesweepSubs * lsb::kBuckets));
  if (!r.ck_counts) LSB_TRY(dev_alloc(&r.ck_counts, (size_t)2 * c->P * lsb::kMaxExchangeChunks));
  if (!r.ck_counts_h) LSB_TRY(host_alloc(&r.ck_counts_h, (size_t)2 * c->P * lsb::kMaxExchangeChunks));
  if (!r.lo_hist_h) LSB_TRY(host_alloc(&r.lo_hist_h, (size_t)lsb::kOnesweepSubs * lsb::kBuckets));
  for (hipEvent_t& e : r.ck_hi)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t& e : r.ck_wire)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!r.xdone) HIP_TRY(hipEventCreateWithFlags(&r.xdone, hipEventDisableTiming));
  HIP_TRY(hipStreamCreateWithFlags(&r.xstream, hipStreamNonBlocking));  // last: marks the set complete
  return LSB_OK;
}

}  // namespace

int exchange_chunked(lsb_ctx* c, int digit, const std::vector<const uint32_t*>& lo_hist) {
  ++c->xs_exchanges;
  const int C = std::min(c->xchunks, lsb::kMaxExchangeChunks), cs = cshift_of(C), P = c->P;
  const int shift = digit * 16, hi_shift = shift + lsb::kDigitBits;
  const size_t nr = c->ranks.size();
  std::vector<ChunkGeom> geo(nr);
  std::vector<Wave> w(nr);
  std::vector<Elem*> X(nr), Y(nr);  // the high-byte pass reads X (A, sorted by l) and writes Y (B)
  // 1. the count read
  for (size_t i = 0; i < nr; ++i) {
    Rank& r = c->ranks[i];
    LSB_TRY(chunk_ensure(c, r));
    LSB_TRY(ensure_recv(c, r));
    HIP_TRY(hipSetDevice(r.dev));
    X[i] = r.A;
    Y[i] = r.B;
    {
      Timer t(c, &r, LSB_K_UPSWEEP);
      HIP_TRY(lsb::launch_count16_chunks(r.A, r.here, shift, lo_hist[i], cs, r.os_grid, r.totals16, r.ck_hist,
                                         r.stream));
    }
    HIP_TRY(hipMemcpyAsync(r.lo_hist_h, lo_hist[i], sizeof(uint32_t) * lsb::kOnesweepSubs * lsb::kBuckets,
                           hipMemcpyDeviceToHost, r.stream));
  }
  // 2. the counts to every rank, the plan in chunk order
  std::vector<const uint64_t*> counts(nr);
  for (size_t i = 0; i < nr; ++i) counts[i] = c->ranks[i].totals16;
  LSB_TRY(gather_counts(c, counts));
  for (Rank& r : c->ranks) LSB_TRY(plan_launch(c, r, cs));
  for (size_t i = 0; i < nr; ++i) {
    Rank& r = c->ranks[i];
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(hipStreamSynchronize(r.stream));
    LSB_TRY(plan_fetch(c, r));
    LSB_TRY(chunk_geom(P, C, r.here, r.lo_hist_h, lsb::kBuckets, lsb::kOnesweepSubs, r.ck_counts_h,
                       r.send_counts.data(), r.recv_counts.data(), geo[i]));
  }
  // Where the next (gathered) pass finds each tile's records: peers' pieces
  // in R, my own in Y, chunk k's at its own offset.
  for (size_t i = 0; i < nr; ++i) {
    Rank& r = c->ranks[i];
    if (!r.gather_next) continue;
    int64_t adj[lsb::kMaxExchangeChunks] = {};
    for (int k = 0; k < C; ++k) {
      chunk_wave(P, C, geo[i], r.recv_displs.data(), k, w[i]);
      adj[k] = w[i].soff[r.rank] - w[i].roff[r.rank];
    }
    LSB_TRY(gather_desc(c, r, Y[i], adj, cs));
  }
  int64_t seg = 0;
  LSB_TRY(call_bound(c, geo[0].send.data(), geo[0].recv.data(), C,
                     (size_t)c->per * 2 > max_call_u64() /* a chunk may hold the block */, &seg));
  // 3. chunk by chunk: the high-byte pass, then the wire
  for (int k = 0; k < C; ++k) {
    for (size_t i = 0; i < nr; ++i) {
      Rank& r = c->ranks[i];
      HIP_TRY(hipSetDevice(r.dev));
      const int64_t lo = geo[i].lo[k], m = geo[i].lo[k + 1] - lo;
      if (m > 0) {
        // Chunk passes differ in tile count: each starts from zeroed look-back
        // rows (epoch 1), and the next plain pass zeroes them all (os_dirty).
        r.os_dirty = true;
        HIP_TRY(hipMemsetAsync(r.os_status, 0, (size_t)lsb::onesweep_tiles(m) * lsb::kBuckets * sizeof(uint32_t),
                               r.stream));
        lsb::OnesweepExtra x;
        x.halves = r.os_halves;
        const int grid = std::max(lsb::kOnesweepSubs, (r.os_grid - c->xchunk_reserve) / 8 * 8);
        hipError_t e;
        if (c->fail_onesweep > 0 && --c->fail_onesweep == 0)  // LSB_OPT_FAIL_ONESWEEP (tests)
          return fail(LSB_ERR_HIP, "exchange_chunked: launch_onesweep", "injected launch failure (LSB_OPT_FAIL_ONESWEEP)");
        {
          Timer t(c, &r, LSB_K_SCATTER);
          e = lsb::launch_onesweep(X[i] + lo, Y[i] + lo, m, hi_shift, -1,
                                   r.ck_hist + (size_t)k * lsb::kOnesweepSubs * lsb::kBuckets, nullptr, r.os_status,
                                   r.os_ctr, 1, r.os_ctr + lsb::kOnesweepSubs, grid, r.stream, x);
        }
        if (e != hipSuccess) {
          (void)hipGetLastError();
          return fail(LSB_ERR_HIP, "exchange_chunked: launch_onesweep", hipGetErrorString(e));
        }
        count_pass_elems(c, m);
      }
      HIP_TRY(hipEventRecord(r.ck_hi[k], r.stream));
    }
    // chunk k on the wire stream, once every local rank's pass has written it
    for (size_t i = 0; i < nr; ++i) {
      Rank& r = c->ranks[i];
      HIP_TRY(hipSetDevice(r.dev));
      for (Rank& s : c->ranks) HIP_TRY(hipStreamWaitEvent(r.xstream, s.ck_hi[k], 0));
      chunk_wave(P, C, geo[i], r.recv_displs.data(), k, w[i]);
    }
    LSB_TRY(wire_step(c, w, Y, seg, &Rank::xstream));
    for (Rank& r : c->ranks) {
      HIP_TRY(hipSetDevice(r.dev));
      HIP_TRY(hipEventRecord(r.ck_wire[k], r.xstream));
    }
  }
  // 4. placements, chunk k's once it has arrived (the last exchange's, which
  //    write X, also once every chunk pass has read X)
  for (size_t i = 0; i < nr; ++i) {
    Rank& r = c->ranks[i];
    HIP_TRY(hipSetDevice(r.dev));
    r.A = Y[i];  // the records, ordered by the digit chunk by chunk (my own segment's source)
    r.B = X[i];  // the placement's destination
    if (!r.gather_next) HIP_TRY(hipStreamWaitEvent(r.pstream, r.ck_hi[C - 1], 0));
    for (int k = 0; k < C; ++k) {
      HIP_TRY(hipStreamWaitEvent(r.pstream, r.ck_wire[k], 0));
      chunk_wave(P, C, geo[i], r.recv_displs.data(), k, w[i]);
      LSB_TRY(place_wave(c, r, shift, w[i], Y[i]));
    }
    HIP_TRY(hipEventRecord(r.xdone, r.xstream));
    HIP_TRY(hipStreamWaitEvent(r.stream, r.xdone, 0));
    LSB_TRY(join_place_timed(c, r));
    end_placement(r);
  }
  // Every rank's copies out of Y must be done before any rank's next pass
  // rewrites it (loopback; RCCL ranks wait for their own wire stream above).
  if (c->mode == Mode::kLoopback)
    for (Rank& r : c->ranks) {
      HIP_TRY(hipSetDevice(r.dev));
      HIP_TRY(hipStreamSynchronize(r.stream));
    }
  return LSB_OK;
}

// ---- per-digit exchange with single-read local passes ----------------------
// lsb_sort of the per-digit exchange forms (radix_bits 8 / 16, P > 1): the
// reference's pass loop (mpi/mpi_lsbsort.cpp:580-585), each exchange digit's
// localShuffle (:213-247) as one or two k_onesweep passes instead of count +
// scan + scatter.  One k_subhist read per sort gives the first byte's
// sub-array histogram and the key span; after that every histogram is
// counted by whatever writes the records: the previous local pass, or the
// exchange's k_place launches (their output is the next pass's input).  The
// last local pass of an exchange digit hands the exchange its counts: the
// 256 totals, or (16-bit digits) the 65536 counts, from the high-byte pass.
bool exchange_onesweep_applies(const lsb_ctx* c) {
  if (!c->onesweep || !exchanging(c) || c->bits == 64) return false;
  for (const Rank& r : c->ranks)
    if (r.here > lsb::kOnesweepMaxElems) return false;
  return true;
}

// One local pass of rank r on the byte at `shift`; next >= 0: also count the
// byte at `next` over the output (the next local pass follows directly).
int local_pass_os(lsb_ctx* c, Rank& r, int shift, int next, lsb::OnesweepExtra extra) {
  HIP_TRY(hipSetDevice(r.dev));
  // A gathered pass always takes the whole stage: the split stage's gathered
  // instances spill (168 VGPRs at 3 workgroups per CU: 160-236 B per lane),
  // while the whole stage's fit (128 VGPRs, no or 12 B of spill) and cost
  // skewed keys ~1 % per pass against the split (58.53 vs 59.24 ms per Zipf
  // sort, profiles/ab/r02_ab28_zipf_stage.log) -- far less than the placement
  // the gathered pass saves (32 B per record).
  extra.halves = r.gather_pending ? 1 : r.os_halves;
  r.starts_fused = false;
  const int64_t m = r.here;
  if (m == 0) {
    if (extra.totals) HIP_TRY(hipMemsetAsync(extra.totals, 0, sizeof(uint64_t) * lsb::kBuckets, r.stream));
    if (extra.count16) HIP_TRY(hipMemsetAsync(extra.count16, 0, sizeof(uint64_t) * 65536, r.stream));
    r.os_valid = -1;
    return LSB_OK;
  }
  uint32_t* hist[2] = {r.os_hist, r.os_hist + lsb::kOnesweepSubs * lsb::kBuckets};
  if (r.gather_pending) {  // the exchange's count-only placement counted this byte
    if (r.os_valid != shift) {
      r.gather_pending = false;
      return fail(LSB_ERR_STATE, "local_pass_os", "gathered pass without its count");
    }
    extra.gather = &r.gsrc;
  } else if (r.os_valid != shift) {  // nothing counted this byte over A: read it
    Timer t(c, &r, LSB_K_UPSWEEP);
    HIP_TRY(lsb::launch_subhist(r.A, m, shift, r.os_grid, hist[r.os_cur], nullptr, r.stream));
  }
  const int rc = onesweep_launch(c, r, shift, next, hist[r.os_cur], hist[r.os_cur ^ 1], extra);
  r.gather_pending = false;
  LSB_TRY(rc);
  if (next >= 0) {
    r.os_cur ^= 1;
    r.os_valid = next;
  } else {
    r.os_valid = -1;
  }
  return LSB_OK;
}


int sort_exchange_onesweep(lsb_ctx* c) {
  const int D = 64 / c->bits, subs = c->bits / lsb::kDigitBits;
  c->pass_cursor = 0;
  c->cur_pass = 0;
  for (Rank& r : c->ranks) {
    HIP_TRY(hipSetDevice(r.dev));
    LSB_TRY(onesweep_ensure(r));
    HIP_TRY(hipMemsetAsync(r.span, 0, 2 * sizeof(uint64_t), r.stream));
    r.os_cur = 0;
    r.os_valid = -1;
    if (r.here > 0) {
      Timer t(c, &r, LSB_K_UPSWEEP);
      HIP_TRY(lsb::launch_subhist(r.A, r.here, 0, r.os_grid, r.os_hist,
                                  c->skip_constant ? r.span : nullptr, r.stream));
      r.os_valid = 0;
    }
    LSB_TRY(queue_halves(c, r, r.os_hist));
  }
  uint64_t varying = ~0ull;
  if (c->skip_constant) {
    uint64_t kor = 0, knor = 0;
    LSB_TRY(gather_span(c, &kor, &knor));
    varying = kor & knor;
  }
  c->last_varying = varying;
  // Local passes in order; an exchange follows the last one of each digit.
  // A digit on which every key agrees needs neither (its stable pass and its
  // (digit, rank) exchange order are the identity), nor does a constant byte
  // its local pass.
  struct Step {
    int shift, digit;
    bool exch;
  };
  std::vector<Step> steps;
  const uint64_t dmask = (1ull << c->bits) - 1;
  for (int d = 0; d < D; ++d) {
    if (((varying >> (d * c->bits)) & dmask) == 0) continue;
    for (int sub = 0; sub < subs; ++sub) {
      const int shift = d * c->bits + sub * lsb::kDigitBits;
      if (((varying >> shift) & (lsb::kBuckets - 1)) != 0) steps.push_back({shift, d, false});
    }
    steps.back().exch = true;
  }
  // The stage split is decided from the first byte that is sorted on: when
  // byte 0 is constant, that byte is counted now (its pass reads the
  // histogram instead of counting it again).  gather_span syncs only the
  // streams it reads from: each rank syncs in choose_halves.
  for (Rank& r : c->ranks) {
    HIP_TRY(hipSetDevice(r.dev));
    if (!steps.empty() && steps[0].shift != 0 && r.here > 0) {
      {
        Timer t(c, &r, LSB_K_UPSWEEP);
        HIP_TRY(lsb::launch_subhist(r.A, r.here, steps[0].shift, r.os_grid, r.os_hist, nullptr,
                                    r.stream));
      }
      r.os_cur = 0;
      r.os_valid = steps[0].shift;
      LSB_TRY(queue_halves(c, r, r.os_hist));
    }
    LSB_TRY(choose_halves(c, r, false));
  }
  std::vector<const uint32_t*> lo_hist(c->ranks.size(), nullptr);
  for (size_t i = 0; i < steps.size(); ++i) {
    const Step& st = steps[i];
    const int after = i + 1 < steps.size() ? steps[i + 1].shift : -1;
    // LSB_OPT_EXCHANGE_CHUNKS: the low byte's pass counts nothing for the next
    // (exchange_chunked's read does), and the high byte's pass runs chunk by
    // chunk inside exchange_chunked.
    const bool chunked = chunked_applies(c, varying, st.digit);
    if (chunked && st.exch) {
      begin_pass(c, st.shift);
    } else {
      // 16-bit digit: its high-byte pass counts the 65536 digits (a constant
      // high byte leaves the count to digit_counts' read of A).
      const bool c16 = c->bits == 16 && st.exch && st.shift == st.digit * 16 + lsb::kDigitBits;
      begin_pass(c, st.shift);
      for (size_t k = 0; k < c->ranks.size(); ++k) {
        Rank& r = c->ranks[k];
        lsb::OnesweepExtra x;
        if (st.exch && c->bits == 8) x.totals = r.totals;
        if (c16) x.count16 = r.totals16;
        r.counts_ready = c16;
        LSB_TRY(local_pass_os(c, r, st.shift, st.exch || chunked ? -1 : after, x));
        // the pass's input histogram (os_cur stays: next = -1): the chunk bounds
        lo_hist[k] = r.os_hist + (size_t)r.os_cur * lsb::kOnesweepSubs * lsb::kBuckets;
      }
    }
    ++c->last_local_passes;
    if (!st.exch) continue;
    for (Rank& r : c->ranks) {
      r.place_next = c->peer || r.here == 0 ? -1 : after;
      // Skewed keys too: their gathered pass takes the whole stage (local_pass_os).
      r.gather_next = c->gather && r.place_next >= 0;
      r.place_hist = nullptr;
      if (r.place_next >= 0) {
        r.place_hist = r.os_hist + (size_t)(r.os_cur ^ 1) * lsb::kOnesweepSubs * lsb::kBuckets;
        HIP_TRY(hipSetDevice(r.dev));
        HIP_TRY(hipMemsetAsync(r.place_hist, 0, sizeof(uint32_t) * lsb::kOnesweepSubs * lsb::kBuckets,
                               r.stream));
      }
    }
    ++c->last_exchanges;
    const int rc = chunked ? exchange_chunked(c, st.digit, lo_hist) : exchange_digit(c, st.digit);
    for (Rank& r : c->ranks) {
      if (rc == LSB_OK && r.place_next >= 0) {
        r.os_cur ^= 1;
        r.os_valid = r.place_next;
      } else {
        r.os_valid = -1;
      }
      r.place_next = -1;
      r.place_hist = nullptr;
      r.counts_ready = false;
      r.gather_next = false;
      if (rc != LSB_OK) r.gather_pending = false;
    }
    LSB_TRY(rc);
  }
  // The look-back's give-up word, read by lsb_sync.
  for (Rank& r : c->ranks) {
    if (r.here == 0) continue;
    HIP_TRY(hipSetDevice(r.dev));
    HIP_TRY(hipMemcpyAsync(r.os_err_h, r.os_ctr + lsb::kOnesweepSubs, sizeof(uint32_t),
                           hipMemcpyDeviceToHost, r.stream));
  }
  return LSB_OK;
}

}  // namespace lsb_rt
