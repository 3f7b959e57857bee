// Host-only geometry of the exchanges: the checked plan, and the waves (one
// all-to-all-v step as one rank sees it) of the sliced, the chunked and the
// whole-key exchange.  Pure functions over plain arrays and vectors, no device
// or collective header: a host program without a device can call them
// (tools/host_asan.cpp does).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lsb.h"

namespace lsb_rt {

// Records `what: detail` for lsb_strerror and returns `code` (lsb_context.cpp).
int fail(int code, const char* what, const char* detail);

// Part j of a per-digit exchange segment of n records cut into `slices`
// halving parts: n/2, n/4, ..., and the last two n / 2^(slices-1) each.  A
// slice is placed (or counted) while the next one is on the wire, so what
// runs after the wire goes quiet is the last slice's placement: 1/16 of the
// records at 5 slices where equal slices leave 1/4 at 4.
// Sender and receiver cut a segment alike (send_counts[q] at s equals
// recv_counts[s] at q).
inline int64_t slice_part(int64_t n, int j, int slices) {
  if (j >= slices) return n;
  return j >= 63 ? n : n - (n >> j);
}

// The plan every transport moves records by: the 2P counts the device plan
// sent back (send, then recv) become counts and displacements, or
// LSB_ERR_STATE unless every count lies in [0, here] and both sums are `here`
// (the reference asserts the sums before every MPI_Alltoallv,
// mpi/mpi_lsbsort.cpp:300,312).  A count is checked against what is left of
// `here` before it is added, so no sum can overflow.
inline int checked_plan(const int64_t* counts, int P, int64_t here, int64_t* sc, int64_t* sd,
                        int64_t* rc, int64_t* rd) {
  int64_t ss = 0, rs = 0;
  for (int q = 0; q < P; ++q) {
    sc[q] = counts[q];
    rc[q] = counts[P + q];
    if (sc[q] < 0 || sc[q] > here - ss || rc[q] < 0 || rc[q] > here - rs)
      return fail(LSB_ERR_STATE, "exchange plan", "count out of range");
    sd[q] = ss;
    rd[q] = rs;
    ss += sc[q];
    rs += rc[q];
  }
  if (ss != here || rs != here) return fail(LSB_ERR_STATE, "exchange plan", "counts do not add up to the block");
  return LSB_OK;
}

// One step of an all-to-all-v as one rank sees it, in records: to peer q go
// scnt[q] records at soff[q] of the source buffer, from peer q come rcnt[q]
// records to roff[q] of R.
struct Wave {
  std::vector<int64_t> soff, scnt, roff, rcnt;
  void resize(int P) {
    for (std::vector<int64_t>* v : {&soff, &scnt, &roff, &rcnt}) v->resize(P);
  }
};

// Slice j of a plan: part j of every peer segment.
inline void slice_wave(int P, const int64_t* sc, const int64_t* sd, const int64_t* rc, const int64_t* rd, int j,
                       int slices, Wave& w) {
  w.resize(P);
  for (int q = 0; q < P; ++q) {
    const int64_t slo = slice_part(sc[q], j, slices), rlo = slice_part(rc[q], j, slices);
    w.soff[q] = sd[q] + slo;
    w.scnt[q] = slice_part(sc[q], j + 1, slices) - slo;
    w.roff[q] = rd[q] + rlo;
    w.rcnt[q] = slice_part(rc[q], j + 1, slices) - rlo;
  }
}

// One rank's chunk geometry (the per-digit exchange in chunks) after the plan.
struct ChunkGeom {
  std::vector<int64_t> lo;     // [C + 1] chunk bounds in A and B
  std::vector<int64_t> send;   // [q * C + k] my records of chunk k for owner q
  std::vector<int64_t> recv;   // [s * C + k] source s's records of chunk k for me
  std::vector<int64_t> sdisp;  // [q * C + k] where owner q's share starts inside chunk k
  std::vector<int64_t> rpre;   // [s * C + k] where chunk k starts inside source s's range of R
};

// From the low byte's sub-array histogram lo_hist[x * buckets + l] (x < subs;
// read only when here > 0), the plan's per-chunk counts ck (send [q * C + k],
// then recv [s * C + k]) and its totals.  LSB_ERR_STATE unless the chunks
// cover the block, each chunk's sends fill it, and the per-chunk counts (each
// in [0, here]) add up to the plan's.
inline int chunk_geom(int P, int C, int64_t here, const uint32_t* lo_hist, int buckets, int subs,
                      const int64_t* ck, const int64_t* send_counts, const int64_t* recv_counts, ChunkGeom& g) {
  const int lw = buckets / C;
  g.lo.assign(C + 1, 0);
  if (here > 0) {
    int64_t acc = 0;
    for (int l = 0; l < buckets; ++l) {
      if (l % lw == 0) g.lo[l / lw] = acc;
      for (int x = 0; x < subs; ++x) acc += lo_hist[x * buckets + l];
    }
    g.lo[C] = acc;
    if (acc != here) return fail(LSB_ERR_STATE, "exchange_chunked", "chunk bounds do not cover the block");
  }
  const size_t PC = (size_t)P * C;
  g.send.assign(ck, ck + PC);
  g.recv.assign(ck + PC, ck + 2 * PC);
  g.sdisp.assign(PC, 0);
  g.rpre.assign(PC, 0);
  for (size_t i = 0; i < PC; ++i)
    if (g.send[i] < 0 || g.send[i] > here || g.recv[i] < 0 || g.recv[i] > here)
      return fail(LSB_ERR_STATE, "exchange_chunked", "chunk count out of range");
  for (int k = 0; k < C; ++k) {
    int64_t a = 0;
    for (int q = 0; q < P; ++q) {
      g.sdisp[(size_t)q * C + k] = a;
      a += g.send[(size_t)q * C + k];
    }
    if (a != g.lo[k + 1] - g.lo[k]) return fail(LSB_ERR_STATE, "exchange_chunked", "chunk send counts");
  }
  for (int q = 0; q < P; ++q) {
    int64_t a = 0, sa = 0;
    for (int k = 0; k < C; ++k) {
      g.rpre[(size_t)q * C + k] = a;
      a += g.recv[(size_t)q * C + k];
      sa += g.send[(size_t)q * C + k];
    }
    if (a != recv_counts[q] || sa != send_counts[q])
      return fail(LSB_ERR_STATE, "exchange_chunked", "chunk counts do not add up");
  }
  return LSB_OK;
}

// Chunk k of a ChunkGeom: every owner's share of chunk k (source buffer: the
// chunk passes' output), chunk k's place inside every source's range of R
// (rd: the plan's receive displacements).
inline void chunk_wave(int P, int C, const ChunkGeom& g, const int64_t* rd, int k, Wave& w) {
  w.resize(P);
  for (int q = 0; q < P; ++q) {
    const size_t i = (size_t)q * C + k;
    w.soff[q] = g.lo[k] + g.sdisp[i];
    w.scnt[q] = g.send[i];
    w.roff[q] = rd[q] + g.rpre[i];
    w.rcnt[q] = g.recv[i];
  }
}

// The largest of the C pieces per peer a rank sends or receives (send, recv:
// [q * C + k]); its own (q == skip) do not count.
inline int64_t max_segment(const int64_t* send, const int64_t* recv, int P, int C, int skip) {
  int64_t m = 0;
  for (int i = 0; i < P * C; ++i)
    if (i / C != skip) m = std::max(m, std::max(send[i], recv[i]));
  return m;
}

// ---- whole-key exchange (lsb_wholekey.cpp) ------------------------------------

// Cut positions of the exchange: owner q's block [q * per, q * per + here_q)
// is cut into S slices (sub-blocks) at q * per + part(here_q, j, S); cut k =
// q * S + j, plus k = P * S at n.  Every cut strictly inside (0, n) is a
// target of the splitter search.  S = 1 gives the owner boundaries q * per.
// Slices let the owner merge slice j while slice j + 1 is on the wire.
struct MergeGeom {
  int S = 1;
  std::vector<int64_t> pos;   // [P * S + 1] global cut positions, nondecreasing
  std::vector<int> target;    // cut indices k with 0 < pos[k] < n (splitter targets)
};
MergeGeom merge_geometry(int64_t n, int P, int slices);
int merge_cuts(int64_t n, int P, const MergeGeom& g, const uint64_t* fin, std::vector<int64_t>& cut);
int merge_owner_counts(int64_t n, int P, int me, const MergeGeom& g, const std::vector<int64_t>& cut,
                       int64_t* sc, int64_t* sd, int64_t* rc, int64_t* rd);

// Owner slice j of the whole-key cuts (mcut[s * (P * S + 1) + k], every
// source's) as rank `me` sees it: to owner q goes my range between its cuts j
// and j + 1; source s's records of my slice j lie in R in source order from
// the slice's output range [lo, hi) of my block on.
inline void owner_wave(int P, int me, int64_t per, const MergeGeom& g, const std::vector<int64_t>& mcut, int j,
                       Wave& w, int64_t* lo, int64_t* hi) {
  const size_t K1 = g.pos.size(), k = (size_t)me * g.S + j;
  *lo = std::max<int64_t>(0, g.pos[k] - me * per);
  *hi = std::max(*lo, g.pos[k + 1] - me * per);
  w.resize(P);
  int64_t off = *lo;
  for (int q = 0; q < P; ++q) {
    const size_t kq = (size_t)q * g.S + j;
    w.soff[q] = mcut[me * K1 + kq];
    w.scnt[q] = mcut[me * K1 + kq + 1] - w.soff[q];
    w.roff[q] = off;
    w.rcnt[q] = mcut[q * K1 + k + 1] - mcut[q * K1 + k];
    off += w.rcnt[q];
  }
}

}  // namespace lsb_rt
