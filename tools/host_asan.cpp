// ASan/UBSan driver for the C ABI's host code (sanitizers on host
// code).  `make -C distributed-lsb_amd asan` links it against an ASan/UBSan
// build of the runtime units (csrc/lsb_*.cpp; device code unchanged) and runs it without a GPU:
//   - lsb_plan_exchange on random, skewed, empty and n < P count matrices:
//     conservation (sum send = sum recv = here), displacement prefix sums,
//     every live placement offset inside [0, here);
//   - the exchanges' host geometry (csrc/lsb_xgeom.h) on the same matrices:
//     the checked plan accepts every host plan and refuses corrupted ones;
//     the slice, chunk and whole-key waves tile every send and receive range
//     once, and sender and receiver agree at every step;
//   - every argument check that returns before a device call;
//   - the key forms of caller-owned columns (lsb_key_encode / lsb_key_decode,
//     csrc/lsb_keyform.h): round trip, order and zero upper words over every
//     type and flag, specials included; lsb_load_columns / lsb_store_columns
//     with a null context and bad arguments;
//   - the planner of the runs of equal keys (lsb_plan_runs) against a count
//     over the whole array: random, single-run, all-distinct and n < P
//     arrays; corrupted summaries are refused; lsb_count_runs /
//     lsb_store_runs with a null context and bad arguments;
//   - the planner of the reductions over the runs' values
//     (lsb_plan_run_tails) on the same partitions against a walk over the
//     whole array; its refusals and identities; lsb_plan_reduce /
//     lsb_store_reduce and lsb_label_runs with a null context;
//   - the planner of the select (lsb_plan_select) for every k of random
//     partitions against the stable sort of the whole array; its refusals;
//     lsb_select / lsb_store_select with a null context and bad arguments;
//   - lsb_search with a null context, with a bad mode and with every argument
//     bad: refused before the columns are looked at; lsb_lookup,
//     lsb_join_count and lsb_store_join alike;
//   - k_onesweep's tile geometry where passes of different tile sizes meet
//     (csrc/lsb_ostile.h): the look-back rows' fill decision replayed over
//     random launch sequences (no launch can read a row of its own parity
//     that it did not write), the bound under which a large tile applies
//     against a search over every sub-array, and a run's cut against the
//     sub-array of each of its slots, for every pair of tile sizes;
//   - lsb_create / lsb_create_rank_ops with no usable device: the failure
//     path tears down a half-built context (no leak, no double free).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "lsb.h"
#include "lsb_keyform.h"
#include "lsb_ostile.h"
#include "lsb_xgeom.h"

static int fails = 0;
#define CHECK(c, what)                                    \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); \
      ++fails;                                            \
    }                                                     \
  } while (0)

typedef std::vector<std::vector<int64_t>> PerRank;  // [rank][peer]
static void checked_plan_case(int P, int64_t here, const std::vector<int64_t>& sc, const std::vector<int64_t>& sd,
                              const std::vector<int64_t>& rc, const std::vector<int64_t>& rd);
static void slice_wave_case(int P, const PerRank& sc, const PerRank& sd, const PerRank& rc, const PerRank& rd);

static void plan_case(std::mt19937_64& rng, int64_t n, int P, int nb, bool skew) {
  std::vector<int64_t> hist((size_t)P * nb, 0);
  for (int s = 0; s < P; ++s) {
    int64_t h = lsb_here(n, P, s);
    for (int64_t i = 0; i < h; ++i) {
      int b = skew ? (int)((rng() % 7 == 0) ? rng() % nb : 3) : (int)(rng() % nb);
      ++hist[(size_t)s * nb + b];
    }
  }
  // every rank's plan
  std::vector<std::vector<int64_t>> sc(P), sd(P), rc(P), rd(P), place(P);
  for (int me = 0; me < P; ++me) {
    sc[me].resize(P), sd[me].resize(P), rc[me].resize(P), rd[me].resize(P);
    place[me].assign((size_t)P * nb, -7);
    int rcode = lsb_plan_exchange(n, P, me, nb, hist.data(), sc[me].data(), sd[me].data(),
                                  rc[me].data(), rd[me].data(), place[me].data());
    CHECK(rcode == LSB_OK, "plan ok");
    int64_t ss = 0, rs = 0;
    for (int q = 0; q < P; ++q) {
      CHECK(sd[me][q] == ss && rd[me][q] == rs, "displacements are prefix sums");
      ss += sc[me][q];
      rs += rc[me][q];
    }
    CHECK(ss == lsb_here(n, P, me), "send total = here");
    CHECK(rs == lsb_here(n, P, me), "recv total = here");
    checked_plan_case(P, lsb_here(n, P, me), sc[me], sd[me], rc[me], rd[me]);
  }
  slice_wave_case(P, sc, sd, rc, rd);
  // Receiver me: record k of the segment from s is record sd[s][me] + (k - rd[me][s])
  // of s's bucket-ordered buffer; its slot place[me][s][bucket] + k must
  // cover [0, here) exactly once.
  for (int me = 0; me < P; ++me) {
    const int64_t here = lsb_here(n, P, me);
    std::vector<char> seen((size_t)here + 1, 0);
    for (int s = 0; s < P; ++s) {
      CHECK(sc[s][me] == rc[me][s], "send/recv counts agree");
      int b = 0;
      int64_t bend = hist[(size_t)s * nb];  // end of bucket b in s's buffer
      for (int64_t i = 0; i < rc[me][s]; ++i) {
        const int64_t pos = sd[s][me] + i;
        while (b < nb - 1 && pos >= bend) bend += hist[(size_t)s * nb + ++b];
        const int64_t k = rd[me][s] + i;
        const int64_t slot = place[me][(size_t)s * nb + b] + k;
        const bool in = slot >= 0 && slot < here;
        CHECK(in, "slot inside here-part");
        if (in) {
          CHECK(!seen[(size_t)slot], "slot used once");
          seen[(size_t)slot] = 1;
        }
      }
    }
  }
}

// The exchange's checked plan (lsb_xgeom.h) on rank me's host plan: accepted,
// same displacements; five corruptions of it are refused.
static void checked_plan_case(int P, int64_t here, const std::vector<int64_t>& sc, const std::vector<int64_t>& sd,
                              const std::vector<int64_t>& rc, const std::vector<int64_t>& rd) {
  std::vector<int64_t> good(sc);
  good.insert(good.end(), rc.begin(), rc.end());
  std::vector<int64_t> o[4];
  for (auto& v : o) v.assign(P, -7);
  auto run = [&](const std::vector<int64_t>& counts) {
    return lsb_rt::checked_plan(counts.data(), P, here, o[0].data(), o[1].data(), o[2].data(), o[3].data());
  };
  CHECK(run(good) == LSB_OK, "checked plan accepts the host plan");
  CHECK(o[0] == sc && o[1] == sd && o[2] == rc && o[3] == rd, "checked plan = host plan");
  std::vector<int64_t> bad(good);
  bad[0] = -1;
  CHECK(run(bad) == LSB_ERR_STATE, "negative count");
  bad = good;
  bad[0] += 1;
  CHECK(run(bad) == LSB_ERR_STATE, "send total = here + 1");
  bad = good;
  bad[2 * P - 1] = INT64_MAX;
  CHECK(run(bad) == LSB_ERR_STATE, "count = INT64_MAX");
  bad[0] = INT64_MAX;
  CHECK(run(bad) == LSB_ERR_STATE, "two counts = INT64_MAX");
  if (here > 0) {
    bad = good;
    for (int q = 0; q < P; ++q)
      if (bad[P + q] > 0) {
        bad[P + q] -= 1;
        break;
      }
    CHECK(run(bad) == LSB_ERR_STATE, "recv total = here - 1");
    bad.assign(2 * P, 0);
    CHECK(run(bad) == LSB_ERR_STATE, "all counts zero");
  }
}

// waves[r][j]: rank r's wave of step j.  Over the steps, in order, the waves
// tile every pair's send range [sd, +sc) and receive range [rd, +rc) exactly
// once, and at every step the sender's count is the receiver's.
typedef std::vector<std::vector<lsb_rt::Wave>> Waves;
static void waves_tile(int P, const Waves& waves, const PerRank& sc, const PerRank& sd, const PerRank& rc,
                       const PerRank& rd) {
  for (int s = 0; s < P; ++s)
    for (int q = 0; q < P; ++q) {
      int64_t scur = sd[s][q], rcur = rd[q][s];
      for (size_t j = 0; j < waves[s].size(); ++j) {
        const lsb_rt::Wave &ws = waves[s][j], &wq = waves[q][j];
        CHECK(ws.scnt[q] >= 0 && ws.soff[q] == scur, "send parts in order");
        CHECK(wq.rcnt[s] >= 0 && wq.roff[s] == rcur, "recv parts in order");
        CHECK(ws.scnt[q] == wq.rcnt[s], "sender and receiver agree");
        scur += ws.scnt[q];
        rcur += wq.rcnt[s];
      }
      CHECK(scur == sd[s][q] + sc[s][q], "send range covered");
      CHECK(rcur == rd[q][s] + rc[q][s], "recv range covered");
    }
}

static void slice_wave_case(int P, const PerRank& sc, const PerRank& sd, const PerRank& rc, const PerRank& rd) {
  for (int slices : {1, 2, 5, 8, 65}) {  // 65: slice_part's j >= 63 guard
    Waves waves(P, std::vector<lsb_rt::Wave>(slices));
    for (int r = 0; r < P; ++r)
      for (int j = 0; j < slices; ++j)
        lsb_rt::slice_wave(P, sc[r].data(), sd[r].data(), rc[r].data(), rd[r].data(), j, slices, waves[r][j]);
    waves_tile(P, waves, sc, sd, rc, rd);
  }
}

// exchange_chunked's geometry: random records of source s for owner q in
// chunk k (empty chunks and empty peers among them; every rank sends as many
// as it receives), the low byte's histogram and the plan totals they imply.
static void chunk_case(std::mt19937_64& rng, int P, int C) {
  const int buckets = 256, subs = 8, lw = buckets / C;
  std::vector<int64_t> m((size_t)P * P * C, 0);  // [s][q][k]
  for (int s = 0; s < P; ++s)
    for (int q = s; q < P; ++q)
      for (int k = 0; k < C; ++k) {
        const bool empty = rng() % 4 == 0 || (s + q) % 3 == 2 || (P > 1 && k == 1);
        const int64_t v = empty ? 0 : (int64_t)(rng() % 50);
        m[((size_t)s * P + q) * C + k] += v;
        if (q != s) m[((size_t)q * P + s) * C + k] += v;
      }
  std::vector<lsb_rt::ChunkGeom> geo(P);
  PerRank ck(P), sc(P), sd(P), rc(P), rd(P);
  std::vector<int64_t> here(P, 0);
  std::vector<std::vector<uint32_t>> lo_hist(P);
  for (int me = 0; me < P; ++me) {
    ck[me].assign((size_t)2 * P * C, 0);
    sc[me].assign(P, 0), sd[me].assign(P, 0), rc[me].assign(P, 0), rd[me].assign(P, 0);
    lo_hist[me].assign((size_t)subs * buckets, 0);
    for (int q = 0; q < P; ++q)
      for (int k = 0; k < C; ++k) {
        const int64_t snd = m[((size_t)me * P + q) * C + k], rcv = m[((size_t)q * P + me) * C + k];
        ck[me][(size_t)q * C + k] = snd;
        ck[me][(size_t)P * C + (size_t)q * C + k] = rcv;
        sc[me][q] += snd;
        rc[me][q] += rcv;
        here[me] += snd;
        for (int64_t i = 0; i < snd; ++i) ++lo_hist[me][(rng() % subs) * buckets + k * lw + rng() % lw];
      }
    for (int q = 1; q < P; ++q) rd[me][q] = rd[me][q - 1] + rc[me][q - 1];
    CHECK(lsb_rt::chunk_geom(P, C, here[me], lo_hist[me].data(), buckets, subs, ck[me].data(), sc[me].data(),
                             rc[me].data(), geo[me]) == LSB_OK, "chunk_geom accepts");
  }
  Waves waves(P, std::vector<lsb_rt::Wave>(C));
  for (int r = 0; r < P; ++r) {
    int64_t cur = 0;  // a rank's sends, chunk by chunk and owner by owner, tile its block
    for (int k = 0; k < C; ++k) {
      lsb_rt::chunk_wave(P, C, geo[r], rd[r].data(), k, waves[r][k]);
      for (int q = 0; q < P; ++q) {
        CHECK(waves[r][k].soff[q] == cur, "chunk sends tile the block");
        cur += waves[r][k].scnt[q];
      }
    }
    CHECK(cur == here[r], "chunk sends cover the block");
  }
  for (int r = 0; r < P; ++r)
    for (int q = 0; q < P; ++q) {
      int64_t sent = 0, rcur = rd[r][q];
      for (int k = 0; k < C; ++k) {
        CHECK(waves[r][k].roff[q] == rcur, "chunk receives tile the source's range");
        CHECK(waves[q][k].scnt[r] == waves[r][k].rcnt[q], "sender and receiver agree");
        rcur += waves[r][k].rcnt[q];
        sent += waves[r][k].scnt[q];
      }
      CHECK(rcur == rd[r][q] + rc[r][q] && sent == sc[r][q], "chunk counts add up to the plan");
    }
  // one count off by one, or negative: refused
  lsb_rt::ChunkGeom g;
  for (int64_t delta : {int64_t(1), int64_t(-1), INT64_MIN}) {
    std::vector<int64_t> bad(ck[0]);
    int64_t& x = bad[rng() % bad.size()];
    x = delta == INT64_MIN ? -5 : x + delta;
    CHECK(lsb_rt::chunk_geom(P, C, here[0], lo_hist[0].data(), buckets, subs, bad.data(), sc[0].data(),
                             rc[0].data(), g) == LSB_ERR_STATE, "chunk_geom refuses a wrong count");
  }
}

// The whole-key exchange's owner slices: P sorted blocks with ties, the cuts
// from the counts a finished splitter search gives.
static void wholekey_case(std::mt19937_64& rng, int64_t n, int P, int slices) {
  using namespace lsb_rt;
  std::vector<std::vector<uint64_t>> blk(P);
  std::vector<uint64_t> all;
  for (int s = 0; s < P; ++s) {
    for (int64_t i = 0; i < lsb_here(n, P, s); ++i) blk[s].push_back(rng() % 40);
    std::sort(blk[s].begin(), blk[s].end());
    all.insert(all.end(), blk[s].begin(), blk[s].end());
  }
  std::sort(all.begin(), all.end());
  const MergeGeom g = merge_geometry(n, P, slices);
  const int Q = (int)g.target.size();
  std::vector<uint64_t> fin((size_t)P * Q * 2 + 1, 0);
  for (int t = 0; t < Q; ++t) {
    const uint64_t key = all[(size_t)g.pos[g.target[t]]];
    for (int s = 0; s < P; ++s) {
      fin[((size_t)s * Q + t) * 2] = std::lower_bound(blk[s].begin(), blk[s].end(), key) - blk[s].begin();
      fin[((size_t)s * Q + t) * 2 + 1] = std::upper_bound(blk[s].begin(), blk[s].end(), key) - blk[s].begin();
    }
  }
  std::vector<int64_t> cut;
  CHECK(merge_cuts(n, P, g, fin.data(), cut) == LSB_OK, "merge_cuts ok");
  PerRank sc(P), sd(P), rc(P), rd(P);
  Waves waves(P, std::vector<Wave>(g.S));
  for (int me = 0; me < P; ++me) {
    sc[me].resize(P), sd[me].resize(P), rc[me].resize(P), rd[me].resize(P);
    CHECK(merge_owner_counts(n, P, me, g, cut, sc[me].data(), sd[me].data(), rc[me].data(), rd[me].data()) == LSB_OK,
          "merge_owner_counts ok");
    int64_t end = 0;
    for (int j = 0; j < g.S; ++j) {
      int64_t lo = -1, hi = -1;
      owner_wave(P, me, lsb_per_rank(n, P), g, cut, j, waves[me][j], &lo, &hi);
      CHECK(lo == end && hi >= lo && waves[me][j].roff[0] == lo, "slices follow each other");
      for (int s = 0; s < P; ++s) lo += waves[me][j].rcnt[s];
      CHECK(lo == hi, "a slice's runs fill its output range");
      end = hi;
    }
    CHECK(end == lsb_here(n, P, me), "slices cover the block");
  }
  // The totals over j are merge_owner_counts'; source s's slice j follows its
  // slice j - 1 in A, but lies after every source's slice j - 1 in R.
  for (int s = 0; s < P; ++s)
    for (int q = 0; q < P; ++q) {
      int64_t scur = sd[s][q], got = 0;
      for (int j = 0; j < g.S; ++j) {
        CHECK(waves[s][j].soff[q] == scur, "send parts in order");
        CHECK(waves[s][j].scnt[q] == waves[q][j].rcnt[s], "sender and receiver agree");
        scur += waves[s][j].scnt[q];
        got += waves[q][j].rcnt[s];
      }
      CHECK(scur == sd[s][q] + sc[s][q] && got == rc[q][s], "owner slices add up to the owner counts");
    }
}

// The key forms: decode(encode(x)) == x, the exported functions equal the
// inline ones the kernels call, 32-bit types keep a zero upper word, and a
// larger encoded key means a later place in the type's own order (descending:
// an earlier one) for the values below, which are listed in ascending order.
static void keyform_case(std::mt19937_64& rng) {
  const uint64_t f64_asc[] = {0xfff8000000000001ull, 0xfff0000000000000ull, 0xc000000000000000ull,
                              0x8000000000000001ull, 0x8000000000000000ull, 0x0000000000000000ull,
                              0x0000000000000001ull, 0x4000000000000000ull, 0x7ff0000000000000ull,
                              0x7ff8000000000001ull};
  const uint64_t f32_asc[] = {0xffc00001u, 0xff800000u, 0xc0000000u, 0x80000001u, 0x80000000u,
                              0x00000000u, 0x00000001u, 0x40000000u, 0x7f800000u, 0x7fc00001u};
  const uint64_t i64_asc[] = {0x8000000000000000ull, 0xffffffffffffffffull, 0, 1, 0x7fffffffffffffffull};
  const uint64_t i32_asc[] = {0x80000000u, 0xffffffffu, 0, 1, 0x7fffffffu};
  const uint64_t u64_asc[] = {0, 1, 0x8000000000000000ull, 0xffffffffffffffffull};
  const uint64_t u32_asc[] = {0, 1, 0x80000000u, 0xffffffffu};
  struct { int kt; const uint64_t* v; int n; } lists[] = {
      {LSB_KEY_U64, u64_asc, 4}, {LSB_KEY_I64, i64_asc, 5}, {LSB_KEY_F64, f64_asc, 10},
      {LSB_KEY_U32, u32_asc, 4}, {LSB_KEY_I32, i32_asc, 5}, {LSB_KEY_F32, f32_asc, 10}};
  for (const auto& l : lists)
    for (int flags : {0, LSB_ORDER_DESCENDING}) {
      const uint64_t mask = l.kt >= LSB_KEY_U32 ? 0xffffffffull : ~0ull;
      for (int i = 0; i < l.n; ++i) {
        const uint64_t e = lsb_key_encode(l.v[i], l.kt, flags);
        CHECK(lsb_key_decode(e, l.kt, flags) == l.v[i], "special round trip");
        CHECK((e & ~mask) == 0, "upper word zero");
        if (i > 0) {
          const uint64_t p = lsb_key_encode(l.v[i - 1], l.kt, flags);
          CHECK(flags ? e < p : e > p, "specials in order");
        }
      }
      for (int i = 0; i < 10000; ++i) {
        const uint64_t x = rng();
        const uint64_t e = lsb_key_encode(x, l.kt, flags);
        CHECK(e == lsb::encode(x, l.kt, flags), "exported encode = inline encode");
        CHECK(lsb_key_decode(e, l.kt, flags) == (x & mask), "random round trip");
        CHECK(lsb::decode(e, l.kt, flags) == (x & mask), "inline round trip");
        CHECK((e & ~mask) == 0, "upper word zero");
      }
    }
  for (int kt : {-1, 6, 1 << 30})
    CHECK(lsb_key_encode(5, kt, 0) == 0 && lsb_key_decode(5, kt, 0) == 0, "unknown type gives 0");
  for (int flags : {2, 3, -1})
    CHECK(lsb_key_encode(5, LSB_KEY_U64, flags) == 0 && lsb_key_decode(5, LSB_KEY_I32, flags) == 0,
          "unknown flag gives 0");
}

// lsb_plan_run_tails on the same partition, with the value of position i a
// hash of i: lead[s] from its definition (garbage where the planner must not
// look), tail[r] against a walk over the whole array from r's end on.  Wrapping
// sums, and the min and max of the signed order: exact in any association.
static uint64_t value_at(int64_t i) {
  uint64_t z = ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint64_t fold_values(int op, int val_type, int64_t lo, int64_t hi) {
  uint64_t acc = op == LSB_REDUCE_SUM ? 0 : op == LSB_REDUCE_MIN ? ~0ull : 0ull;  // the encoding's identity
  for (int64_t i = lo; i < hi; ++i) {
    const uint64_t e = op == LSB_REDUCE_SUM ? value_at(i) : lsb_key_encode(value_at(i), val_type, 0);
    acc = op == LSB_REDUCE_SUM ? acc + e : op == LSB_REDUCE_MIN ? std::min(acc, e) : std::max(acc, e);
  }
  return op == LSB_REDUCE_SUM ? acc : lsb_key_decode(acc, val_type, 0);
}

static void tails_case(const std::vector<uint64_t>& a, int P, const std::vector<uint64_t>& sum) {
  const int64_t n = (int64_t)a.size(), per = lsb_per_rank(n, P);
  const int forms[][2] = {{LSB_REDUCE_SUM, LSB_KEY_U64}, {LSB_REDUCE_MIN, LSB_KEY_I64}, {LSB_REDUCE_MAX, LSB_KEY_F64}};
  for (const auto& f : forms) {
    std::vector<uint64_t> lead(P, 0xDEADull), tail(P, 0xBEEFull);
    for (int s = 0; s < P; ++s) {
      const int64_t lo = s * per;
      if (lsb_here(n, P, s) > 0 && lo > 0 && a[(size_t)lo] == a[(size_t)(lo - 1)])
        lead[s] = fold_values(f[0], f[1], lo, lo + (int64_t)sum[(size_t)s * 4 + 3]);
    }
    CHECK(lsb_plan_run_tails(n, P, sum.data(), f[0], f[1], lead.data(), tail.data()) == LSB_OK, "plan_run_tails ok");
    for (int r = 0; r < P; ++r) {
      const int64_t here = lsb_here(n, P, r);
      int64_t end = r * per + here;
      while (here > 0 && end < n && a[(size_t)end] == a[(size_t)(end - 1)]) ++end;
      CHECK(tail[r] == fold_values(f[0], f[1], r * per + here, here > 0 ? end : r * per + here),
            "tail = the run's records on later ranks");
    }
  }
}

// lsb_plan_runs on the block partition of a[0..n) over P ranks: the summary
// words from their definition, the plan against a walk over the whole array.
static void runs_case(const std::vector<uint64_t>& a, int P) {
  const int64_t n = (int64_t)a.size(), per = lsb_per_rank(n, P);
  std::vector<uint64_t> sum((size_t)P * 4, 0);
  for (int r = 0; r < P; ++r) {
    const int64_t here = lsb_here(n, P, r), lo = r * per;
    if (here == 0) continue;
    uint64_t inner = 0, lead = (uint64_t)here;
    for (int64_t i = here - 1; i >= 1; --i)
      if (a[(size_t)(lo + i)] != a[(size_t)(lo + i - 1)]) {
        ++inner;
        lead = (uint64_t)i;
      }
    sum[(size_t)r * 4 + 0] = a[(size_t)lo];
    sum[(size_t)r * 4 + 1] = a[(size_t)(lo + here - 1)];
    sum[(size_t)r * 4 + 2] = inner;
    sum[(size_t)r * 4 + 3] = lead;
  }
  std::vector<int> head0(P, -7);
  std::vector<int64_t> runs(P, -7), bases(P, -7), ends(P, -7);
  int64_t total = -7;
  CHECK(lsb_plan_runs(n, P, sum.data(), head0.data(), runs.data(), bases.data(), ends.data(), &total) == LSB_OK,
        "plan_runs ok");
  int64_t seen = 0;
  for (int r = 0; r < P; ++r) {
    const int64_t here = lsb_here(n, P, r), lo = r * per;
    int64_t mine = 0;
    for (int64_t i = lo; i < lo + here; ++i) mine += i == 0 || a[(size_t)i] != a[(size_t)(i - 1)];
    int64_t end = lo + here;  // one past the run that holds the rank's last record
    while (here > 0 && end < n && a[(size_t)end] == a[(size_t)(end - 1)]) ++end;
    CHECK(runs[r] == mine, "runs = heads of the rank's positions");
    CHECK(bases[r] == (here ? seen : 0), "bases are the prefix sums");
    CHECK(ends[r] == (here ? end : 0), "ends");
    CHECK(head0[r] == (here > 0 && (lo == 0 || a[(size_t)lo] != a[(size_t)(lo - 1)]) ? 1 : 0), "head0");
    seen += mine;
  }
  CHECK(total == seen, "total");
  tails_case(a, P, sum);
  // every corruption of a non-empty rank's words the header lists is refused
  for (int r = 0; r < P; ++r) {
    const uint64_t here = (uint64_t)lsb_here(n, P, r);
    if (here == 0) continue;
    const uint64_t* w = &sum[(size_t)r * 4];
    const uint64_t bad[][4] = {{w[0], w[1], w[2], 0},          {w[0], w[1], w[2], here + 1},
                               {w[0], w[1], w[2], ~0ull},      {w[0], w[1], here, w[3]},
                               {w[0], w[1], ~0ull, w[3]},      {w[0], w[1], w[2] ? 0ull : 1ull, w[3]},
                               {w[0], w[0] + 1, 0, here}};
    for (const auto& b : bad) {
      std::vector<uint64_t> s2(sum);
      std::copy(b, b + 4, s2.begin() + (size_t)r * 4);
      CHECK(lsb_plan_runs(n, P, s2.data(), head0.data(), runs.data(), bases.data(), ends.data(), &total) ==
                LSB_ERR_INVALID, "corrupted summary refused");
      std::vector<uint64_t> lead(P, 0), tail(P, 0);
      CHECK(lsb_plan_run_tails(n, P, s2.data(), LSB_REDUCE_SUM, LSB_KEY_U64, lead.data(), tail.data()) ==
                LSB_ERR_INVALID, "corrupted summary refused by the tails too");
    }
  }
}

static void runs_cases(std::mt19937_64& rng) {
  for (int it = 0; it < 3000; ++it) {
    const int64_t n = (int64_t)(rng() % 40);
    const int P = 1 + (int)(rng() % 8), d = 1 + (int)(rng() % 5);
    std::vector<uint64_t> a((size_t)n);
    for (auto& x : a) x = rng() % d;
    if (rng() % 2) std::sort(a.begin(), a.end());
    runs_case(a, P);
  }
  for (int P : {1, 2, 3, 8, 64}) {
    runs_case({}, P);
    runs_case(std::vector<uint64_t>(37, 9), P);  // a single run
    std::vector<uint64_t> d(41);
    for (size_t i = 0; i < d.size(); ++i) d[i] = i * 3;
    runs_case(d, P);                              // all distinct
    runs_case({5, 5, 7}, P);                      // n < P for most P
    runs_case({~0ull}, P);
  }
  std::vector<uint64_t> s(8, 0);
  std::vector<int> h(2);
  std::vector<int64_t> o(2);
  int64_t t = 0;
  CHECK(lsb_plan_runs(0, 2, nullptr, h.data(), o.data(), o.data(), o.data(), &t) == LSB_ERR_INVALID, "null summary");
  CHECK(lsb_plan_runs(0, 2, s.data(), nullptr, o.data(), o.data(), o.data(), &t) == LSB_ERR_INVALID, "null head0");
  CHECK(lsb_plan_runs(0, 2, s.data(), h.data(), o.data(), o.data(), o.data(), nullptr) == LSB_ERR_INVALID, "null total");
  CHECK(lsb_plan_runs(-1, 2, s.data(), h.data(), o.data(), o.data(), o.data(), &t) == LSB_ERR_INVALID, "n < 0");
  CHECK(lsb_plan_runs(0, 0, s.data(), h.data(), o.data(), o.data(), o.data(), &t) == LSB_ERR_INVALID, "P = 0");
  CHECK(lsb_plan_runs(0, 65, s.data(), h.data(), o.data(), o.data(), o.data(), &t) == LSB_ERR_INVALID, "P = 65");
  uint64_t col[4] = {0, 1, 2, 3};  // host memory: never reaches a device call with a null context
  t = -5;
  CHECK(lsb_count_runs(nullptr, &t, nullptr, nullptr) == LSB_ERR_INVALID && t == -5, "count_runs: null ctx");
  CHECK(lsb_count_runs(nullptr, nullptr, o.data(), o.data()) == LSB_ERR_INVALID, "count_runs: all null");
  CHECK(lsb_store_runs(nullptr, 0, 4, col, LSB_KEY_U64, 0, (int64_t*)col, (int64_t*)col, col, 8, &t) ==
            LSB_ERR_INVALID && t == -5, "store_runs: null ctx");
  CHECK(lsb_store_runs(nullptr, -1, -1, nullptr, 6, 2, nullptr, (int64_t*)col, nullptr, 3, nullptr) ==
            LSB_ERR_INVALID, "store_runs: all bad");
  // the tails' planner: arguments, and the float sum's identity
  std::vector<uint64_t> ld(2, 0), tl(2, 7);
  s[3] = s[7] = 1;  // n = 2 over 2 ranks: one record each
  CHECK(lsb_plan_run_tails(2, 2, s.data(), LSB_REDUCE_SUM, LSB_KEY_U64, ld.data(), tl.data()) == LSB_OK, "tails ok");
  CHECK(lsb_plan_run_tails(2, 2, nullptr, 0, 0, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: null summary");
  CHECK(lsb_plan_run_tails(2, 2, s.data(), 0, 0, nullptr, tl.data()) == LSB_ERR_INVALID, "tails: null lead");
  CHECK(lsb_plan_run_tails(2, 2, s.data(), 0, 0, ld.data(), nullptr) == LSB_ERR_INVALID, "tails: null tail");
  CHECK(lsb_plan_run_tails(-1, 2, s.data(), 0, 0, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: n < 0");
  CHECK(lsb_plan_run_tails(2, 0, s.data(), 0, 0, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: P = 0");
  CHECK(lsb_plan_run_tails(2, 65, s.data(), 0, 0, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: P = 65");
  CHECK(lsb_plan_run_tails(2, 2, s.data(), 3, 0, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: op 3");
  CHECK(lsb_plan_run_tails(2, 2, s.data(), 0, LSB_KEY_U32, ld.data(), tl.data()) == LSB_ERR_INVALID, "tails: u32");
  const uint64_t neg0 = 0x8000000000000000ull;
  ld[1] = neg0;  // both records carry key 0: rank 1's lead continues rank 0's run
  CHECK(lsb_plan_run_tails(2, 2, s.data(), LSB_REDUCE_SUM, LSB_KEY_F64, ld.data(), tl.data()) == LSB_OK &&
            tl[0] == neg0 && tl[1] == neg0, "a chain of -0.0 sums to -0.0, the identity");
  CHECK(lsb_plan_reduce(nullptr, LSB_REDUCE_SUM, LSB_KEY_U64) == LSB_ERR_INVALID, "plan_reduce: null ctx");
  t = -5;
  CHECK(lsb_store_reduce(nullptr, 0, 4, col, &t) == LSB_ERR_INVALID && t == -5, "store_reduce: null ctx");
  CHECK(lsb_store_reduce(nullptr, -1, -1, nullptr, nullptr) == LSB_ERR_INVALID, "store_reduce: all bad");
  CHECK(lsb_label_runs(nullptr, LSB_LABEL_KEEP) == LSB_ERR_INVALID, "label_runs: null ctx");
  CHECK(lsb_label_runs(nullptr, 2) == LSB_ERR_INVALID, "label_runs: null ctx, unknown mode");
}

// lsb_plan_select on the block partition of a[0..n) over P ranks for every k:
// the counts from their definition, take against the first k + 1 positions of
// the stable sort counted per rank.
static void select_cases(std::mt19937_64& rng) {
  for (int it = 0; it < 1500; ++it) {
    const int64_t n = 1 + (int64_t)(rng() % 40);
    const int P = 1 + (int)(rng() % 8), d = 1 + (int)(rng() % 5);
    const int64_t per = lsb_per_rank(n, P);
    std::vector<uint64_t> a((size_t)n);
    for (auto& x : a) x = rng() % d;
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return a[(size_t)x] < a[(size_t)y]; });
    for (int64_t k = 0; k < n; ++k) {
      const uint64_t pivot = a[(size_t)order[(size_t)k]];
      std::vector<int64_t> below(P, 0), equal(P, 0), want(P, 0), take(P, -7), bases(P, -7);
      for (int64_t i = 0; i < n; ++i) {
        below[(size_t)(i / per)] += a[(size_t)i] < pivot;
        equal[(size_t)(i / per)] += a[(size_t)i] == pivot;
      }
      for (int64_t j = 0; j <= k; ++j) ++want[(size_t)(order[(size_t)j] / per)];
      CHECK(lsb_plan_select(n, P, k + 1, below.data(), equal.data(), take.data(), bases.data()) == LSB_OK,
            "plan_select ok");
      int64_t acc = 0;
      for (int r = 0; r < P; ++r) {
        CHECK(take[r] == want[r], "take = the rank's share of the first k + 1");
        CHECK(bases[r] == acc, "bases are the prefix sums");
        acc += take[r];
      }
      std::vector<int64_t> bad(below);
      bad[rng() % P] = -1;
      CHECK(lsb_plan_select(n, P, k + 1, bad.data(), equal.data(), take.data(), bases.data()) == LSB_ERR_INVALID,
            "negative count refused");
      bad = equal;
      bad[0] = lsb_here(n, P, 0) - below[0] + 1;
      CHECK(lsb_plan_select(n, P, k + 1, below.data(), bad.data(), take.data(), bases.data()) == LSB_ERR_INVALID,
            "more keys than the rank holds refused");
    }
  }
  std::vector<int64_t> b(2, 0), e(2, 1), o(2);
  CHECK(lsb_plan_select(2, 2, 1, b.data(), e.data(), o.data(), o.data()) == LSB_OK, "plan_select: first of two");
  CHECK(lsb_plan_select(2, 2, 0, b.data(), e.data(), o.data(), o.data()) == LSB_ERR_INVALID, "plan_select: count 0");
  CHECK(lsb_plan_select(2, 2, 3, b.data(), e.data(), o.data(), o.data()) == LSB_ERR_INVALID, "plan_select: count 3");
  CHECK(lsb_plan_select(2, 2, 1, nullptr, e.data(), o.data(), o.data()) == LSB_ERR_INVALID, "plan_select: null below");
  CHECK(lsb_plan_select(2, 2, 1, b.data(), e.data(), nullptr, o.data()) == LSB_ERR_INVALID, "plan_select: null take");
  CHECK(lsb_plan_select(-1, 2, 1, b.data(), e.data(), o.data(), o.data()) == LSB_ERR_INVALID, "plan_select: n < 0");
  CHECK(lsb_plan_select(2, 65, 1, b.data(), e.data(), o.data(), o.data()) == LSB_ERR_INVALID, "plan_select: P = 65");
  uint64_t col[4] = {0, 1, 2, 3}, key = 5;
  int64_t t = -5;
  CHECK(lsb_select(nullptr, 0, &key, &t, &t, o.data(), o.data()) == LSB_ERR_INVALID && key == 5 && t == -5,
        "select: null ctx");
  CHECK(lsb_store_select(nullptr, 0, 4, col, LSB_KEY_U64, 0, col, 8, &t) == LSB_ERR_INVALID && t == -5,
        "store_select: null ctx");
  CHECK(lsb_store_select(nullptr, -1, -1, nullptr, 6, 2, nullptr, 3, nullptr) == LSB_ERR_INVALID,
        "store_select: all bad");
  CHECK(lsb_get_last_select(nullptr, nullptr, nullptr) == LSB_ERR_INVALID, "last_select: null ctx");
}

// lsb_search's refusals that come before any device call.
static void search_cases() {
  uint64_t q[4] = {0, 1, 2, 3};  // host memory: never reaches a device call with a null context
  int64_t out[4] = {-5, -5, -5, -5};
  for (int mode : {LSB_SEARCH_LOWER, LSB_SEARCH_UPPER, LSB_SEARCH_COUNT, LSB_SEARCH_COUNT | LSB_SEARCH_ADD})
    CHECK(lsb_search(nullptr, 0, 4, q, LSB_KEY_U64, 0, mode, out) == LSB_ERR_INVALID, "search: null ctx");
  for (int mode : {3, 7, 8, -1, 1 << 30})
    CHECK(lsb_search(nullptr, 0, 4, q, LSB_KEY_U64, 0, mode, out) == LSB_ERR_INVALID, "search: bad mode");
  CHECK(lsb_search(nullptr, 0, 0, nullptr, LSB_KEY_U64, 0, LSB_SEARCH_LOWER, nullptr) == LSB_ERR_INVALID,
        "search: null ctx, m = 0");
  CHECK(lsb_search(nullptr, -1, -1, nullptr, 6, 2, 3, nullptr) == LSB_ERR_INVALID, "search: all bad");
  for (int i = 0; i < 4; ++i) CHECK(out[i] == -5 && q[i] == (uint64_t)i, "search: a refusal writes nothing");
}

// The refusals of lsb_lookup, lsb_join_count and lsb_store_join that come
// before any device call.
static void join_cases() {
  uint64_t q[4] = {0, 1, 2, 3};
  int64_t col[3][4];
  uint8_t found[4] = {0x55, 0x55, 0x55, 0x55};
  for (auto& c : col)
    for (int64_t& x : c) x = -5;
  int64_t total = -5;
  for (int vb : {0, 4, 8, 3}) {
    CHECK(lsb_lookup(nullptr, 0, 4, q, LSB_KEY_U64, 0, vb ? col[0] : nullptr, vb, found) == LSB_ERR_INVALID,
          "lookup: null ctx");
    CHECK(lsb_store_join(nullptr, 0, 4, 0, col[0], vb ? col[1] : nullptr, vb, col[2], &total) == LSB_ERR_INVALID,
          "store_join: null ctx");
  }
  CHECK(lsb_lookup(nullptr, 0, 0, nullptr, LSB_KEY_U64, 0, nullptr, 0, nullptr) == LSB_ERR_INVALID,
        "lookup: null ctx, m = 0");
  CHECK(lsb_lookup(nullptr, -1, -1, nullptr, 6, 2, nullptr, 8, nullptr) == LSB_ERR_INVALID, "lookup: all bad");
  CHECK(lsb_join_count(nullptr, 0, 4, q, LSB_KEY_U64, 0, col[0], &total) == LSB_ERR_INVALID, "join_count: null ctx");
  CHECK(lsb_join_count(nullptr, 0, 0, nullptr, LSB_KEY_U64, 0, nullptr, nullptr) == LSB_ERR_INVALID,
        "join_count: null ctx, m = 0");
  CHECK(lsb_join_count(nullptr, -1, -1, nullptr, 6, 2, nullptr, &total) == LSB_ERR_INVALID, "join_count: all bad");
  CHECK(lsb_store_join(nullptr, -1, -1, 7, nullptr, nullptr, 5, nullptr, nullptr) == LSB_ERR_INVALID,
        "store_join: all bad");
  for (int i = 0; i < 4; ++i)
    CHECK(col[0][i] == -5 && col[1][i] == -5 && col[2][i] == -5 && found[i] == 0x55 && q[i] == (uint64_t)i,
          "join: a refusal writes nothing");
  CHECK(total == -5, "join: a refusal leaves the total");
}

static int noop_ag(void*, const void*, void*, size_t) { return 0; }
static int noop_a2a(void*, const void*, const size_t*, const size_t*, void*, const size_t*,
                    const size_t*) { return 0; }
// ---- k_onesweep's tile geometry (csrc/lsb_ostile.h) ------------------------
// Sub-array of tile t by the definition: the x with first(x) <= t < first(x + 1).
static int sub_by_definition(int64_t t, int64_t TT) {
  for (int x = 0; x < lsb::kOnesweepSubs; ++x)
    if (lsb::os_sub_first_tile(x, TT) <= t && t < lsb::os_sub_first_tile(x + 1, TT)) return x;
  return -1;
}

// Replays launches of `tiles[i]` rows on one row buffer as the runtime queues
// them (onesweep_launch): the epoch counts up (wrapping to 2 before 2^30),
// a reset zeroes every row and restarts it.  Returns the rows a launch could
// have taken for its own without having written them.
static int64_t replay_rows(const std::vector<int64_t>& tiles, const std::vector<bool>& reset, int64_t cap,
                           uint32_t epoch0, bool fill) {
  std::vector<uint8_t> parity((size_t)cap, 0);
  uint32_t last = epoch0;
  int64_t prev = cap, bad = 0;
  if (epoch0 != 0)  // a buffer in use: every row written at epoch0
    for (auto& p : parity) p = epoch0 & 1u;
  for (size_t i = 0; i < tiles.size(); ++i) {
    if (reset[i]) {
      std::fill(parity.begin(), parity.end(), 0);
      last = 0;
      prev = cap;
    }
    uint32_t epoch = last + 1;
    if (epoch >= (1u << 30)) epoch = 2;
    const lsb::StatusFill f = lsb::status_fill(prev, tiles[i], epoch);
    CHECK(f.count >= 0 && f.first >= 0 && f.first + f.count <= cap, "fill inside the buffer");
    CHECK(f.count == 0 || (f.first == prev && f.first + f.count == tiles[i]), "fill = the rows the last launch left");
    CHECK((f.word & 0x7FFFFFFFu) == 0, "fill word: a parity and nothing else");
    if (fill)
      for (int64_t r = f.first; r < f.first + f.count; ++r) parity[(size_t)r] = (uint8_t)(f.word >> 31);
    for (int64_t r = 0; r < tiles[i]; ++r) bad += parity[(size_t)r] == (epoch & 1u) ? 1 : 0;
    for (int64_t r = 0; r < tiles[i]; ++r) parity[(size_t)r] = epoch & 1u;
    prev = tiles[i];
    last = epoch;
  }
  return bad;
}

static void onesweep_tile_cases(std::mt19937_64& rng) {
  const int sizes[] = {4096, 4608, 5120};
  // The rows' fill: random tile counts, resets and starting epochs.
  int64_t unfilled = 0;
  for (int rep = 0; rep < 200; ++rep) {
    const int64_t cap = 1 + (int64_t)(rng() % 300);
    const size_t len = 1 + rng() % 40;
    std::vector<int64_t> tiles(len);
    std::vector<bool> reset(len);
    for (size_t i = 0; i < len; ++i) {
      // mostly the two counts of a sort (cap and 4 / 5 of it), sometimes any
      const uint64_t k = rng() % 4;
      tiles[i] = k == 0 ? cap : k == 1 ? (cap * 4 + 4) / 5 : 1 + (int64_t)(rng() % (uint64_t)cap);
      reset[i] = rng() % 16 == 0;
    }
    const uint32_t epoch0 = rep % 3 == 0 ? 0u : rep % 3 == 1 ? (uint32_t)(rng() % 1000) : (1u << 30) - 1u - (uint32_t)(rng() % 8);
    CHECK(replay_rows(tiles, reset, cap, epoch0, true) == 0, "a launch takes only rows it wrote");
    unfilled += replay_rows(tiles, reset, cap, epoch0, false);
  }
  CHECK(unfilled > 0, "without the fill the replay finds stale rows (the check has teeth)");
  // The sort's own sequence at 2^30 records: pass 0 (4096), passes 2-6 (5120), pass 7 (4096), twice.
  {
    const int64_t t4 = lsb::os_tiles(int64_t(1) << 30, 4096), t5 = lsb::os_tiles(int64_t(1) << 30, 5120);
    const std::vector<int64_t> seq = {t4, t5, t5, t5, t5, t5, t4, t4, t5, t5, t5, t5, t5, t4};
    CHECK(replay_rows(seq, std::vector<bool>(seq.size(), false), t4, 0, true) == 0, "two packed sorts");
    CHECK(replay_rows(seq, std::vector<bool>(seq.size(), false), t4, 0, false) > 0, "two packed sorts, no fill");
    const lsb::StatusFill f = lsb::status_fill(t5, t4, 7);
    CHECK(f.first == t5 && f.count == t4 - t5 && f.word == 0u, "odd epoch: even fill");
    CHECK(lsb::status_fill(t5, t4, 8).word == 0x80000000u, "even epoch: odd fill, not zero");
    CHECK(lsb::status_fill(t4, t5, 8).count == 0 && lsb::status_fill(t4, t4, 8).count == 0, "no fill for fewer rows");
  }
  // The second track (the pass that reads the regional layout) at 2^30
  // records, regions of 532480 slots: packed sorts read it in tiles of 5120,
  // sorts of whole records and the hybrid in tiles of 4096, in any order.
  {
    const int64_t r4 = lsb::os_rows_track2(532480, 4096, 2048), r5 = lsb::os_rows_track2(532480, 5120, 2048);
    CHECK(r4 == 130 * 2048 && r5 == 104 * 2048, "the layout's tiles at 2^30 records");
    const std::vector<int64_t> seq = {r5, r4, r5, r4, r4, r5, r5, r4, r5};
    CHECK(replay_rows(seq, std::vector<bool>(seq.size(), false), r4, 0, true) == 0, "packed and whole-record sorts on track 2");
    CHECK(replay_rows(seq, std::vector<bool>(seq.size(), false), r4, 0, false) > 0, "track 2 without the fill");
  }
  // Which edge passes take the large tile (tools/edgetile_host.cpp has the
  // search): the caps of 2^24, 2^25 and 2^30 records, the setting's bits,
  // and nothing without large middle passes.
  CHECK(lsb::os_edge_applies(int64_t(1) << 30, 532480, lsb::kOsEdgeAll, 5120, 4096) == lsb::kOsEdgeAll, "2^30: every edge pass");
  CHECK(lsb::os_edge_applies(int64_t(1) << 25, 20480, lsb::kOsEdgeAll, 5120, 4096) == lsb::kOsEdgeAll, "2^25: every edge pass");
  CHECK(lsb::os_edge_applies(int64_t(1) << 24, 12288, lsb::kOsEdgeAll, 5120, 4096) == (lsb::kOsEdgeFirst | lsb::kOsEdgeLast),
        "2^24: 12288 slots are no whole large tiles");
  CHECK(lsb::os_edge_applies(int64_t(1) << 30, 532480, lsb::kOsEdgeLayout, 5120, 4096) == lsb::kOsEdgeLayout, "the setting's bits");
  CHECK(lsb::os_edge_applies(int64_t(1) << 30, 532480, lsb::kOsEdgeAll, 4096, 4096) == 0 &&
            lsb::os_edge_applies(int64_t(1) << 30, 532480, lsb::kOsEdgeAll, 4608, 4096) == 0 &&
            lsb::os_edge_applies(int64_t(1) << 30, 532480, lsb::kOsEdgeAll, 0, 4096) == 0,
        "4096 and 4608 middle passes: every edge pass at 4096");
  CHECK(lsb::os_edge_applies(61440, 4096, lsb::kOsEdgeAll, 5120, 4096) == 0, "too small for the large tile");
  // The applicability bound against a search: os_tile_fits must rule out
  // every m at which a run of t records could cover a whole non-empty
  // sub-array of the next pass and go on past it.
  std::vector<int64_t> ms;
  for (int64_t m = 1; m <= 20 * 5120; m += 509) ms.push_back(m);
  for (int64_t m : {int64_t(61440), int64_t(61441), int64_t(65536), int64_t(81920), int64_t(81921), int64_t(300007),
                    (int64_t(1) << 20) + 12345, int64_t(1) << 30})
    ms.push_back(m);
  for (int64_t m : ms)
    for (int t : sizes)
      for (int tn : sizes) {
        const int64_t TTn = lsb::os_tiles(m, tn);
        bool two = false;  // two boundaries within t - 2 slots of each other, records on both sides
        int64_t prevb = -1;
        for (int x = 1; x < lsb::kOnesweepSubs; ++x) {
          const int64_t b = lsb::os_sub_first_tile(x, TTn) * tn;
          if (b <= 0 || b >= m || b == prevb) continue;
          if (prevb >= 0 && b - prevb <= t - 2) two = true;
          prevb = b;
        }
        if (lsb::os_tile_fits(t, tn, m)) CHECK(!two, "a fitting tile's run crosses at most one boundary");
        if (t <= tn) CHECK(lsb::os_tile_fits(t, tn, m), "a tile no larger than the next pass's always fits");
      }
  CHECK(!lsb::os_big_applies(61440, 5120, 4096) && lsb::os_big_applies(61441, 5120, 4096), "5120 from 16 tiles of 4096 on");
  CHECK(lsb::os_big_applies(65536, 5120, 4096) && lsb::os_big_applies(65536, 4608, 4096), "the smallest regional sort");
  CHECK(!lsb::os_big_applies(int64_t(1) << 30, 4096, 4096), "4096 is not a large tile");
  // A run's cut against the sub-array of each of its slots, both tile sizes.
  for (int rep = 0; rep < 4000; ++rep) {
    const int t = sizes[rng() % 3], tn = sizes[rng() % 3];
    const int64_t m = rep % 4 == 0 ? 61441 + (int64_t)(rng() % 30000) : 1 + (int64_t)(rng() % 2000000);
    if (!lsb::os_tile_fits(t, tn, m)) continue;
    const int64_t TTn = lsb::os_tiles(m, tn);
    // runs near a boundary half of the time
    int64_t R = (int64_t)(rng() % (uint64_t)m);
    if (rep % 2 == 0) {
      const int64_t b = lsb::os_sub_first_tile(1 + (int)(rng() % 7), TTn) * tn;
      R = std::max<int64_t>(0, std::min<int64_t>(m - 1, b - (int64_t)(rng() % (uint64_t)t)));
    }
    const uint32_t cnt = (uint32_t)std::min<int64_t>(m - R, 1 + (int64_t)(rng() % (uint64_t)t));
    const uint32_t lstart = (uint32_t)(rng() % (uint64_t)(t - cnt + 1));
    const uint32_t c = lsb::os_run_cut(R, cnt, lstart, tn, TTn, m);
    bool ok = true;
    for (uint32_t p = 0; p < cnt; ++p) {
      const uint32_t j = lstart + p;
      const int xs = j >= (c & 0xFFFFu) ? (int)(c >> 24) : (int)((c >> 16) & 0xFFu);
      const int64_t tile = (R + p) / tn;
      ok = ok && xs == sub_by_definition(tile, TTn) && xs == lsb::os_sub_of_tile(tile, TTn);
    }
    CHECK(ok, "every slot of a run counted in the sub-array that holds it");
  }
}

static int noop_min(void*, int64_t*) { return 0; }
static int noop_bar(void*) { return 0; }

int main() {
  std::mt19937_64 rng(12345);
  const int64_t ns[] = {0, 1, 7, 1000, 100003};
  const int Ps[] = {1, 2, 3, 8, 64};
  for (int64_t n : ns)
    for (int P : Ps)
      for (int nb : {256, 65536})
        for (bool skew : {false, true})
          if (!(nb == 65536 && P == 64)) plan_case(rng, n, P, nb, skew);
  for (int C : {2, 4, 8})
    for (int P : {1, 3, 8}) chunk_case(rng, P, C);
  for (int64_t n : {int64_t(5), int64_t(1000), int64_t(1003)})
    for (int P : {2, 3, 8})
      for (int S : {1, 4}) wholekey_case(rng, n, P, S);

  // argument checks
  std::vector<int64_t> h(2 * 256, 0), o(2), pl(2 * 256);
  CHECK(lsb_plan_exchange(0, 2, 2, 256, h.data(), o.data(), o.data(), o.data(), o.data(),
                          pl.data()) == LSB_ERR_INVALID, "rank >= P");
  h[5] = -1;
  CHECK(lsb_plan_exchange(10, 2, 0, 256, h.data(), o.data(), o.data(), o.data(), o.data(),
                          pl.data()) == LSB_ERR_INVALID, "negative count");
  lsb_ctx_t* c = nullptr;
  CHECK(lsb_create(nullptr, 1, 1, nullptr, 8) == LSB_ERR_INVALID, "null out");
  CHECK(lsb_create(&c, 1, 0, nullptr, 8) == LSB_ERR_INVALID, "P = 0");
  CHECK(lsb_create(&c, 1, 1, nullptr, 12) == LSB_ERR_UNSUPPORTED, "radix 12");
  CHECK(lsb_sort(nullptr) == LSB_ERR_INVALID, "null ctx");
  CHECK(lsb_set_option(nullptr, 0, 0) == LSB_ERR_INVALID, "null ctx option");
  for (int code = 0; code < 8; ++code) CHECK(lsb_strerror(code) != nullptr, "strerror");
  keyform_case(rng);
  runs_cases(rng);
  select_cases(rng);
  search_cases();
  join_cases();
  onesweep_tile_cases(rng);
  uint64_t col[4] = {0, 1, 2, 3};  // host memory: never reaches a device call with a null context
  CHECK(lsb_load_columns(nullptr, 0, 0, 4, col, LSB_KEY_U64, col, 8, 0) == LSB_ERR_INVALID, "load: null ctx");
  CHECK(lsb_store_columns(nullptr, 0, 0, 4, col, LSB_KEY_U64, col, 8, 0) == LSB_ERR_INVALID, "store: null ctx");
  CHECK(lsb_load_columns(nullptr, -1, -1, -1, nullptr, 6, nullptr, 3, 2) == LSB_ERR_INVALID, "load: all bad");
  CHECK(lsb_store_columns(nullptr, 0, 0, 0, nullptr, LSB_KEY_F32, nullptr, 0, 0) == LSB_ERR_INVALID,
        "store: null ctx, no column");
  CHECK(lsb_per_rank(10, 3) == 4 && lsb_here(10, 3, 2) == 2 && lsb_here(10, 3, 3) == 0, "geometry");

  // no usable device in this container: creation fails cleanly
  int rc1 = lsb_create(&c, 1 << 20, 3, nullptr, 16);
  CHECK((rc1 == LSB_OK) == (c != nullptr), "create result consistent");
  if (c) lsb_destroy(c);
  lsb_comm_ops_t ops = {nullptr, noop_ag, noop_a2a, noop_min, noop_bar};
  c = nullptr;
  int rc2 = lsb_create_rank_ops(&c, 1 << 20, 2, 0, 0, 8, &ops);
  CHECK((rc2 == LSB_OK) == (c != nullptr), "create_rank_ops result consistent");
  if (c) lsb_destroy(c);
  lsb_destroy(nullptr);

  std::printf("host ABI sanitizer driver: %s (create without device: %d, %d)\n",
              fails ? "FAILED" : "ok", rc1, rc2);
  return fails ? 1 : 0;
}
