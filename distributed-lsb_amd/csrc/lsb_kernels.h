// Internal interface between the runtime (lsb_context.cpp, lsb_passes.cpp,
// lsb_exchange.cpp, lsb_wholekey.cpp) and the HIP kernels (lsb_kernels.hip).  Not part of the C ABI (that is include/lsb.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsb_keyform.h"
#include "lsb_ostile.h"

namespace lsb {

// == SortElement (mpi/mpi_lsbsort.cpp:29-32); lsb_elem_t in the ABI.
struct alignas(16) Elem {
  uint64_t key;
  uint64_t val;
};
static_assert(sizeof(Elem) == 16, "16-byte records");
// A record between two passes of a sort whose values all fit 32 bits
// (LSB_OPT_PACK_VALUES): 12 bytes, in the same record buffers.
struct alignas(4) Packed {
  uint32_t klo, khi;  // the key's low and high words
  uint32_t val;
};
static_assert(sizeof(Packed) == 12, "12-byte packed records");

constexpr int kDigitBits = 8;                 // one local pass = one 8-bit digit
constexpr int kBuckets = 1 << kDigitBits;     // 256
#ifndef LSB_SCATTER_BLOCK
#define LSB_SCATTER_BLOCK 256
#define LSB_SCATTER_IPT 16
#endif
constexpr int kScatterBlock = LSB_SCATTER_BLOCK;  // 4 waves
constexpr int kScatterIpt = LSB_SCATTER_IPT;      // items per thread
constexpr int kTile = kScatterBlock * kScatterIpt;  // 4096 elements = 64 KiB in LDS
#ifndef LSB_OS_BLOCK
#define LSB_OS_BLOCK 512
#endif
// k_onesweep workgroups: 8 waves x 8 records for the whole stage (2 per CU),
// 4 waves x 16 for the split stage (3 per CU; at 8 waves its registers spill).
constexpr int kOsBlock = LSB_OS_BLOCK;
constexpr int kOsIpt = kTile / kOsBlock;
#ifndef LSB_OS_SPLIT_BLOCK
#define LSB_OS_SPLIT_BLOCK 256
#endif
constexpr int kOsSplitBlock = LSB_OS_SPLIT_BLOCK;
constexpr int kOsSplitIpt = kTile / kOsSplitBlock;
static_assert(kOsBlock % kBuckets == 0 && kOsBlock * kOsIpt == kTile, "onesweep tile shape");
static_assert(kTile == kOsTile && kOsBlock == kOsWholeBlock && kOsSplitBlock == kOsHalvesBlock,
              "kOsInstances (lsb_ostile.h) is written for these shapes");
constexpr int kMaxChunks = 65536;             // upper bound on the chunk grid

// A rank's `m` elements are cut into `num_chunks` contiguous chunks of
// `chunk_elems` (a multiple of kTile; the last may be short).  The count
// (upsweep) and scatter kernels both run one workgroup per chunk, so the
// per-chunk bucket counts of the former are the exact run offsets of the
// latter.
struct Chunking {
  int64_t chunk_elems = 0;
  int num_chunks = 0;
};
Chunking make_chunking(int64_t m, int max_chunks);

// Input distribution of lsb_generate_ex: the key made from the PCG draw.
constexpr int kDistUniform = 0;  // key = draw (the reference's input)
constexpr int kDistZipf = 1;     // key = mix64(Zipf-like rank of the draw), SURVEY §8d C4
struct KeyGen {
  int dist = kDistUniform;
  double zipf_s = 1.1;
  uint64_t zipf_n = 1ull << 30;
};

// On-device PCG64 (pcg-cpp setseq_xsl_rr_128_64):
// A[i] = {make_key(pcg64(seed)[i]), val0 + i}.
hipError_t launch_pcg_fill(Elem* A, int64_t count, uint64_t seed, uint64_t val0, KeyGen gen,
                           hipStream_t s);

// 65536-bin histogram of the 16-bit digit at `shift` of records already
// sorted by that digit (first[] is 65536 int64 scratch).
hipError_t launch_digit16_counts(const Elem* A, int64_t m, int shift, int64_t* first,
                                 uint64_t* counts, hipStream_t s);

// chunk_hist[b * G + c] = number of elements of chunk c whose digit is b.
// span (optional, 2 words, OR-accumulated): span[0] |= OR of the keys,
// span[1] |= OR of their complements.
hipError_t launch_upsweep(const Elem* A, int64_t m, int shift, Chunking ch,
                          uint32_t* chunk_hist, uint64_t* span, hipStream_t s);

// chunk_off[b * G + c] = sum_{c' < c} chunk_hist[b * G + c'];  totals[b] = row sum.
hipError_t launch_scan(const uint32_t* chunk_hist, int G, uint64_t* chunk_off,
                       uint64_t* totals, hipStream_t s);

// Stable counting-sort scatter of one digit: out[pos] with
// pos = bucket_start[b] + chunk_off[b][c] + rank of the element among the
// chunk's digit-b elements (localShuffle, mpi/mpi_lsbsort.cpp:240-246).
// first16 (optional; the high byte of a 16-bit digit whose low byte the input
// is sorted by): atomicMin of candidate start positions of every 16-bit digit
// at shift - 8; reset it with launch_starts_reset, then launch_starts_to_counts.
hipError_t launch_scatter(const Elem* in, Elem* out, int64_t m, int shift, Chunking ch,
                          const uint64_t* chunk_off, const uint64_t* totals, int64_t* first16,
                          hipStream_t s);
hipError_t launch_starts_reset(int64_t* first16, hipStream_t s);
// counts[d] of a rank whose m records are sorted by the 16-bit digit, from the
// first index of every present digit (first[d] < 0 or >= m: absent).
hipError_t launch_starts_to_counts(const int64_t* first16, int64_t m, uint64_t* counts,
                                   hipStream_t s);

// Single-read passes (P == 1; k_onesweep in lsb_kernels.hip).  The m records
// are kTile-record tiles (a packed sort's middle passes: kOsTile10, below) in
// kOnesweepSubs contiguous sub-arrays (lsb_ostile.h), sub-array x
// = tiles [x*TT/8, (x+1)*TT/8).  sub_hist[x * 256 + b] = count of digit b
// in sub-array x.
// Look-back values are 30 bits (a bucket's count within one sub-array of
// m / 8 + kTile records): m < 2^33 - 2^16, i.e. 137 GB per record buffer.
constexpr int64_t kOnesweepMaxElems = (int64_t(1) << 33) - (int64_t(1) << 16);
inline int64_t onesweep_tiles(int64_t m) { return (m + kTile - 1) / kTile; }
// The packed middle passes (Packed -> Packed counting the next digit, no
// regional layout) may take larger tiles: their stage costs 12 bytes per
// record, so 512 threads x 10 records still fit two workgroups per CU
// (kOsTile10; kOsTile9 is the size between, for measurements).  A packed
// sort's edge passes have kOsTile10 instances too (lsb_ostile.h
// os_edge_applies: the packing first pass, the pass that reads the regional
// layout where its regions are whole tiles of that size, and the last pass,
// which stages keys and 32-bit values apart).  Every other instance keeps
// kTile.  A pass counts the next digit per sub-array of the next pass's
// input, so it is told the next pass's tile size (tn) as well as its own (t).
constexpr int kOsTile9 = kOsBlock * 9;    // 4608
constexpr int kOsTile10 = kOsBlock * 10;  // 5120
inline bool onesweep_packed_tile_ok(int t) { return t == kTile || t == kOsTile9 || t == kOsTile10; }
inline int64_t onesweep_tiles_of(int64_t m, int t) { return os_tiles(m, t); }
// A pass of t-record tiles before one of tn-record tiles over m records, and
// the runtime's rule for the large tile of a sort (lsb_ostile.h: a run may
// cross at most one of the next pass's sub-array boundaries).
inline bool onesweep_tile_fits(int t, int tn, int64_t m) { return os_tile_fits(t, tn, m); }
inline bool onesweep_big_applies(int64_t m, int big) { return os_big_applies(m, big, kTile); }
// sub_hist (zeroed here) of the digit at `shift`; span as for launch_upsweep.
hipError_t launch_subhist(const Elem* A, int64_t m, int shift, int grid, uint32_t* sub_hist,
                          uint64_t* span, hipStream_t s);
// One stable pass in -> out on the digit at `shift`, offsets from sub_hist
// plus a look-back over status (onesweep_tiles(m) * 256 u32 granules, zeroed
// once at allocation; epoch >= 1, new for every launch over the same m, and
// the first launch after a zeroing odd: a granule's tag is the epoch's
// parity, so every launch must write every row it may read: a launch of more
// tiles than the one before on that buffer needs status_fill's rows filled
// first).  next_shift >= 0: also
// next_hist (zeroed here) = sub_hist of the digit at next_shift over out.
// tile_ctr: kOnesweepSubs words of scratch; *err |= 1 if a look-back gave up.
// -DLSB_OS_PROFILE builds: summed s_memtime ticks of k_onesweep's phases
// (0 dequeue, 1 load + rank, 2 publish + scan, 3 stage, 4 write, 5 look-back,
// 6 tile loads in flight, 9 run cuts + the barrier after them; 7 rows summed,
// 8 tiles) over all workgroups' thread 0; hipErrorNotSupported otherwise.
hipError_t onesweep_profile(unsigned long long* out10, bool reset);
// What a pass also hands the exchange that follows it (per-digit exchange
// forms, P > 1): totals[b] = the pass's 256 digit counts; count16 (zeroed
// here) = the 65536 counts of the 16-bit digit at shift - 8, for the high
// byte of a 16-bit exchange digit whose input is sorted by the low byte.
// The hybrid's last byte pass (LSB_OPT_HYBRID, lsb_segsort.hip): the pass
// also orders every segment (records equal on pmask, the k top varying
// bytes) inside its tile by the whole key, so no separate k_segsort pass is
// needed.  A segment lies inside one run of records equal on rmask (pmask
// without this pass's byte), and the pass's input is sorted by rmask; only
// runs that cross a tile boundary can leave a segment split between two
// tiles, and launch_segfix merges those from the pass's input, its look-back
// rows and base (workgroup 0 writes base[x * 256 + b] = the first output slot
// of bucket b's sub-array x records).  *err |= 1 (launch_segfix) when a
// crossing run holds more than kSegCap records (4 * kSegCap when runs
// average over 64 records) on one side of its boundary or spans a whole
// tile: that boundary is left alone, the output is still a permutation sorted
// by pmask, and the runtime runs k_segsort on it.  *err |= 2 (this pass)
// when a segment inside a tile holds more than kSegMax records: its records'
// slots came from walks cut at kSegMax and may collide, so the output is not
// a permutation, and the runtime sorts the kept input with the LSD passes
// (stress seed 19: k_segsort over such an output, its holes holding stale
// records that split the long segments, found nothing too long and kept a
// wrong result).
constexpr int kSegCap = 256;
struct SegPass {
  uint64_t pmask = 0;
  uint64_t rmask = 0;
  int64_t* base = nullptr;  // kOnesweepSubs * 256
  uint32_t* err = nullptr;
};
// Gathered input (per-digit exchange, LSB_OPT_EXCHANGE_GATHER): the pass
// after an exchange reads its records where they arrived instead of from a
// placed copy.  Position p of the placed order (the rank's block in
// (digit, source) order) lies in piece e = b * P + s (bucket b's records from
// source s), the last e with gstart[e] <= p; its record is
//   R[p - place[s * nb + b]]                          (a peer's piece)
//   A[p - place[s * nb + b] + self_adj[chunk of b]]   (s == me, self_in_a)
// (chunk of b: (b & 255) >> chunk_shift; the per-digit exchange in chunks,
// launch_count16_chunks, keeps the rank's own records in C chunk ranges of A;
// unchunked, chunk_shift = 8: one chunk.)
// TileDesc caches that per onesweep tile: up to 4 pieces (first position
// relative to the tile, pointer adjustment, bit j of sel: piece j is in A);
// n = kDescOverflow sends the tile's records to the search over [e0, e1].
constexpr int kDescPieces = 4;
constexpr int kDescOverflow = 0xFF;
struct alignas(16) TileDesc {
  int32_t n, e0, e1, sel;
  int32_t start[kDescPieces];
  int64_t adj[kDescPieces];
};
constexpr int kMaxExchangeChunks = 8;
struct GatherSrc {
  const Elem* R = nullptr;
  const Elem* A = nullptr;
  int64_t self_adj[kMaxExchangeChunks] = {};
  int chunk_shift = 8;
  const int64_t* place = nullptr;  // P * nb place_off (launch_plan)
  const int64_t* gstart = nullptr;  // P * nb piece starts (launch_plan)
  const int64_t* gadj = nullptr;    // P * nb scratch: 2 * pointer adjustment + (1: in A)
  const TileDesc* desc = nullptr;   // onesweep_tiles(m)
  int P = 1, nb = 256, me = 0, self_in_a = 1;
  int64_t a_len = 0, r_len = 0;     // records in A and R (debug builds check every gathered read)
};
// gadj, then desc[t] for every onesweep tile of m records (after launch_plan
// with gstart).
hipError_t launch_gather_desc(const GatherSrc& g, int64_t m, TileDesc* desc, hipStream_t s);
// The per-digit exchange in chunks (LSB_OPT_EXCHANGE_CHUNKS, 16-bit digits;
// DESIGN.md §6): after the low-byte pass of digit d, B (m records) is sorted
// by the low byte l; chunk k = the records with l in [k << cshift,
// (k + 1) << cshift), a contiguous range of B (C = 256 >> cshift chunks).  One
// read of B gives count16[(h << 8) | l] (zeroed here: the digit's 65536
// counts, for the exchange plan) and chunk_hist[(k * 8 + x) * 256 + h]
// (zeroed here: the high byte's sub-array histogram over chunk k's own tiles,
// the sub_hist of chunk k's high-byte pass), so the plan and the sends can
// precede the high-byte pass, which then runs chunk by chunk while the
// previous chunk is on the wire.  lo_hist: the low byte's sub-array
// histogram (its totals give the chunk bounds).  shift16 = 16 * d.
hipError_t launch_count16_chunks(const Elem* B, int64_t m, int shift16, const uint32_t* lo_hist, int cshift,
                                 int grid, uint64_t* count16, uint32_t* chunk_hist, hipStream_t s);
// Regional first pass (P == 1 LSD sorts of at least kRegionMin records,
// LSB_OPT_REGION_FIRST): the sort's first pass needs no
// histogram read.  Its records of digit b from sub-array x go to region
// r = b * kOnesweepSubs + x of the output, a slot range of `cap` records
// (a multiple of kTile, with slack over the mean region_mean(m)): slot
// r * cap + (the record's rank among them, from the look-back alone).  The
// output then holds the records in the stable order of that digit, with a
// gap at the end of every region, and the second pass reads it tile by tile,
// taking counts[r] records of each region (its tiles of kTile slots:
// the valid prefix of each).  A region that would overflow sets *ovf (the
// output is invalid and the runtime sorts the kept input the usual way).
// Mode 1 (the first pass, next digit counted over the regional layout's
// tiles): counts[r] accumulated here (zeroed by the launcher).  Mode 2 (the
// second pass): reads that layout, writes a dense one.  No key span: the
// runtime takes the form only when a sample shows every byte varying.
constexpr int64_t kRegionMin = int64_t(1) << 27;
constexpr int kRegions = kBuckets * kOnesweepSubs;  // 2048
inline int64_t region_mean(int64_t m) { return (m + kRegions - 1) / kRegions; }
// Slots per region for m records (0: fewer than min_m records, too few for
// the form): the mean plus max(mean / 64, 6 standard deviations of a uniform
// region's count), rounded up to whole tiles.  2^27 records: +6.25 % slots;
// 2^30: +1.6 % (130 tiles per region).  (Tests lower min_m to cover small
// sorts, whose regions are then one mostly empty tile each.)  The two
// constants are build knobs for experiments (tools/r05/region_slack.sh).
#ifndef LSB_REGION_SIGMA
#define LSB_REGION_SIGMA 6
#endif
#ifndef LSB_REGION_DIV
#define LSB_REGION_DIV 64
#endif
inline int64_t region_cap(int64_t m, int64_t min_m = kRegionMin) {
  if (m < min_m || m <= 0) return 0;
  const int64_t mu = region_mean(m);
  int64_t sd = 1;
  while (sd * sd < mu) ++sd;
  const int64_t a = mu / LSB_REGION_DIV, b = LSB_REGION_SIGMA * sd;
  const int64_t slack = a > b ? a : b;
  return (mu + slack + kTile - 1) / kTile * kTile;
}
// Region r's first slot.  LSB_REGION_STAGGER (experiment): regions one tile
// apart more than `cap`, each shifted by (37 r mod 16) x 256 records, so that
// the first pass's 2048 write frontiers do not sit at one stride.
#ifndef LSB_REGION_STAGGER
#define LSB_REGION_STAGGER 0
#endif
__host__ __device__ inline int64_t region_stride(int64_t cap) { return cap + (LSB_REGION_STAGGER ? kTile : 0); }
__host__ __device__ inline int64_t region_base(int64_t r, int64_t cap) {
  return r * region_stride(cap) + (LSB_REGION_STAGGER ? ((r * 37) & 15) * 256 : 0);
}
// Records a buffer holding the regional layout needs.
inline int64_t region_slots(int64_t m, int64_t min_m = kRegionMin) {
  return region_stride(region_cap(m, min_m)) * kRegions;
}
struct RegionPass {
  int64_t cap = 0;                    // slots per region
  uint32_t* counts = nullptr;         // [kRegions] records per region
  uint32_t* ovf = nullptr;            // mode 1: set when a region overflows
  uint32_t* wide = nullptr;           // mode 1 writing packed records: set when a value needs over 32 bits
};
// Sample of the sort's first digit (the regional first pass's go / no-go):
// 256 workgroups read one tile each, spread over the m records; hist[256]
// (zeroed here) gets the tiles' digit counts at `shift`, span[2] (zeroed
// here) the OR of their keys and complements, *wide (zeroed here) the OR of
// their values' high words.
hipError_t launch_sample(const Elem* A, int64_t m, int shift, uint32_t* hist, uint64_t* span, uint32_t* wide,
                         hipStream_t s);
struct OnesweepExtra {
  uint64_t* totals = nullptr;
  uint64_t* count16 = nullptr;
  int halves = 1;  // 2: split stage, 3 workgroups per CU (skewed keys; not with count16)
  const SegPass* seg = nullptr;  // the hybrid's last pass (no next digit, whole stage)
  const GatherSrc* gather = nullptr;  // records gathered from an exchange (`in` unused)
  bool probe = false;  // the placement probe's pass (a last pass, launched as k_onesweep_probe)
  const RegionPass* region = nullptr;  // with region_mode 1 or 2: the regional layout
  int region_mode = 0;  // 1: write it (needs a next digit); 2: read it (sub_hist over its tiles)
  // Packed records (regional LSD sorts only: whole stage, nothing else set).
  // `in` / `out` then point at Packed records.  The four forms: region_mode 1
  // Elem -> Packed (values truncated; region->wide says when that lost bits),
  // region_mode 2 and a next-counting pass Packed -> Packed, and a last pass
  // Packed -> Elem.
  bool pack_in = false, pack_out = false;
  // Records per tile of this pass's input and of the next pass's (0: kTile).
  // Over kTile only for a packed sort's passes, and only where
  // onesweep_tile_fits.  The launch is refused unless kOsInstances
  // (lsb_ostile.h) has a row for the request (os_select): a new tile size or
  // form is one more row there, and the row is what builds its kernel.
  int tile = 0, next_tile = 0;
};
// The runtime's choice of OnesweepExtra::halves for a rank, from a digit's
// sub-array histogram (kOnesweepSubs x 256 counts of m records): 2 when one
// bucket holds more than 1/32 of the records.
int onesweep_halves_for(const uint32_t* sub_hist_host, int64_t m);
hipError_t launch_onesweep(const Elem* in, Elem* out, int64_t m, int shift, int next_shift,
                           const uint32_t* sub_hist, uint32_t* next_hist, uint32_t* status,
                           uint32_t* tile_ctr, uint32_t epoch, uint32_t* err, int grid,
                           hipStream_t s, OnesweepExtra extra = OnesweepExtra());

// Hybrid local sort (LSB_OPT_HYBRID, lsb_segsort.hip): `in` is stably sorted
// by the bits of pmask (the top varying bytes of the key); k_segsort sorts
// every segment (maximal run of equal key & pmask) stably by the whole key,
// in -> out.  A segment longer than kSegMax records sets *err (output
// invalid: the runtime sorts the kept input by the LSD passes instead).
// grid: persistent workgroups (3 per CU).
// 64: past ~32 records per segment the walks cost more than the LSD passes
// the hybrid saves (64 per segment: k_segsort 69 ms against 7 for a byte
// pass), and each walk is bounded by kSegMax each way, so
// duplicate-heavy keys that do not look skewed (e.g. 2^20 distinct keys,
// ~1000 copies each, at 2^30 records) cost the hybrid at most a few ms of
// walks before the sort redoes the kept input by the LSD passes (advisor
// r03).  Uniform keys at the runtime's k hold ~0.25-2 records per segment
// (the longest of 2^33 records: ~17).
constexpr int kSegMax = 64;
hipError_t launch_segsort(const Elem* in, Elem* out, int64_t m, uint64_t pmask, uint32_t* err,
                          int grid, hipStream_t s);
// After a SegPass launch in -> out over m records on the byte at `shift`
// (status: that launch's look-back rows): merge every segment split between
// tiles t and t + 1, in place in `out`.
hipError_t launch_segfix(const Elem* in, Elem* out, int64_t m, int shift, const uint32_t* status,
                         const SegPass& seg, int grid, hipStream_t s);

// Receiver-side placement of one source's received range: src[i] (receive
// index k0 + i) goes to out[off_row[digit] + k0 + i], off_row = the source's
// row of the placement table (place_off[s * nbuckets ...]); out holds
// out_len records (the receive order [k0, k0 + count) lies inside it).
// next_shift >= 0: also add the placed records' digit at next_shift to
// next_hist[x * 256 + b] (x = the out position's onesweep sub-array over
// out_len records; zeroed by the caller): the next local pass's sub_hist.
// store = false (with next_shift >= 0): count only, out untouched (the next
// pass gathers, GatherSrc).  skew: the sort's keys are skewed (its stage
// split): the count adds once per run of equal counters.
hipError_t launch_place(const Elem* src, Elem* out, int64_t out_len, int64_t k0, int64_t count,
                        int shift, int nbuckets, const int64_t* off_row, hipStream_t s,
                        int next_shift = -1, uint32_t* next_hist = nullptr, bool store = true,
                        bool skew = false);

// Peer-store exchange (opt-in, LSB_OPT_EXCHANGE_PEER): from the all-gathered
// counts hist[s * nb + b], rank `me` writes each of its m bucket-ordered
// records straight into its owner's receiving buffer: record i of bucket b
// goes to global position g = base[b] + i, i.e. dst[g / per][g % per].
// dst[q] is rank q's buffer as this process sees it; base: nb int64 scratch.
// Each workgroup ends with a system-scope release; launch_system_acquire is
// the owner's matching acquire (every XCD's L2) after the barrier collective.
hipError_t launch_peer_exchange(const Elem* src, int64_t m, int shift, int nbuckets,
                                const uint64_t* hist, int P, int me, int64_t per,
                                Elem* const* dst, int64_t* base, hipStream_t s);
hipError_t launch_system_acquire(hipStream_t s);

// Exchange plan of rank `me` on device from the all-gathered counts
// hist[s * nb + b] (same rule as the host planner lsb_plan_exchange):
// place[s * nb + b] = place_off, place[P * nb + s] = rend (inclusive scan of
// recv counts), counts[0..P) = send counts, counts[P..2P) = recv counts.
// work: P * nb int64, total: nb int64 scratch.  gstart (optional, P * nb):
// gstart[b * P + s] = first position of piece (b, s) in my block, clamped to
// [0, here] (nondecreasing in b * P + s).  cshift < 8 (the chunked exchange,
// nb = 65536, C = 256 >> cshift chunks of the low byte): a source's pieces
// lie in R in chunk order (chunk of l, h, l) instead of digit order, which
// place_off follows, and chunk_counts[q * C + k] = my records of chunk k for
// owner q, chunk_counts[P * C + s * C + k] = source s's records of chunk k
// for me.
hipError_t launch_plan(const uint64_t* hist, int P, int nb, int me, int64_t n, int64_t* work,
                       int64_t* total, int64_t* place, int64_t* counts, hipStream_t s,
                       int64_t* gstart = nullptr, int cshift = 8, int64_t* chunk_counts = nullptr);

// ---- whole-key exchange (radix_bits = 64; lsb_merge.hip) ----
// Splitter search: for Q targets T_t, state[2t .. 2t+1] = key interval
// [lo, hi] holding the key found at global position T_t.  One round:
// launch_split_cands (cnt[t * kSplitCands + j] = this rank's count of keys
// below candidate j), all-gather cnt over the P ranks, launch_split_update.
// kSplitRounds rounds leave lo == hi; launch_split_final then writes this
// rank's {#keys < k*, #keys <= k*} per target.  A is sorted by key.
constexpr int kSplitCands = 256;
constexpr int kSplitRounds = 8;
constexpr int kMergeMaxCuts = 512;  // P * slices cap of the whole-key exchange
hipError_t launch_split_init(uint64_t* state, int Q, hipStream_t s);
hipError_t launch_split_cands(const Elem* A, int64_t m, const uint64_t* state, int Q, uint64_t* cnt,
                              hipStream_t s);
hipError_t launch_split_update(const uint64_t* gathered, int P, int Q, const int64_t* targets,
                               uint64_t* state, hipStream_t s);
hipError_t launch_split_final(const Elem* A, int64_t m, const uint64_t* state, int Q, uint64_t* out,
                              hipStream_t s);
// One level of a merge tree: npairs stable merges of two key-sorted runs (a
// before b on equal keys; nb = 0 copies a) into out (na + nb records,
// disjoint from a and b).  tile0[p] = first tile of pair p in the level's
// tile numbering (tiles of kMergeTile outputs), tiles = their total.
// path: tiles + npairs int64 scratch; grid: persistent workgroups (3 per CU).
constexpr int kMergeTile = 2048;
constexpr int kMergeMaxPairs = 32;
struct MergePair {
  const Elem* a;
  const Elem* b;
  Elem* out;
  int64_t na, nb, tile0;
};
struct MergeLevel {
  MergePair p[kMergeMaxPairs];
  int npairs;
  int64_t tiles;
};
inline int64_t merge_tiles(int64_t n) { return (n + kMergeTile - 1) / kMergeTile; }
hipError_t launch_merge_level(const MergeLevel& level, int64_t* path, int grid, hipStream_t s);

// O(n) bit-exact stable-sort check of a rank's here-part (see lsb_verify).
// first_bad must hold UINT64_MAX before the launch; receives min bad global index.
// cnt records src -> dst on one device (loopback exchange copies).
hipError_t launch_copy_records(Elem* dst, const Elem* src, int64_t cnt, hipStream_t s);
// cnt packed records src -> Elem records dst (distinct buffers).
hipError_t launch_unpack(Elem* dst, const Packed* src, int64_t cnt, hipStream_t s);
// Caller-owned columns (lsb_columns.hip; key forms: lsb_keyform.h).  Load:
// A[i] = {encode(keys[i]), vals[i]} for i in [0, cnt), the value 8 bytes raw,
// 4 bytes zero-extended, or val0 + i when val_bytes is 0 (vals null exactly
// then).  Store: the inverse, keys[i] = decode(A[i].key), vals[i] = the value
// or its low word; keys or vals may be null.  Columns are aligned to their
// element; 16-byte aligned ones take 16-byte accesses.  hipErrorInvalidValue
// on an unknown key type, flag or val_bytes, before any launch.
hipError_t launch_load_columns(Elem* A, int64_t cnt, const void* keys, int key_type, const void* vals,
                               int val_bytes, uint64_t val0, int flags, hipStream_t s);
hipError_t launch_store_columns(const Elem* A, int64_t cnt, void* keys, int key_type, void* vals, int val_bytes,
                                int flags, hipStream_t s);
// The records A[0, cnt) rekeyed in place by their values (k_rekey, one launch
// on s).  Columns: A[i].key = encode(keys[A[i].val]) with keys a column of
// n_col elements of key_type, aligned to its element; a record whose value is
// not below n_col stays as it is, no address is formed from it, and *err (a
// device word the caller zeroed) becomes non-zero.  Index: A[i].key =
// A[i].val / divisor.  The values are never written differently.
// hipErrorInvalidValue on an unknown key type or flag, null keys or err,
// n_col <= 0 or divisor == 0, before any launch.
hipError_t launch_rekey_columns(Elem* A, int64_t cnt, const void* keys, int64_t n_col, int key_type, int flags,
                                uint32_t* err, hipStream_t s);
hipError_t launch_rekey_index(Elem* A, int64_t cnt, uint64_t divisor, hipStream_t s);
hipError_t launch_verify(const Elem* A, int64_t here, int64_t gbase, int64_t n, int64_t per,
                         KeyGen gen, unsigned long long* first_bad, hipStream_t s);

// Key-only local sortedness (checkSorted); *unsorted set to 1 on a descent.
hipError_t launch_check_sorted(const Elem* A, int64_t here, unsigned int* unsorted, hipStream_t s);

// Runs of equal keys (lsb_runs.hip; lsb_count_runs / lsb_store_runs,
// include/lsb.h).  A head is a position i in [1, here) with
// A[i].key != A[i-1].key; position 0 is never counted (the host planner
// decides it from the previous rank: head0).  The rank's records are tiles
// of kTile, run_tiles(here) of them.
inline int64_t run_tiles(int64_t here) { return (here + kTile - 1) / kTile; }
constexpr int kRunSumWords = 5;  // sum[0..3]: first key, last key, inner, lead; sum[4]: error word
// One read of A (here > 0): tile_cnt[t] = heads of tile t; tile_base[t] = heads
// of the tiles before it; sum[0..3] = the rank's summary words (first and
// last key, the number of heads, the smallest head or `here`).
hipError_t launch_run_count(const Elem* A, int64_t here, uint32_t* tile_cnt, int64_t* tile_base, uint64_t* sum,
                            hipStream_t s);
// One more read of A.  With head j (in position order, position 0 among them
// exactly when head0) at position i: keys[j] = decode(A[i].key), starts[j] =
// gbase + i, firsts[j] = A[i].val (val_bytes 8) or its low word (4); then
// counts[j] = starts[j + 1] - starts[j], the last one end - starts[j].  Any
// output may be null (counts only with starts; firsts null exactly when
// val_bytes is 0).  runs = head0 + the heads counted by launch_run_count:
// every output holds that many elements.  A tile whose heads are not the
// tile_cnt[t] of the count sets *err and writes nothing.
// hipErrorInvalidValue on an unknown key type, flag or val_bytes, before any
// launch.
hipError_t launch_run_write(const Elem* A, int64_t here, int64_t gbase, int head0, const uint32_t* tile_cnt,
                            const int64_t* tile_base, void* keys, int key_type, int flags, int64_t* starts,
                            int64_t* counts, void* firsts, int val_bytes, int64_t runs, int64_t end,
                            uint32_t* err, hipStream_t s);

// Reductions over the values of a run (lsb_plan_reduce / lsb_store_reduce,
// include/lsb.h).  (op, val_type) picks one of four
// associative combines over 64-bit words: integer add, double add, and the
// unsigned min / max of encode(value) (lsb_keyform.h's order of the type).
// Values lie in memory as the caller's bits; red_load / red_store move them
// into and out of the form the combine works on.  Host and device run the
// same code: the planner folds the ranks' leads with what the kernels use.
constexpr int kReduceSum = 0, kReduceMin = 1, kReduceMax = 2;  // == LSB_REDUCE_*
enum RedForm { kRedAdd = 0, kRedFadd = 1, kRedMin = 2, kRedMax = 3 };
inline bool reduce_valid(int op, int val_type) {
  return op >= kReduceSum && op <= kReduceMax && val_type >= kKeyU64 && val_type <= kKeyF64;
}
inline int red_form(int op, int val_type) {
  return op == kReduceSum ? (val_type == kKeyF64 ? kRedFadd : kRedAdd) : op == kReduceMin ? kRedMin : kRedMax;
}
template <int F>
__host__ __device__ inline uint64_t red(uint64_t a, uint64_t b) {
  if constexpr (F == kRedAdd) return a + b;
  else if constexpr (F == kRedFadd)
    return __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, a) + __builtin_bit_cast(double, b));
  else if constexpr (F == kRedMin) return a < b ? a : b;
  else return a > b ? a : b;
}
__host__ __device__ inline uint64_t red(int form, uint64_t a, uint64_t b) {
  switch (form) {
    case kRedAdd: return red<kRedAdd>(a, b);
    case kRedFadd: return red<kRedFadd>(a, b);
    case kRedMin: return red<kRedMin>(a, b);
    default: return red<kRedMax>(a, b);
  }
}
// The combine's identity, in the working form: 0, -0.0 (x + -0.0 == x for
// every double, -0.0 included), the largest and the smallest encoding.
__host__ __device__ inline uint64_t red_identity(int form) {
  return form == kRedFadd ? 0x8000000000000000ull : form == kRedMin ? ~0ull : 0ull;
}
__host__ __device__ inline bool red_encodes(int form) { return form == kRedMin || form == kRedMax; }
__host__ __device__ inline uint64_t red_load(int form, uint64_t bits, const KeyForm& f) {
  return red_encodes(form) ? encode(bits, f) : bits;
}
__host__ __device__ inline uint64_t red_store(int form, uint64_t x, const KeyForm& f) {
  return red_encodes(form) ? decode(x, f) : x;
}
// The workgroup partials of launch_run_lead, at most (== kRunGridCap).
constexpr int kRunLeadParts = 8192;
// *out = op over A[0, lead).val (lead > 0): at most kRunLeadParts workgroup
// partials into parts, then one workgroup over them.  The order and the
// association of the combines depend on lead alone.
hipError_t launch_run_lead(const Elem* A, int64_t lead, int op, int val_type, uint64_t* parts, uint64_t* out,
                           hipStream_t s);
// One more read of A after launch_run_count, then one workgroup.  out[j] = op
// over the values of the records from head j up to the next head or the
// rank's end, j as in launch_run_write (runs = head0 + the counted heads,
// > 0); the rank's last run also takes `tail` (the caller's bits).
// tile_lead[run_tiles(here)] is scratch: op over each tile's records in front
// of its first head.  A tile whose heads are not the tile_cnt[t] of the count
// sets *err and writes nothing; no index leaves [0, runs).
hipError_t launch_run_reduce(const Elem* A, int64_t here, int head0, const uint32_t* tile_cnt,
                             const int64_t* tile_base, int op, int val_type, uint64_t tail, uint64_t* tile_lead,
                             uint64_t* out, int64_t runs, uint32_t* err, hipStream_t s);

// A run id per record (lsb_label_runs, include/lsb.h).  One
// more read of A after launch_run_count and one write of B (another buffer of
// at least `here` records): B[i] = {A[i].key, id} (kLabelKeep) or
// {A[i].val, id} (kLabelByValue), id = gid0 + the heads of the rank at or
// below i (position 0 among them exactly when head0) - 1: the index
// launch_run_write gives the run that holds position i, plus gid0, the global
// index of the rank's first run (>= 1 when head0 is 0: the records in front
// of the first head get gid0 - 1).  A tile whose heads are not the tile_cnt[t]
// of the count sets *err and writes nothing.  hipErrorInvalidValue on an
// unknown mode, before any launch.
constexpr int kLabelKeep = 0, kLabelByValue = 1;  // == LSB_LABEL_*
hipError_t launch_run_label(const Elem* A, Elem* B, int64_t here, int64_t gid0, int head0, const uint32_t* tile_cnt,
                            const int64_t* tile_base, int mode, uint32_t* err, hipStream_t s);

// The scan within the runs (lsb_plan_scan / lsb_store_scan / lsb_scan_runs,
// include/lsb.h): per record, op over the values of its run's
// records up to and including it.  Ops 0..2 are the reductions' (the same four
// combines); kScanCount and kScanStart take every record's operand as 1 under
// the integer add, so the inclusive scan c of a record gives its position in
// its run, c - 1, and its run's first global position, its own - (c - 1).
constexpr int kScanCount = 3, kScanStart = 4;  // == LSB_SCAN_COUNT, LSB_SCAN_START
inline bool scan_valid(int op, int val_type) {
  return reduce_valid(op, val_type) || ((op == kScanCount || op == kScanStart) && val_type == kKeyU64);
}
inline int scan_form(int op, int val_type) { return op >= kScanCount ? kRedAdd : red_form(op, val_type); }
// One more read of A after launch_run_count (here > 0), then one workgroup.
// tile_open[t] = the combine over tile t's records from its last head on (the
// whole tile without one; position 0 is a head exactly when head0);
// tile_in[t] = the combine, in tile order, over the tile_open of the tiles
// before t back to and including the last one with a head (the identity for
// tile 0): what the rank's earlier tiles add to the run open at t's first
// record.  Both in the combine's working form, run_tiles(here) words each.
// *trail = the same over all the rank's tiles, in the caller's bits: the
// combine over the rank's records from its last head on.  A tile whose heads
// are not the tile_cnt[t] of the count sets *err.
hipError_t launch_run_scan_plan(const Elem* A, int64_t here, int head0, const uint32_t* tile_cnt, int op,
                                int val_type, uint64_t* tile_open, uint64_t* tile_in, uint64_t* trail,
                                uint32_t* err, hipStream_t s);
// One more read of A and one write.  The result of the record at slot i is
// ((carry + tile_in[t]) + the scan inside tile t) for i < lead, (tile_in[t] +
// the scan inside t) for a later record in front of its tile's first head,
// and the scan inside t otherwise; carry in the caller's bits, lead = the
// rank's first head (0 when head0, `here` without one).  gbase = the global
// position of slot 0 (kScanStart).  sink: kScanColumn writes out[i] = the
// result (8-byte elements), kScanKeep out[i] = {A[i].key, result} and
// kScanByValue {A[i].val, result} (16-byte records, another buffer than A).
// A tile whose heads are not the tile_cnt[t] of the count sets *err and writes
// nothing; no index leaves [0, here).
constexpr int kScanColumn = 0, kScanKeep = 1, kScanByValue = 2;
hipError_t launch_run_scan_write(const Elem* A, int64_t here, int64_t gbase, int head0, int64_t lead,
                                 const uint32_t* tile_cnt, const uint64_t* tile_in, int op, int val_type,
                                 uint64_t carry, int sink, void* out, uint32_t* err, hipStream_t s);

// The k-th key and the first k + 1 records without a sort (lsb_select.hip;
// lsb_select / lsb_store_select, include/lsb.h).
// A rank's table of a round: kSelHist counts, then two words (round one: the
// OR of the keys and the OR of their complements; later rounds: the records
// the compaction reserved, and its error word); these kSelWords are what the
// ranks gather.  The word after them is the store's error word.
constexpr int kSelHist = 256;
constexpr int kSelWords = kSelHist + 2;
constexpr int kSelBufWords = kSelWords + 1;
// One read of src[0, m) (m > 0): words[d] += the records with
// (key & mask) == prefix whose byte at `shift` is d.  span: words[256] |= key,
// words[257] |= ~key over every record (round one; mask is 0 then).  dst not
// null: the matching records are also copied, whole and in any order, into
// dst[0, bound); words[256] += the records reserved there, and a record past
// `bound` is not stored and sets words[257].  dst and src do not overlap.
hipError_t launch_select_hist(const Elem* src, int64_t m, int shift, uint64_t prefix, uint64_t mask, bool span,
                              Elem* dst, int64_t bound, uint64_t* words, hipStream_t s);
// One read of A (here > 0): tile_cnt[t] = (keys == pivot) << 16 | (keys <
// pivot) of tile t (run_tiles(here) of them); tile_base[2 t], [2 t + 1] = the
// keys below and equal in the tiles before t.  Totals other than `below` and
// `equal` set *err.
hipError_t launch_select_count(const Elem* A, int64_t here, uint64_t pivot, int64_t below, int64_t equal,
                               uint32_t* tile_cnt, int64_t* tile_base, uint32_t* err, hipStream_t s);
// One more read of A.  The record at slot i is selected when key < pivot, or
// key == pivot and fewer than `share` equal keys lie in front of it; the j-th
// selected record in slot order writes keys[j] = decode(key) and vals[j] = its
// value (val_bytes 8) or its low word (4).  Either output may be null (vals
// exactly when val_bytes is 0), not both.  take = below + share: no index
// leaves [0, take); a record that would sets *err, and so does a tile whose
// counts are not the tile_cnt[t] of the count, which then writes nothing.
// Columns aligned to 16 bytes are written in 16-byte accesses.
hipError_t launch_select_write(const Elem* A, int64_t here, uint64_t pivot, int64_t share, int64_t take,
                               const uint32_t* tile_cnt, const int64_t* tile_base, void* keys, int key_type, int flags,
                               void* vals, int val_bytes, uint32_t* err, hipStream_t s);

// Searching a rank's sorted records for a column of queries (lsb_search.hip;
// lsb_search, include/lsb.h).  == LSB_SEARCH_*.
constexpr int kSearchLower = 0, kSearchUpper = 1, kSearchCount = 2, kSearchAdd = 4;
inline bool search_mode_valid(int mode) { return mode >= 0 && (mode & ~kSearchAdd) <= kSearchCount; }
// One strided read of A (here > 0): fence[t] = the key of record t * kTile,
// run_tiles(here) words.
hipError_t launch_search_fence(const Elem* A, int64_t here, uint64_t* fence, hipStream_t s);
// out[i] = (mode & kSearchAdd ? out[i] : 0) + c_i for the m typed queries
// (m > 0, here > 0), c_i the records of A[0, here) with key <, <= or == the
// encoded query; fence as launch_search_fence left it.  Every record index
// probed lies in [0, here), every fence index in [0, run_tiles(here)),
// whatever A holds; every c_i in [0, here].
hipError_t launch_search(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                         int key_type, int flags, int mode, int64_t* out, hipStream_t s);

// The matches themselves (lsb_search.hip; lsb_lookup, lsb_join_count,
// lsb_store_join, include/lsb.h).  A, here, fence and the
// typed queries as for launch_search; the same bounds hold for every probe.
// Query i with a record of its encoded key e_i: vals[i] = the value of the
// first such record (val_bytes 8) or its low word (4), found[i] = 1; a query
// without one touches neither.  vals null exactly when val_bytes is 0; vals or
// found is given.
hipError_t launch_lookup(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                         int key_type, int flags, void* vals, int val_bytes, uint8_t* found, hipStream_t s);
// A rank's join plan: lower[i] = the records below e_i, off[i] = the matches
// of the queries in front of i (their counts c_i first, then scanned in
// place), counts[i] = c_i when given, tile[join_qtiles(m)] = the sum of all
// c_i (tile[t] = the sum over the tiles of kJoinQTile queries before t).
// m int64 each for lower and off, join_qtiles(m) + 1 for tile.  Three kernels
// and no wait between workgroups.  lower[i] + c_i <= here whatever A holds.
constexpr int kJoinQTile = 4096;
__host__ __device__ inline int64_t join_qtiles(int64_t m) { return (m + kJoinQTile - 1) / kJoinQTile; }
hipError_t launch_join_count(const Elem* A, int64_t here, const uint64_t* fence, const void* queries, int64_t m,
                             int key_type, int flags, int64_t* lower, int64_t* off, int64_t* counts, int64_t* tile,
                             hipStream_t s);
// Output slot o of [0, total), total > 0 the plan's sum: i = the query with
// off[i] <= o < off[i + 1] (off[m] = total), p = lower[i] + o - off[i];
// left[o] = query_base + i, right[o] = A[p].val (val_bytes 8) or its low word
// (4), pos[o] = gbase + p.  Any output may be null (right exactly when
// val_bytes is 0), not all.  With lower and off as launch_join_count left
// them, no index leaves [0, m), [0, here) or [0, total).
hipError_t launch_join_expand(const Elem* A, int64_t here, const int64_t* lower, const int64_t* off, int64_t m,
                              int64_t total, int64_t query_base, int64_t gbase, int64_t* left, void* right,
                              int val_bytes, int64_t* pos, hipStream_t s);

}  // namespace lsb
