/*
 * lsb.h — C ABI of the MI355X-native distributed LSD radix sort.
 *
 * The reference (ronawho/distributed-lsb) has no library or FFI: every
 * variant is one program whose in-process seams are
 *   mySort(A, B)              mpi/mpi_lsbsort.cpp:580-585, shmem/shmem_lsbsort.cpp:460-472
 *   globalShuffle(A, B, d)    mpi/mpi_lsbsort.cpp:481-577, shmem/shmem_lsbsort.cpp:388-457
 *   DistributedArray::create  mpi/mpi_lsbsort.cpp:137-161
 *   checkSorted()             shmem/shmem_lsbsort.cpp:180-219
 *   PCG input init            mpi/mpi_lsbsort.cpp:643-666
 *   verify (gather + stable_sort + ==)  mpi/mpi_lsbsort.cpp:673-679,710-738
 * Each entry point below names the seam it replaces.  Plain C types only;
 * no C++ exception crosses this boundary; every function returning int
 * returns LSB_OK (0) or an LSB_ERR_* code (lsb_strerror() describes it).
 *
 * A context is one "world" of P ranks (P = num_ranks) over the block
 * partition per = ceil(n/P) (mpi/mpi_lsbsort.cpp:144-149):
 *   - lsb_create():      one process drives all P ranks (logical ranks, each
 *                        with its own buffers; several may share one GPU).
 *                        The per-pass exchange is a device-to-device copy
 *                        with exactly the all-to-all-v semantics of RCCL.
 *   - lsb_create_rank(): one process per GPU (torchrun / hip_lsbsort --gpus);
 *                        this process is rank `rank`; the exchange is RCCL
 *                        (AllGather of bucket counts + AllToAllv)
 *                        over xGMI.  Collective calls must be made by all
 *                        ranks in the same order, as in the MPI reference.
 * The context owns every device buffer (A, B, send/recv, histograms, RCCL
 * communicator), as DistributedArray owns localPart_.  A context is driven
 * by one host thread and is not re-entrant.
 */
#ifndef LSB_H
#define LSB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSB_OK                 0
#define LSB_ERR_INVALID        1  /* bad argument (rank, range, digit, radix) */
#define LSB_ERR_HIP            2  /* a HIP runtime call failed */
#define LSB_ERR_RCCL           3  /* an RCCL call failed */
#define LSB_ERR_NOMEM          4  /* device or host allocation failed */
#define LSB_ERR_VERIFY         5  /* lsb_verify found a mismatch */
#define LSB_ERR_UNSUPPORTED    6  /* valid request this build does not do */
#define LSB_ERR_STATE          7  /* call not valid in this context state */

#define LSB_UNIQUE_ID_BYTES  128  /* == NCCL_UNIQUE_ID_BYTES */

/* == struct SortElement (mpi/mpi_lsbsort.cpp:29-32): 16 B, little-endian,
 * key then val, no padding.  Order of the sort: key only, stable. */
typedef struct lsb_elem {
  uint64_t key;
  uint64_t val;
} lsb_elem_t;

typedef struct lsb_ctx lsb_ctx_t;

/* Kernel / phase ids for lsb_get_kernel_stats(). */
#define LSB_K_UPSWEEP   0  /* per-chunk digit histogram (count)           */
#define LSB_K_SCAN      1  /* chunk x bucket exclusive scan               */
#define LSB_K_SCATTER   2  /* stable LDS-staged scatter (shuffle)         */
#define LSB_K_EXCHANGE  3  /* bucket-count allgather + element all-to-all */
#define LSB_K_PLACE     4  /* received runs -> final local slots          */
#define LSB_K_SORT      5  /* whole lsb_sort()                            */
#define LSB_K_SEGSORT   6  /* segmented local sort (LSB_OPT_HYBRID)       */
#define LSB_K_WIRE      7  /* the element all-to-all calls alone (RCCL,
                              host ops, or loopback device copies)        */
#define LSB_K_PLACE_TAIL 8 /* placement still running after the last slice
                              arrived (rank's stream waiting on it)       */
#define LSB_K_COUNT     9
#define LSB_MAX_RANKS  64  /* ranks of a context */

/* Options for lsb_set_option(). */
#define LSB_OPT_TIMING          0  /* 1: record HIP events around every kernel */
#define LSB_OPT_FORCE_EXCHANGE  1  /* 1: run the exchange path even when P == 1 */
#define LSB_OPT_SKIP_CONSTANT_DIGITS 2  /* 1 (default): lsb_sort skips every digit after
                                           the first on which all keys agree */
#define LSB_OPT_EXCHANGE_SLICES 3  /* 1..64 (default 5; 8 for radix_bits = 64): the all-to-all of a pass is cut into
                                      this many groups; each slice is placed while the next
                                      is in flight.  Per-digit exchanges cut each peer segment
                                      in halving parts (1/2, 1/4, ..., the last two equal), so
                                      the placement left after the wire is 1/2^(slices-1) of it;
                                      the whole-key exchange in equal parts */
#define LSB_OPT_EXCHANGE_P2P    4  /* RCCL contexts: 0 (default) ncclAllToAllv per slice,
                                      1 the same as grouped ncclSend/ncclRecv */
#define LSB_OPT_EXCHANGE_PEER   5  /* 1: exchange by direct stores into the owners' buffers
                                      (shmem_putmem / MPI_Put form; IPC-mapped across
                                      processes); no receive buffer, no placement pass.
                                      Opt-in: set on every rank before the first sort. */
#define LSB_OPT_ONESWEEP        6  /* 1 (default): lsb_sort reads each record once per
                                      local pass (P == 1, the per-digit exchange forms and
                                      the whole-key form's local sort): offsets by decoupled
                                      look-back, histograms carried from pass to pass (or
                                      counted by the exchange's placement); 0: reduce-then-
                                      scan (count, scan, scatter), as lsb_pass always is */
#define LSB_OPT_EXCHANGE_SELF   7  /* one-rank-per-process contexts: 1 sends the rank's own
                                      segment through the element collective as well
                                      (ncclAllToAllv / ncclSend+ncclRecv to itself, or the
                                      caller's alltoallv) and places it from the receive
                                      buffer like every other source; 0 (default) places it
                                      straight out of A.  Same output; lets a world of one
                                      carry the whole payload through RCCL (tests). */
#define LSB_OPT_ONESWEEP_SPLIT  8  /* single-read passes' LDS stage: 0 (default) chosen per
                                      sort from the first digit's histogram (one bucket over
                                      1/32 of a rank's records: the tile is staged in two
                                      halves, 3 workgroups per CU); 1 never split; 2 always
                                      split.  Same output. */
#define LSB_OPT_HYBRID          9  /* local sorts without an exchange between digits (P == 1,
                                      and each rank's block in the whole-key form): 0 (default)
                                      the LSD passes; 1 the hybrid: stable 8-bit passes on the k
                                      most significant varying bytes only (k = 4 at 2^30 records),
                                      the last of which also orders every segment (run of records
                                      equal on those bytes, ~0.25 records on average) by the whole
                                      key inside its tile, and k_segfix merges the segments split
                                      between two tiles; 2 the same passes, then a separate
                                      segmented sort (k_segsort) orders the segments.  Same output
                                      (the stable sort by key) from k passes over HBM instead of up
                                      to 8.  Skewed keys (one bucket of the first byte over 1/32 of
                                      the records) take the LSD passes; runs too long for k_segfix
                                      take k_segsort, and segments longer than 64 records
                                      (kSegMax) make the sort redo the kept input by the LSD
                                      passes.  Needs a third record buffer. */
#define LSB_OPT_EXCHANGE_GATHER 10 /* per-digit exchange forms with single-read local passes:
                                      1 (default) every exchange but the last only counts
                                      the next byte as the records arrive, and the next local
                                      pass reads its tiles from where they arrived (the
                                      receive buffer, the rank's own segment in A) through
                                      the plan's piece table: no placement pass (k_place's
                                      16 B of writes per record) before it; 0 places every
                                      exchange.  Same output. */
#define LSB_OPT_FAIL_ONESWEEP   11 /* tests (fault injection): n >= 1 makes the n-th k_onesweep
                                      launch from now (the chunked exchange's chunk passes
                                      included) fail with LSB_ERR_HIP before it is queued, as a
                                      failed launch would; 0 (default) off.  The context stays
                                      usable: its buffers keep their roles and the next sort
                                      starts from the records in A (the input, or after an
                                      exchange's local pass a permutation of it).  lsb_sort
                                      returns any error only once every rank's streams are
                                      idle. */
#define LSB_OPT_REGION_FIRST    12 /* P == 1 sorts of >= 2^27 records by the LSD passes:
                                      1 (default) the first pass takes no histogram read: it
                                      writes each (digit, sub-array) class of records into a
                                      slot range of its own, sized with slack over a uniform
                                      class (A and B hold 1.6 % more slots at 2^30), and the
                                      second pass reads that layout back to a dense one.  A
                                      2^20-record sample sends skewed or structured low bytes
                                      to the usual start (a histogram read), and a range that
                                      overflows all the same makes the sort start over from
                                      its input.  0: every sort starts with the histogram
                                      read.  Same output. */
#define LSB_OPT_EXCHANGE_CHUNKS 13 /* radix_bits = 16 exchanges (P > 1 or forced; RCCL or loopback):
                                      C = 2, 4 or 8 sends each digit's records in C chunks of
                                      its low byte while the high-byte pass runs chunk by chunk
                                      (chunk k's records on the wire during chunk k + 1's pass;
                                      mpi/mpi_lsbsort.cpp:481-577 runs localShuffle, then the
                                      whole exchange).  One read after the low-byte pass counts
                                      the digit first.  0 (default; the
                                      environment's LSB_EXCHANGE_CHUNKS sets a context's start
                                      value) sends after the whole pass.  Same output. */

#define LSB_OPT_PACK_VALUES     14 /* P == 1 LSD sorts that start with the regional pass
                                      (LSB_OPT_REGION_FIRST): 1 (default) when no value of the
                                      2^20-record sample needs more than 32 bits (the reference's
                                      values are global indices), the passes hand each other
                                      12-byte records {key, low word of the value}: the first
                                      pass packs, the last writes 16-byte records again, and the
                                      sort moves 200 instead of 256 bytes per record.  The first
                                      pass checks every value; one that does not fit makes the
                                      sort start over from its input with whole records, and
                                      later sorts of the context do not try again.  0: never
                                      pack.  2 (tests): pack without consulting the sample or
                                      earlier sorts.  Same output (lsb_get_last_records says
                                      which form ran).  The environment's LSB_PACK_VALUES sets
                                      a context's start value. */

/* ---- geometry: DistributedArray::create (mpi/mpi_lsbsort.cpp:144-149) ---- */
int64_t lsb_per_rank(int64_t n_total, int num_ranks);            /* ceil(n/P) */
int64_t lsb_here(int64_t n_total, int num_ranks, int rank);      /* clamp(n - r*per, 0, per) */

/* ---- lifecycle ---------------------------------------------------------- */
/* One process, `num_ranks` logical ranks; rank r lives on device dev_ids[r]
 * (dev_ids == NULL: every rank on device 0).  Up to 64 ranks.
 * radix_bits is the width of the digit the ranks exchange on: 8 (256
 * buckets, 8 passes) or 16 (65536 buckets, 4 passes: the reference's own
 * RADIX, mpi/mpi_lsbsort.cpp:21).  On device every digit is sorted by
 * stable 8-bit local passes (a 16-bit digit = low byte, then high byte), so
 * the output is the same for both; 16 halves the all-to-alls when P > 1.
 * radix_bits = 64 makes the whole key one digit: each rank sorts its block
 * (all 8 local passes), then ONE all-to-all moves every record to its owner,
 * which merges the P sorted runs in rank order (lsb_plan_merge).  Same
 * output again; one exchange per sort instead of 64 / radix_bits.
 * Device memory per rank: lsb_rank_footprint (A and B here; R, the receive
 * buffer, at the first exchange or hybrid sort; record buffers of >= 1 GiB
 * are whole 1 GiB VMM pieces).  While its placement probe runs
 * (lsb_get_placement) a rank alone on its device holds K - 2 more record
 * buffers for a moment: by default K = 4 for buffers of >= 4 GiB, as many as
 * fit in half the free memory at that moment (2^30 records: 34 GiB more for
 * ~0.2 s); LSB_PLACEMENT_CANDIDATES = K sets K (0: no probe; at most 8,
 * within 90 % of the free memory). */
int  lsb_create(lsb_ctx_t** ctx, int64_t n_total, int num_ranks,
                const int* dev_ids, int radix_bits);
/* HIP devices this process can see (hipGetDeviceCount; 0 when there is
 * none).  For a binding that maps one rank per GPU, e.g. the mySort stub of
 * INTEGRATION.md (rank r on device r % count). */
int  lsb_device_count(int* count);
/* RCCL bootstrap: rank 0 calls this and ships the bytes to the other ranks
 * (bench.py uses torch.distributed; hip_lsbsort uses a pipe). */
int  lsb_get_unique_id(unsigned char id[LSB_UNIQUE_ID_BYTES]);
/* One process per GPU: this process is `rank` of `num_ranks`, on `dev_id`. */
int  lsb_create_rank(lsb_ctx_t** ctx, int64_t n_total, int num_ranks, int rank,
                     int dev_id, int radix_bits,
                     const unsigned char id[LSB_UNIQUE_ID_BYTES]);
/* One process per rank with caller-supplied collectives instead of RCCL (any
 * transport: MPI, gloo, sockets).  The runtime runs exactly the per-rank code
 * of lsb_create_rank; around each collective it synchronizes its stream and
 * stages the data through host memory.  All pointers are host pointers, all
 * sizes are bytes; every rank makes the same calls in the same order (as
 * MPI requires); a callback returns 0 on success.  `user` is passed back. */
typedef struct lsb_comm_ops {
  void* user;
  /* recv[r * bytes .. (r+1) * bytes) = send of rank r */
  int (*allgather)(void* user, const void* send, void* recv, size_t bytes);
  /* MPI_Alltoallv on bytes */
  int (*alltoallv)(void* user, const void* send, const size_t* send_bytes,
                   const size_t* send_displs, void* recv, const size_t* recv_bytes,
                   const size_t* recv_displs);
  /* *value = min over ranks */
  int (*allreduce_min_i64)(void* user, int64_t* value);
  int (*barrier)(void* user);
} lsb_comm_ops_t;
int  lsb_create_rank_ops(lsb_ctx_t** ctx, int64_t n_total, int num_ranks, int rank,
                         int dev_id, int radix_bits, const lsb_comm_ops_t* ops);
void lsb_destroy(lsb_ctx_t* ctx);
int  lsb_set_option(lsb_ctx_t* ctx, int option, int64_t value);
/* Ranks owned by this context: [*first_rank, *first_rank + *num_local). */
int  lsb_local_ranks(const lsb_ctx_t* ctx, int* first_rank, int* num_local);

/* ---- data --------------------------------------------------------------- */
/* PCG input init (mpi/mpi_lsbsort.cpp:650-656), on device: for every local
 * rank r and every one of its `per` slots i: key = i-th output of pcg64(r),
 * val = r*per + i.  Untimed in the reference; untimed here. */
int  lsb_generate(lsb_ctx_t* ctx);
/* Same stream, other key distributions (build-defined):
 *   LSB_DIST_UNIFORM         == lsb_generate
 *   LSB_DIST_ZIPF, param = s key = mix64(k), k = floor of a power law with
 *                            exponent s on [1, 2^30], drawn by inverse CDF
 *                            from the same pcg64(r) draw (heavy duplicates).
 * lsb_verify() recomputes keys with the distribution last generated. */
#define LSB_DIST_UNIFORM 0
#define LSB_DIST_ZIPF    1
int  lsb_generate_ex(lsb_ctx_t* ctx, int dist, double param);
/* Host <-> A of a local rank, slots [off, off+cnt) of that rank's per slots. */
int  lsb_copy_in(lsb_ctx_t* ctx, int rank, int64_t off, int64_t cnt, const lsb_elem_t* host);
int  lsb_copy_out(lsb_ctx_t* ctx, int rank, int64_t off, int64_t cnt, lsb_elem_t* host);

/* ---- caller-owned device columns ------------------------------------------ */
/* A caller on the GPU (the reference's mySort stub, a torch pipeline) holds
 * separate key and value arrays on the device.  lsb_load_columns turns them
 * into the records of A, lsb_store_columns turns A back into columns; no byte
 * passes through host memory.
 * A key's raw bits are mapped to the unsigned 64-bit key the passes sort by:
 *   LSB_KEY_U64               identity
 *   LSB_KEY_I64               bit 63 flipped
 *   LSB_KEY_F64               sign set: ~bits; else bit 63 flipped
 *   LSB_KEY_U32 / I32 / F32   the same rules at 32 bits, zero-extended
 * LSB_ORDER_DESCENDING (flags bit 0) complements that key within the key's
 * width.  32-bit keys keep a zero upper word in both orders, so lsb_sort
 * skips their four upper digits.  The sort is the stable ascending sort of
 * the mapped key: equal keys keep their input order in both directions (the
 * rule of a stable descending sort, e.g. torch.sort(stable=True,
 * descending=True)).
 * Float keys sort in the order of their bits, ascending:
 *   1. NaNs with the sign bit set
 *   2. -inf
 *   3. finite values, -0.0 before +0.0
 *   4. +inf
 *   5. NaNs with the sign bit clear
 * (descending: the reverse).  Keys come back bit for bit, NaN payloads and
 * the sign of zero included. */
#define LSB_KEY_U64 0
#define LSB_KEY_I64 1
#define LSB_KEY_F64 2
#define LSB_KEY_U32 3
#define LSB_KEY_I32 4
#define LSB_KEY_F32 5
#define LSB_ORDER_DESCENDING 1
/* The mapping itself and its inverse: pure host functions, no device needed
 * (the kernels run the same code).  A 32-bit type takes and returns its key
 * in the low word.  0 on an unknown type or flag. */
uint64_t lsb_key_encode(uint64_t bits, int key_type, int flags);
uint64_t lsb_key_decode(uint64_t key, int key_type, int flags);
/* Load: A[off + i] = {encode(keys_dev[i]), value} for i in [0, cnt), slots of
 * local rank `rank` as for lsb_copy_in.  The value is vals_dev[i]: 8 bytes
 * raw (val_bytes 8) or 4 bytes zero-extended (val_bytes 4); with vals_dev
 * NULL and val_bytes 0 it is the record's global index rank * per + off + i,
 * the reference's value (mpi/mpi_lsbsort.cpp:650-656), so the sorted values
 * are the stable argsort.
 * Store: the inverse, keys_dev[i] = decode(A[off + i].key) and vals_dev[i] =
 * the value (val_bytes 8) or its low word (val_bytes 4).  Either output may
 * be NULL (val_bytes 0 with vals_dev NULL), not both.
 * Both calls are stateless: the caller gives the store the key_type and flags
 * it gave the load; the context remembers neither.  They work alike in every
 * kind of context.  cnt == 0 returns LSB_OK and launches nothing.
 * Streams: the call waits for the rank's own stream, runs one kernel on it
 * and returns once that kernel has finished.  It does not wait for any other
 * stream: the caller's arrays must be ready (written, or free to overwrite)
 * when the call is made.
 * LSB_ERR_INVALID, before any kernel is launched: bad rank or range; unknown
 * key type; unknown flag bits; val_bytes not 0, 4 or 8, or disagreeing with
 * vals_dev; a pointer not aligned to its element size; a pointer that
 * hipPointerGetAttributes does not report as device or managed memory of the
 * rank's device (a pageable host pointer never reaches a kernel); a range
 * [ptr, ptr + cnt * element size) that leaves the allocation
 * hipMemGetAddressRange reports for ptr.  Columns aligned to 16 bytes are
 * moved in 16-byte accesses, others element by element, with equal results.
 * lsb_check_sorted works on loaded data (it compares the mapped keys);
 * lsb_verify does not (PCG input only). */
int  lsb_load_columns(lsb_ctx_t* ctx, int rank, int64_t off, int64_t cnt,
                      const void* keys_dev, int key_type,
                      const void* vals_dev, int val_bytes, int flags);
int  lsb_store_columns(lsb_ctx_t* ctx, int rank, int64_t off, int64_t cnt,
                       void* keys_dev, int key_type,
                       void* vals_dev, int val_bytes, int flags);

/* ---- ordering by several columns: rekey by a gathered column --------------- */
/* A sorted array whose values are input indices is a permutation.  The rekey
 * replaces each record's key with the key of that input row in another
 * column, so that the next (stable) lsb_sort orders by that column and keeps
 * the order reached so far among its equal keys: an LSD sort over columns,
 * least significant column first (ORDER BY a, b, c; numpy.lexsort).
 *
 * lsb_rekey_columns: for every slot i in [0, here(rank)) of local rank
 * `rank`, with v = A[i].val (all 64 bits, unsigned), the record becomes
 * {lsb_key_encode(keys_dev[v], key_type, flags), v}.  keys_dev is a column of
 * n_col typed keys on the rank's device, read as lsb_load_columns reads its
 * keys (all six key types, LSB_ORDER_DESCENDING).  The value is not changed.
 * The rekey is in place: A and B do not swap, slots [here, per) are not
 * touched, and each thread rewrites only the records it read.
 * In a world of several ranks the values are global input indices, so every
 * rank needs the WHOLE column (all n_col = n keys) on its own device, not its
 * block of it; worlds whose columns are not replicated are out of scope.
 *
 * lsb_rekey_index: the record becomes {v / divisor, v} (unsigned division),
 * no column involved.  divisor 1 restores "key = input index", so a following
 * lsb_sort returns the records to input order; divisor L keys each record by
 * its row of a row-major [R, L] array (sort by key, rekey by row, sort again:
 * every row sorted).
 *
 * Both calls are local, not collective, and work alike in every kind of
 * context.  here(rank) == 0 returns LSB_OK, launches nothing and does not
 * look at keys_dev.  Streams as lsb_load_columns: the call waits for the
 * rank's own stream, runs one kernel on it and returns once it has finished.
 * Both change the records, so they end the run plan, the select plan, the
 * search table and the join plan as lsb_load_columns does.
 * LSB_ERR_INVALID, before any kernel is launched and with A untouched: null
 * context or bad rank; unknown key type or flag bits; null keys_dev;
 * n_col <= 0; the pointer checks of lsb_load_columns on keys_dev over n_col
 * elements; divisor == 0.  LSB_ERR_STATE as lsb_sort, when an earlier failed
 * sort left the context unusable.
 * LSB_ERR_INVALID after the kernel, from lsb_rekey_columns, when some
 * record's value is >= n_col.  The kernel forms no address from such a value
 * and leaves that record as it was.  Afterwards every value and every slot is
 * intact; the keys of the records whose values are in range have already been
 * replaced.  The caller still holds its columns and the indices are still in
 * the records, so it can rekey again (with the right column, or with
 * lsb_rekey_index).  The error word is 8 bytes of scratch every rank has from
 * its creation. */
int  lsb_rekey_columns(lsb_ctx_t* ctx, int rank, const void* keys_dev, int64_t n_col,
                       int key_type, int flags);
int  lsb_rekey_index(lsb_ctx_t* ctx, int rank, uint64_t divisor);

/* ---- runs of equal keys --------------------------------------------------- */
/* What a caller does next with a sorted array: the distinct keys, how often
 * each occurs, where each group starts and which input record was its first
 * (dedup, histogram, group-by offsets, unique with index and counts), on the
 * device and across rank boundaries.
 * A run is a maximal range of adjacent global positions (rank 0's slots, then
 * rank 1's, ...) whose records have the same mapped unsigned 64-bit key.  On a
 * sorted array the runs are the groups of equal keys; the definition does not
 * need sortedness (it is unique_consecutive on any array).
 * Equality is equality of the key's bits: -0.0 and +0.0 are two keys, NaNs
 * with different payloads are different keys, and every NaN equals itself.
 * A run belongs to the rank that holds its first record; its count includes
 * its records on later ranks.
 *
 * lsb_plan_runs: the host planner, pure host code.  summary[r][0..3] of a
 * non-empty rank r (here(r) > 0; the words of empty ranks are ignored):
 *   first  key of its first record        last   key of its last record
 *   inner  number of i in [1, here) with key[i] != key[i-1]
 *   lead   the smallest such i, or here when there is none
 * Out, per rank (P entries each, zeros for empty ranks): head0[r] = 1 when a
 * run starts at r's first slot; runs[r] = inner + head0, the runs r owns;
 * bases[r] = the global index of r's first run (exclusive prefix sum of
 * runs); ends[r] = the global position one past the end of the run that holds
 * r's last record; *total = the number of runs.  LSB_ERR_INVALID on a null
 * argument, n < 0, P outside [1, 64], or a summary no array gives: lead < 1,
 * lead > here, inner > here - 1, (inner == 0) != (lead == here), or
 * inner == 0 with first != last.
 *
 * lsb_count_runs: collective in one-rank-per-process contexts (every rank
 * calls it, in the same order as its other collectives, as lsb_check_sorted).
 * Reads every local rank's A once, gathers the ranks' summaries, runs the
 * planner and keeps the plan in the context.  *total = the number of runs of
 * the whole array; runs[P] and bases[P] (either may be NULL) as above, for
 * every rank of the world.  n == 0: *total = 0, nothing is launched.  The
 * first call allocates 12 bytes per 4096 records of scratch on each rank.
 * The plan stays valid until lsb_generate, lsb_generate_ex, lsb_copy_in,
 * lsb_load_columns, lsb_rekey_columns, lsb_rekey_index, lsb_sort, lsb_pass,
 * lsb_label_runs or lsb_scan_runs is called.  In a one-rank-per-process world
 * lsb_copy_in, lsb_load_columns and the two rekeys are local calls and drop the
 * plan of the calling process only, while the other ranks' plans depend on
 * its records (a run's count reaches into later ranks): after any rank has
 * changed its records, every rank calls lsb_count_runs again before its next
 * lsb_store_runs.
 * LSB_ERR_INVALID: null context or total.  LSB_ERR_STATE: an earlier sort
 * left the context unusable (as lsb_sort), or the gathered summaries are not
 * those of an array.
 *
 * lsb_store_runs: local, no collective; needs a valid plan (LSB_ERR_STATE
 * otherwise).  Reads rank's A once more and writes, for the j-th run that
 * starts on this rank, j in [0, runs[rank]):
 *   keys_dev[j]   = decode(key) with key_type and flags as lsb_store_columns
 *   starts_dev[j] = the global position of the run's first record
 *   counts_dev[j] = the run's length (records on later ranks included)
 *   firsts_dev[j] = the first record's value (val_bytes 8) or its low word
 *                   (val_bytes 4); after a stable sort of a load without
 *                   values this is the input index of the key's first
 *                   occurrence
 * Every output is optional and at least one is required; counts_dev needs
 * starts_dev (the counts are the differences of the starts); firsts_dev NULL
 * goes with val_bytes 0.  cap = the elements every given output holds.
 * The outputs must not overlap one another.
 * *runs (may be NULL) = runs[rank]; cap < runs[rank] returns LSB_ERR_INVALID
 * with *runs set and nothing written.  A rank that owns no run returns LSB_OK
 * and launches nothing; nothing would be written, so its output pointers are
 * not examined (the pointer checks below do not apply to it).
 * LSB_ERR_INVALID, before any kernel is launched: bad rank, cap < 0, unknown
 * key type or flag bits, val_bytes not 0, 4 or 8 or disagreeing with
 * firsts_dev, no output, counts_dev without starts_dev, and for each output
 * the pointer checks of lsb_load_columns over cap elements (alignment, device
 * memory of the rank's device, range inside its allocation), and two outputs
 * whose ranges of cap elements share a byte.
 * LSB_ERR_STATE after the kernel: A was changed behind the library's back
 * since lsb_count_runs (a tile's heads differ from those counted); the
 * outputs are then unspecified, nothing is written outside them, and the
 * plan is dropped.
 * Streams as lsb_store_columns: the call waits for the rank's stream, runs on
 * it and returns when done. */
int  lsb_plan_runs(int64_t n_total, int num_ranks, const uint64_t* summary,
                   int* head0, int64_t* runs, int64_t* bases, int64_t* ends, int64_t* total);
int  lsb_count_runs(lsb_ctx_t* ctx, int64_t* total, int64_t* runs, int64_t* bases);
int  lsb_store_runs(lsb_ctx_t* ctx, int rank, int64_t cap, void* keys_dev, int key_type, int flags,
                    int64_t* starts_dev, int64_t* counts_dev, void* firsts_dev, int val_bytes,
                    int64_t* runs);

/* Reductions over the runs' values: the group-by's last step, one number per
 * run from the records' 64 value bits, across rank boundaries (a run's
 * records on later ranks, whole middle ranks included, are part of it).
 * op: LSB_REDUCE_SUM, LSB_REDUCE_MIN or LSB_REDUCE_MAX.  val_type names how
 * the 64 value bits are read: LSB_KEY_U64, LSB_KEY_I64 or LSB_KEY_F64; the
 * 32-bit types are refused (a value loaded with val_bytes 4 is zero-extended:
 * reduce it as LSB_KEY_U64).
 *   SUM  U64 and I64 add modulo 2^64 (the same bits).  F64 adds doubles: for
 *        given (n, P, records) the result is bit-identical from call to call
 *        (the code fixes the order and the association of the additions; no
 *        atomics, no timing); it may differ between values of P.  The
 *        identity combined with is -0.0 (0x8000000000000000), the additive
 *        identity of IEEE doubles: a run of -0.0 values sums to -0.0.
 *   MIN / MAX  in the order lsb_key_encode defines for the type, the float
 *        order above included: -0.0 is below +0.0, a NaN with the sign clear
 *        is the maximum of its run, one with the sign set its minimum.  The
 *        result is one of the run's values, bit for bit.
 * The identity of (op, val_type): SUM 0 (U64, I64) or -0.0 (F64); MIN the
 * value whose encoding is all ones; MAX the value whose encoding is 0.
 *
 * lsb_plan_run_tails: the host planner, pure host code.  summary as for
 * lsb_plan_runs (and checked the same way); lead[s] = op over the values of
 * rank s's leading run, its first summary[s][lead] records (ignored for
 * empty ranks and for ranks whose first slot starts a run).  tail[r] = op, in
 * rank order, over lead[s] of the ranks after r whose leading run continues
 * r's last run (the chain lsb_plan_runs walks for ends[r]); the identity when
 * there is none, and for empty ranks.  LSB_ERR_INVALID on a null argument,
 * n < 0, P outside [1, 64], an unknown op, a value type outside {U64, I64,
 * F64}, or a summary lsb_plan_runs refuses.
 *
 * lsb_plan_reduce: collective in one-rank-per-process contexts, like
 * lsb_count_runs; needs a valid run plan (LSB_ERR_STATE otherwise).  Every
 * non-empty local rank whose first slot does not start a run reduces its
 * leading run on its own stream; the words are gathered (8 bytes per rank),
 * lsb_plan_run_tails runs on them, and the tails, op and val_type are kept in
 * the context.  An unknown op or type returns LSB_ERR_INVALID before anything
 * is launched or gathered.  n == 0 returns LSB_OK and launches nothing.  The
 * reduce plan dies with the run plan; a later lsb_plan_reduce replaces it.
 * The first call allocates, on each rank, 8 bytes per 4096 records and 64 KiB
 * of scratch (freed with the context; lsb_rank_footprint models neither this
 * nor lsb_count_runs' scratch).
 *
 * lsb_store_reduce: local, no collective; needs a reduce plan (LSB_ERR_STATE
 * otherwise).  Reads rank's A once more and writes out_dev[j] = op over the
 * values of all records of the j-th run that starts on this rank, j in
 * [0, runs[rank]): the indices of lsb_store_runs.  out_dev is a column of cap
 * 8-byte elements.  *runs (may be NULL) = runs[rank]; cap < runs[rank]
 * returns LSB_ERR_INVALID with *runs set and nothing written.  A rank that
 * owns no run returns LSB_OK, launches nothing and does not examine out_dev.
 * LSB_ERR_INVALID, before any kernel is launched: bad rank, cap < 0, null
 * out_dev, and the pointer checks of lsb_load_columns over cap 8-byte
 * elements.  LSB_ERR_STATE after the kernel: A was changed behind the
 * library's back since lsb_count_runs; the outputs are then unspecified,
 * nothing is written outside [0, runs[rank]) and both plans are dropped.
 * Streams as lsb_store_runs. */
#define LSB_REDUCE_SUM 0
#define LSB_REDUCE_MIN 1
#define LSB_REDUCE_MAX 2
int  lsb_plan_run_tails(int64_t n_total, int num_ranks, const uint64_t* summary,
                        int op, int val_type, const uint64_t* lead, uint64_t* tail);
int  lsb_plan_reduce(lsb_ctx_t* ctx, int op, int val_type);
int  lsb_store_reduce(lsb_ctx_t* ctx, int rank, int64_t cap, void* out_dev, int64_t* runs);

/* A run id per record: which group a row belongs to.  The calls above answer
 * per run; this one labels every record with the global index of the run
 * that holds it, id = bases[owner] + j, the index under which lsb_store_runs
 * and lsb_store_reduce write that run.  It is the inverse of unique, the
 * codes of factorize, DENSE_RANK() on a sorted array, a segment id, and the
 * index that broadcasts a run's aggregate back to its records.
 * For the record at slot i of rank r:
 *   id = bases[r] + (the heads of rank r at or below i, slot 0 among them
 *        exactly when head0[r]) - 1
 * so the records of a leading run that began on an earlier rank (in front of
 * the rank's first head, head0[r] == 0) get bases[r] - 1, and a rank that lies
 * wholly inside one run (runs[r] == 0) gets that one id throughout.
 *   LSB_LABEL_KEEP      the record becomes {key, id}: the order stays, the
 *                       value is replaced
 *   LSB_LABEL_BY_VALUE  the record becomes {key = its old value, value = id}
 *
 * lsb_label_runs: local, no collective; needs a valid run plan (LSB_ERR_STATE
 * otherwise) and uses only what lsb_count_runs left behind.  One call labels
 * every local rank of the context, each on its own stream, and returns when
 * all of them are done.  It changes the records, so a successful call ends
 * the run plan and the reduce plan like the calls lsb_count_runs lists; in a
 * one-rank-per-process world every process calls it once, before the next
 * collective.  An unknown mode returns LSB_ERR_INVALID before anything is
 * launched and leaves the plan as it was.  n == 0 returns LSB_OK and launches
 * nothing; empty local ranks launch nothing.
 * Not in place: each rank's labelled records are written to its second record
 * buffer, which then becomes A, as in a pass of the sort (the first buffer's
 * contents are unspecified afterwards).  No scratch is allocated.
 * LSB_ERR_STATE after the kernels: a local rank's A was changed behind the
 * library's back since lsb_count_runs (a tile's heads differ from those
 * counted).  Then no local rank is labelled, every A is what it was, and the
 * plans are dropped.
 * The inverse in input order: load the keys with lsb_load_columns and
 * vals_dev NULL (the values are the global input indices), lsb_sort,
 * lsb_count_runs, lsb_label_runs(LSB_LABEL_BY_VALUE), lsb_sort again.  Slot i
 * of rank r then holds {r * per + i, the id of input record r * per + i}, and
 * lsb_store_columns(keys_dev NULL, vals_dev, val_bytes 8 or 4) writes the
 * rank's block of the inverse column.  The index keys are below n, so the
 * second sort skips their constant upper digits.  The call does not check
 * what the values are: with other values BY_VALUE sorts by those. */
#define LSB_LABEL_KEEP     0
#define LSB_LABEL_BY_VALUE 1
int  lsb_label_runs(lsb_ctx_t* ctx, int mode);

/* A scan within the runs: one number per record, from the records in front of
 * it in its run (a running sum, min or max of a group's values:
 * groupby().cumsum(), a window aggregate OVER (PARTITION BY key ORDER BY
 * position); the record's place inside its group: cumcount, ROW_NUMBER(); the
 * group's start: RANK()), across tile and rank boundaries.  Runs, key equality
 * and the global position order are those of "runs of equal keys" above.  For
 * the record at global position g whose run starts at global position s <= g:
 *   LSB_SCAN_SUM, LSB_SCAN_MIN, LSB_SCAN_MAX (== LSB_REDUCE_*)
 *                    op over the values of the positions s .. g, the 64 value
 *                    bits read as val_type (LSB_KEY_U64, LSB_KEY_I64 or
 *                    LSB_KEY_F64), as for lsb_plan_reduce
 *   LSB_SCAN_COUNT   g - s: the run's records in front of this one (0-based;
 *                    cumcount, ROW_NUMBER() - 1).  No operand: val_type must
 *                    be LSB_KEY_U64
 *   LSB_SCAN_START   s: the global position of the run's first record
 *                    (RANK() - 1 on a sorted array; starts_dev[id] of
 *                    lsb_store_runs).  No operand: val_type must be LSB_KEY_U64
 * The rules of the reductions carry over: integer sums wrap modulo 2^64; MIN
 * and MAX follow lsb_key_encode's order, the float order included, and return
 * one of the run's values bit for bit; the F64 SUM combines with the identity
 * -0.0 (a run of -0.0 values scans to -0.0), the code fixes the order and the
 * association of every addition (no float atomics, no timing), and for given
 * (n, P, records) the result is bit-identical from call to call; it may differ
 * between values of P.  The association: with t the record's 4096-record tile
 * of its rank, result = ((carry[rank] + in(t)) + scan inside t), where in(t)
 * is what the rank's earlier tiles add to the run open at t's first record
 * (folded forwards in tile order) and carry[rank] what the earlier ranks add
 * to the rank's leading run (folded forwards in rank order); a part is
 * present only where no head lies between it and the record.
 * The last record of a run carries what lsb_store_reduce writes for that run,
 * bit for bit for MIN, MAX and the integer SUM; for the F64 SUM the two agree
 * within the rounding of two summation orders (the reduction folds backwards
 * from the run's tail, the scan forwards).
 *
 * lsb_plan_run_carries: the host planner, pure host code, the mirror of
 * lsb_plan_run_tails.  summary as for lsb_plan_runs (and checked the same
 * way); trail[s] = op over the operands of rank s's records from its last
 * head on (all its records when it has none; slot 0 is a head when a run
 * starts there); ignored for empty ranks.  carry[r] = the left fold, in
 * increasing rank order and from the identity, of trail[s] over the ranks
 * s < r whose last run is r's leading run: the walk goes down from r - 1,
 * skips empty ranks, stops at a rank whose last key is not r's first key,
 * takes the rank, and stops after a rank that has a head of its own (inner
 * > 0, or a run starts at its slot 0).  The identity for empty ranks and for
 * ranks whose slot 0 starts a run.  For COUNT and START every record's
 * operand is 1 and the fold the u64 sum: carry[r] = the records of r's
 * leading run on earlier ranks.  LSB_ERR_INVALID on a null argument, n < 0, P
 * outside [1, 64], an unknown op, a value type outside {U64, I64, F64}, COUNT
 * or START with a type other than U64, or a summary lsb_plan_runs refuses.
 *
 * lsb_plan_scan: collective in one-rank-per-process contexts, like
 * lsb_plan_reduce; needs a valid run plan (LSB_ERR_STATE otherwise).  An
 * unknown op or type returns LSB_ERR_INVALID before anything is launched or
 * gathered.  n == 0 returns LSB_OK and launches nothing.  Every non-empty
 * local rank, on its own stream, reads its A once (what each tile leaves open
 * at its end), then scans those words in one workgroup (what each tile takes
 * in, and the rank's trail word); the trail words are gathered (8 bytes per
 * rank), lsb_plan_run_carries runs on them, and the carries, op and val_type
 * are kept in the context.  LSB_ERR_STATE after the gather when a local
 * rank's A was changed behind the library's back since lsb_count_runs; the
 * run plan is then dropped.  The scan plan dies with the run plan; a later
 * lsb_plan_scan replaces it; it is independent of the reduce plan, and a
 * caller may hold both.  The first call allocates, on each rank, 16 bytes per
 * 4096 records and 16 bytes more of scratch (freed with the context;
 * lsb_rank_footprint does not model it, as it does not the reduce scratch).
 *
 * lsb_store_scan: local, no collective; needs a scan plan (LSB_ERR_STATE
 * otherwise).  Reads rank's A once more and writes out_dev[i] = the result of
 * the record at slot i, i in [0, here(rank)): a column of cap 8-byte elements
 * in slot order.  A is untouched and the plans stay: several ops can be
 * planned and stored one after another from one lsb_count_runs.  *count (may
 * be NULL) = here(rank); cap < here(rank) returns LSB_ERR_INVALID with *count
 * set and nothing written.  An empty rank returns LSB_OK, launches nothing
 * and does not examine out_dev.  LSB_ERR_INVALID, before any kernel is
 * launched: bad rank, cap < 0, null out_dev, and the pointer checks of
 * lsb_load_columns over cap 8-byte elements.  The column is written in 8-byte
 * accesses, adjacent lanes writing adjacent elements (a record's result stays
 * in the lane that loaded the record), whatever its alignment beyond 8 bytes.
 * LSB_ERR_STATE after the kernel: A was changed behind the library's back
 * since lsb_count_runs; the output is then unspecified, nothing is written
 * outside [0, here(rank)) and the plans are dropped.  Streams as
 * lsb_store_runs.
 *
 * lsb_scan_runs: the records form, lsb_label_runs with the scan's result in
 * place of the run id.  LSB_LABEL_KEEP: each record becomes {key, result};
 * LSB_LABEL_BY_VALUE: {key = its old value, value = result}.  Local, no
 * collective; needs a scan plan (LSB_ERR_STATE otherwise).  One call covers
 * every local rank, each on its own stream, into its second record buffer,
 * which then becomes A.  A successful call ends the run, reduce, scan and
 * select plans.  An unknown mode returns LSB_ERR_INVALID and leaves the plans
 * as they were.  n == 0 returns LSB_OK.  LSB_ERR_STATE after the kernels: a
 * local rank's A was changed since lsb_count_runs; then no rank is swapped,
 * every A is what it was, and the plans are dropped.
 * cumcount or rank in input order, the recipe of the inverse: load the keys
 * with vals_dev NULL, lsb_sort, lsb_count_runs, lsb_plan_scan(LSB_SCAN_COUNT
 * or LSB_SCAN_START, LSB_KEY_U64), lsb_scan_runs(LSB_LABEL_BY_VALUE), lsb_sort
 * again, lsb_store_columns(keys_dev NULL, vals_dev). */
#define LSB_SCAN_SUM   0
#define LSB_SCAN_MIN   1
#define LSB_SCAN_MAX   2
#define LSB_SCAN_COUNT 3
#define LSB_SCAN_START 4
int  lsb_plan_run_carries(int64_t n_total, int num_ranks, const uint64_t* summary,
                          int op, int val_type, const uint64_t* trail, uint64_t* carry);
int  lsb_plan_scan(lsb_ctx_t* ctx, int op, int val_type);
int  lsb_store_scan(lsb_ctx_t* ctx, int rank, int64_t cap, void* out_dev, int64_t* count);
int  lsb_scan_runs(lsb_ctx_t* ctx, int mode);

/* ---- the k-th key and the first k + 1 records, without a sort -------------- */
/* The commonest question that needs no full sort: the k-th smallest key
 * (median, percentile, threshold) and the k best records (top-k with their
 * input indices), across rank boundaries.
 * The array is the global one: rank 0's slots, then rank 1's, ...  It may be
 * in any order; sortedness is neither needed nor used.  Keys are the mapped
 * unsigned 64-bit keys of lsb_key_encode: a descending load selects from the
 * top, and floats follow the order given above.
 * For 0 <= k < n let pivot be the key the stable sort would put at global
 * position k, below the number of records with key < pivot and equal the
 * number with key == pivot, so below <= k < below + equal.  The selection of
 * k is the first k + 1 records of the stable sort, as a set: every record
 * with key < pivot, and the first k + 1 - below records with key == pivot in
 * global position order (with index values: the lowest input indices among
 * the ties).
 *
 * lsb_plan_select: the host planner, pure host code.  count = k + 1 records
 * are wanted; below[r] and equal[r] are rank r's records below and equal to
 * the pivot.  With E = count - sum(below), rank r gives
 * min(equal[r], max(0, E - sum of equal[s] over s < r)) of its equal records,
 * the rule of lsb_plan_merge: equal keys keep rank order.  Out, P entries
 * each: take[r] = below[r] + that; bases[r] = the exclusive prefix sum of
 * take.  LSB_ERR_INVALID on a null argument, n < 0, P outside [1, 64], a
 * negative entry, below[r] + equal[r] > here(r), or counts that do not
 * bracket count: sum(below) < count <= sum(below) + sum(equal) is false.
 *
 * lsb_select: collective in one-rank-per-process contexts, like
 * lsb_count_runs: every rank calls it with the same k.  An MSD radix select:
 * a round reads each rank's candidates once and counts one key byte of those
 * whose upper bits equal the prefix found so far; the ranks' 256 counts are
 * gathered (258 words per rank), the bucket that holds the wanted rank is
 * chosen and the buckets in front of it are added to below.  Round one reads
 * A, takes the top byte and also reduces the span of the keys; a byte on
 * which all keys of the array agree costs no round after that (all-equal keys
 * finish after one read, 32-bit key types do their four upper bytes in round
 * one).  A rank whose count in the chosen bucket is at most half of what its
 * source holds copies those records into its B in the next round's read and
 * reads only them from then on.
 * Every A stays bit for bit as it was.  Each rank's B is scratch: its
 * contents are unspecified afterwards, as after lsb_label_runs.
 * *key = pivot, *below and *equal = the counts over the whole array; take[P]
 * and bases[P] as lsb_plan_select gives them for count = k + 1, for every
 * rank of the world.  Every output may be NULL.
 * The context keeps the plan (pivot and the per-rank counts) until
 * lsb_generate, lsb_generate_ex, lsb_copy_in, lsb_load_columns,
 * lsb_rekey_columns, lsb_rekey_index, lsb_sort,
 * lsb_pass, lsb_label_runs or lsb_scan_runs is called: the calls that end a run plan, and
 * the note on one-rank-per-process worlds there applies unchanged.  The run
 * plan and the reduce plan are left alone, and lsb_count_runs,
 * lsb_store_runs, lsb_plan_reduce and lsb_store_reduce leave this plan alone.
 * LSB_ERR_INVALID, before anything is launched or gathered: null context, or
 * k outside [0, n) (n == 0: every k).  LSB_ERR_STATE: an earlier sort left
 * the context unusable (as lsb_sort), or the gathered counts are not those of
 * an array (A was changed during the call).
 * The first call allocates, on each rank, 259 + 258 P words of tables (the
 * gather area only in one-rank-per-process contexts), freed with the context;
 * nothing sized by the records.
 *
 * lsb_store_select: local, no collective; needs a select plan (LSB_ERR_STATE
 * otherwise).  Reads rank's A twice more (counts per 4096-record tile, then
 * the write) and writes the rank's part of the selection, take[rank] records,
 * compacted, in slot order (not in key order: a caller that wants the k + 1
 * records ordered sorts them): for the j-th selected record of the rank
 *   keys_dev[j] = decode(key) with key_type and flags as lsb_store_columns
 *   vals_dev[j] = the value (val_bytes 8) or its low word (val_bytes 4)
 * Either output may be NULL (val_bytes 0 with vals_dev NULL), not both.
 * cap = the elements every given output holds.  *count (may be NULL) =
 * take[rank]; cap < take[rank] returns LSB_ERR_INVALID with *count set and
 * nothing written.  A rank that takes nothing returns LSB_OK, launches
 * nothing and does not examine the pointers.
 * LSB_ERR_INVALID, before any kernel is launched: bad rank, cap < 0, unknown
 * key type or flag bits, val_bytes not 0, 4 or 8 or disagreeing with
 * vals_dev, no output, and for each output the pointer checks of
 * lsb_load_columns over cap elements.  Columns aligned to 16 bytes are
 * written in 16-byte accesses, others element by element, with equal results.
 * LSB_ERR_STATE after the kernels: A was changed behind the library's back
 * since lsb_select (a tile's counts differ on the second read, or the rank's
 * totals are not the plan's); the outputs are then unspecified, nothing is
 * written outside [0, take[rank]) and the plan is dropped.
 * The first call allocates 20 bytes per 4096 records of scratch on the rank.
 * Streams as lsb_store_runs.
 *
 * lsb_get_last_select: what the last lsb_select of the context ran: *rounds =
 * its histogram rounds, each with its gather; *records_read = the records
 * its kernels read on this context's local ranks, summed: reads of A and
 * reads of candidates in B.  Either may be NULL. */
int  lsb_plan_select(int64_t n_total, int num_ranks, int64_t count,
                     const int64_t* below, const int64_t* equal, int64_t* take, int64_t* bases);
int  lsb_select(lsb_ctx_t* ctx, int64_t k, uint64_t* key, int64_t* below, int64_t* equal,
                int64_t* take, int64_t* bases);
int  lsb_store_select(lsb_ctx_t* ctx, int rank, int64_t cap, void* keys_dev, int key_type, int flags,
                      void* vals_dev, int val_bytes, int64_t* count);
int  lsb_get_last_select(lsb_ctx_t* ctx, int* rounds, int64_t* records_read);

/* ---- searching the sorted records: lower and upper bound, match count ------ */
/* A question about a second column against the sorted one: where would this
 * key go, is it present, and how often (searchsorted, bucketize, isin; the
 * probe side of a sort-merge join or a dictionary lookup).
 * Take a local rank whose A is sorted by mapped key: after lsb_sort, or any A
 * for which lsb_check_sorted holds.  queries_dev is a column of m typed keys
 * on that rank's device, read with key_type and flags as lsb_load_columns
 * reads its keys.  With e_i = lsb_key_encode(queries_dev[i], key_type, flags):
 *   LSB_SEARCH_LOWER   c_i = the number of the rank's records with key <  e_i
 *   LSB_SEARCH_UPPER   c_i = the number with key <= e_i
 *   LSB_SEARCH_COUNT   c_i = the number with key == e_i (UPPER - LOWER, in one
 *                      call and one kernel)
 * out_dev[i] = c_i; with LSB_SEARCH_ADD or-ed into mode, out_dev[i] += c_i.
 *
 * Across ranks: the global array (rank 0's slots, then rank 1's, ...) is
 * sorted, so the global lower bound of a query is the sum of the ranks' c_i,
 * and the same holds for UPPER and COUNT.  That is the whole cross-rank story:
 * a loopback caller calls once per local rank, with LSB_SEARCH_ADD from the
 * second on; a one-rank-per-process caller whose ranks hold the same queries
 * adds the ranks' columns with an all-reduce of its own.  The call is local,
 * not collective, and needs no plan from another call.  Two early-outs make a
 * rank that a query does not fall into cheap: a query not above the rank's
 * first key gives LOWER 0, a query above its last key gives here(rank),
 * neither with a probe of a tile (UPPER alike: below the first key 0, not
 * below the last here(rank)).
 *
 * Order: equality and order are those of the mapped unsigned key.  -0.0 is
 * below +0.0; NaNs sort at both ends by sign, and a NaN equals only its own
 * bit pattern; LSB_ORDER_DESCENDING searches an array that was loaded
 * descending.  This is deliberately not torch.searchsorted's or numpy's float
 * behaviour (where -0.0 == +0.0 and every NaN sorts last).
 *
 * Edges: m == 0 returns LSB_OK and launches nothing.  On a rank that holds no
 * record every c_i is 0: zeros are written without LSB_SEARCH_ADD, nothing is
 * touched with it.
 * Unsorted A is the caller's error and is not detected.  The result is then
 * unspecified, but every c_i lies in [0, here(rank)], no record outside the
 * rank's here(rank) slots is read and nothing outside out_dev[0, m) is
 * written: the probe indices are bounded by construction, not by the data.
 *
 * The first search of a rank after a change of its A reads the key of every
 * 4096th record into a table (8 bytes per 4096 records of scratch, allocated
 * at the rank's first search and freed with the context; lsb_rank_footprint
 * does not model it, as for the other scratch).  The table is kept until
 * lsb_generate, lsb_generate_ex, lsb_copy_in, lsb_load_columns,
 * lsb_rekey_columns, lsb_rekey_index, lsb_sort,
 * lsb_pass, lsb_label_runs or lsb_scan_runs is called.  lsb_select leaves A
 * bit for bit and uses B only, so it keeps the table; so do the calls that
 * only read A.  A query then costs a binary search of that table and at most
 * 12 probes of one 4096-record tile.
 *
 * LSB_ERR_INVALID, before anything is launched: null context, bad rank,
 * m < 0, unknown key type or flag bits, unknown mode bits, and with m > 0 a
 * null pointer, the pointer checks of lsb_load_columns on both columns
 * (aligned to the element, 8 bytes for out_dev; device memory of the rank's
 * device; the range inside its allocation), or query and output ranges that
 * share a byte.  LSB_ERR_STATE: an earlier sort left the context unusable (as
 * lsb_sort).
 * Streams as lsb_store_columns: the call waits for the rank's stream, runs on
 * it and returns when the column is written. */
#define LSB_SEARCH_LOWER 0
#define LSB_SEARCH_UPPER 1
#define LSB_SEARCH_COUNT 2
#define LSB_SEARCH_ADD   4   /* or-ed into mode: out_dev[i] += c_i */
int  lsb_search(lsb_ctx_t* ctx, int rank, int64_t m, const void* queries_dev,
                int key_type, int flags, int mode, int64_t* out_dev);

/* ---- the matches themselves: value lookup and matched pairs ---------------- */
/* What lsb_search counts, handed back: for each query the value stored with
 * its key (lsb_lookup: dictionary decode, a dimension-table fetch, index_of),
 * and all (query index, record) pairs with equal keys, materialised
 * (lsb_join_count + lsb_store_join: the sort-merge join whose probe side
 * lsb_search is).
 * The preconditions are those of lsb_search: the rank's A is sorted by mapped
 * key; queries_dev is a column of m typed keys on the rank's device, read with
 * key_type and flags as lsb_load_columns reads its keys.  Equality is equality
 * of the mapped key's bits: -0.0 and +0.0 are two keys, a NaN equals only its
 * own bit pattern, a descending load is searched with LSB_ORDER_DESCENDING.
 * Unsorted A is the caller's error and is not detected; the results are then
 * unspecified, but no record outside the rank's here(rank) slots is read and
 * nothing is written outside the given outputs.
 * With e_i = lsb_key_encode(queries_dev[i], key_type, flags), for one rank:
 *   lower_i = the number of the rank's records with key <  e_i
 *   c_i     = the number of the rank's records with key == e_i
 * All three calls are local, not collective, and use the streams as
 * lsb_search does: a call waits for the rank's stream, runs on it and returns
 * when its outputs are written.  They share lsb_search's table of every 4096th
 * key, built by whichever of them comes first after a change of A.
 *
 * lsb_lookup: one kernel, no plan.  For every i with c_i > 0, vals_dev[i] =
 * the value of record lower_i, 8 bytes (val_bytes 8) or its low word
 * (val_bytes 4): the first match in the rank, after a stable sort of an index
 * load the lowest input index; and found_dev[i] = 1 when found_dev is given.
 * For every i with c_i == 0 neither element is touched: the caller prefills
 * its default and zeros.  At least one of vals_dev and found_dev is required;
 * vals_dev NULL goes with val_bytes 0.  Each thread writes only the elements
 * of its own query: no atomics.
 * Across ranks the global array is sorted, so the global first match lies on
 * the lowest rank that has one: a caller that calls its local ranks from the
 * last to the first ends up with the global first match in vals_dev (a later
 * call overwrites an earlier one's element; first to last leaves the last
 * rank's first match instead).
 * m == 0 returns LSB_OK and launches nothing; a rank without records touches
 * nothing.
 *
 * lsb_join_count: computes lower_i and c_i for every query and the exclusive
 * prefix sum off_i of the c_i (off_m = *total), and keeps them as the rank's
 * join plan in scratch the library owns: no intermediate column is left to the
 * caller, so nothing the expansion indexes with can be changed from outside.
 * counts_dev (optional, int64[m]) = c_i, what LSB_SEARCH_COUNT gives.  *total
 * (may be NULL) = the rank's pairs.  Everything is 64-bit: *total may exceed
 * 2^32.  Three kernels (count with a sum per 4096 queries, a scan of those
 * sums by one workgroup, the offsets), none of which waits for another
 * workgroup, and one 8-byte read of the total.
 * Scratch: 16 bytes per query plus 8 bytes per 4096 queries, allocated at the
 * rank's first call, regrown when a later m is larger, freed with the context;
 * lsb_rank_footprint does not model it, as for the other scratch.  A failed
 * allocation returns LSB_ERR_NOMEM and leaves the rank without a plan.
 * Plans are per rank: a new lsb_join_count on a rank replaces that rank's plan
 * only.  A plan lasts as the table of lsb_search does: until lsb_generate,
 * lsb_generate_ex, lsb_copy_in, lsb_load_columns, lsb_rekey_columns,
 * lsb_rekey_index, lsb_sort, lsb_pass,
 * lsb_label_runs or lsb_scan_runs is called; lsb_select and the calls that
 * only read A keep it.
 * m == 0 or a rank without records: *total = 0 and a valid plan of zero pairs;
 * no kernel is launched (counts_dev, when given, is zeroed).
 *
 * lsb_store_join: needs the rank's join plan (LSB_ERR_STATE otherwise).  For
 * output slot o in [0, total): i = the query with off_i <= o < off_{i+1},
 * j = o - off_i, p = lower_i + j, and
 *   left_dev[o]  = query_base + i
 *   right_dev[o] = the value of record p (val_bytes 8) or its low word (4)
 *   pos_dev[o]   = rank * per + p, the record's global position
 * Each output is optional, at least one is required; right_dev NULL goes with
 * val_bytes 0.  cap = the elements every given output holds.  The rank's pairs
 * come out ordered by query index, then by record position: after a stable
 * sort of an index load, by left index, then by right input index.
 * *count (may be NULL) = total; cap < total returns LSB_ERR_INVALID with
 * *count set and nothing written; total == 0 returns LSB_OK, launches nothing
 * and does not examine the pointers.  The plan stays valid: a second store,
 * for instance with other outputs, gives the same pairs.
 * One kernel, a workgroup per 2048 outputs: it finds the queries whose pairs
 * meet its outputs by two searches of off, then every output finds its query
 * among them, so the work per output is logarithmic whatever the skew (one
 * query with a million matches, the next thousand with none).
 * The pairs of the ranks are disjoint and their union is the join with the
 * whole array: that is the whole cross-rank story, as for lsb_search.
 *
 * LSB_ERR_INVALID, before anything is launched: null context, bad rank, m < 0
 * or cap < 0, unknown key type or flag bits, val_bytes not 0, 4 or 8 or
 * disagreeing with its pointer, no output, a null queries pointer with m > 0,
 * the pointer checks of lsb_load_columns on every given column (m elements
 * each; the outputs of lsb_store_join cap elements each), and any two given
 * columns of one call that share a byte (queries against an output, or two
 * outputs).  LSB_ERR_STATE: an earlier sort left the context unusable (as
 * lsb_sort). */
int  lsb_lookup(lsb_ctx_t* ctx, int rank, int64_t m, const void* queries_dev, int key_type, int flags,
                void* vals_dev, int val_bytes, uint8_t* found_dev);
int  lsb_join_count(lsb_ctx_t* ctx, int rank, int64_t m, const void* queries_dev, int key_type, int flags,
                    int64_t* counts_dev, int64_t* total);
int  lsb_store_join(lsb_ctx_t* ctx, int rank, int64_t cap, int64_t query_base, int64_t* left_dev,
                    void* right_dev, int val_bytes, int64_t* pos_dev, int64_t* count);

/* ---- the hot path ------------------------------------------------------- */
/* == mySort(A, B): all 64/radix_bits passes; result in A.  Asynchronous
 * with respect to the host except for the per-pass count exchange when
 * P > 1 and one 16-byte key-span read after the first pass; call
 * lsb_sync() to wait.
 * The first pass's count kernel also reduces the OR of all keys and of their
 * complements (all-gathered when P > 1).  A later digit on which every key
 * agrees is skipped: its stable pass and its exchange are the identity, so
 * the output is unchanged (keys < 2^32 take 4 of 8 passes).  Uniform 64-bit
 * keys run every pass.  LSB_OPT_SKIP_CONSTANT_DIGITS = 0 turns this off. */
int  lsb_sort(lsb_ctx_t* ctx);
/* What the last lsb_sort ran: 8-bit local passes, exchanges (0 when P == 1
 * and not forced) and the key bits that vary (~0 when skipping is off). */
int  lsb_get_last_sort(lsb_ctx_t* ctx, int* local_passes, int* exchanges,
                       uint64_t* varying_bits);
/* How the last lsb_sort began (LSB_OPT_REGION_FIRST): LSB_FIRST_COUNT a
 * histogram read (k_subhist / k_upsweep) before the first pass, or none ran;
 * LSB_FIRST_REGIONAL the regional first pass; LSB_FIRST_REGIONAL_REDONE the
 * regional pass overflowed a region, and the sort started over from its
 * input with the histogram read.  With LSB_FIRST_REGIONAL the varying bits
 * of lsb_get_last_sort are those of a 2^20-record sample (every byte varies
 * there, so every pass runs). */
#define LSB_FIRST_COUNT           0
#define LSB_FIRST_REGIONAL        1
#define LSB_FIRST_REGIONAL_REDONE 2
int  lsb_get_first_pass(lsb_ctx_t* ctx, int* form);
/* The records the last lsb_sort's passes handed each other
 * (LSB_OPT_PACK_VALUES): LSB_RECORDS_FULL 16-byte records throughout;
 * LSB_RECORDS_PACKED 12-byte records between the first and the last pass;
 * LSB_RECORDS_PACKED_REDONE the first pass packed, met a value over 32 bits,
 * and the sort started over from its input with 16-byte records.
 * If a pass of a packed sort fails to launch, lsb_sort leaves whole records
 * (a permutation of the input) in A as after any error; should even that
 * fail, lsb_sort returns LSB_ERR_STATE until lsb_generate loads A again. */
#define LSB_RECORDS_FULL          0
#define LSB_RECORDS_PACKED        1
#define LSB_RECORDS_PACKED_REDONE 2
int  lsb_get_last_records(lsb_ctx_t* ctx, int* form);
/* Records per tile of the last lsb_sort's packed middle passes (12-byte
 * records in and out, LSB_RECORDS_PACKED): 5120 where every sub-array of the
 * next pass holds at least a tile (from 61441 records on), else 4096; the
 * environment's LSB_PACKED_TILE = 4096 | 4608 | 5120, read when the context
 * is created, sets the size asked for.  0 when no such pass ran. */
int  lsb_get_last_packed_tile(lsb_ctx_t* ctx, int* records);
/* Records per tile of each local pass of the last lsb_sort, in pass order:
 * records[i] for i < *passes <= max_passes (0: that pass was no k_onesweep
 * launch).  In a packed sort whose middle passes take 5120, the first and
 * the last pass take 5120 too, and so does the pass that reads the regional
 * layout where the regions' slots are whole tiles of it (2^25, 2^29 and 2^30
 * records; not 2^26 to 2^28 nor below 2^25); the environment's
 * LSB_EDGE_TILES (1: the first pass, 2: the layout's pass, 4: the last;
 * default 7), read when the context is created, names the ones that may. */
int  lsb_get_last_pass_tiles(lsb_ctx_t* ctx, int* records, int max_passes, int* passes);
/* == globalShuffle(A, B, digit): one pass, result in A. */
int  lsb_pass(lsb_ctx_t* ctx, int digit);
int  lsb_sync(lsb_ctx_t* ctx);
/* lsb_sync, then (RCCL contexts) a device all-reduce across the ranks:
 * the MPI_Barrier around the timed region (mpi/mpi_lsbsort.cpp:688,693). */
int  lsb_barrier(lsb_ctx_t* ctx);

/* ---- checks ------------------------------------------------------------- */
/* Bit-exact check equivalent to the MPI verify (stable_sort + ==), in O(n)
 * on device, valid for PCG input from lsb_generate(): for every global i,
 * out[i].val < n, out[i].key == pcg64(val / per)[val % per] and
 * (key, val)[i] < (key, val)[i+1] strictly, across rank boundaries too.
 * Returns LSB_OK when all hold, LSB_ERR_VERIFY otherwise; *first_bad gets
 * the smallest failing global index (or -1).  PCG input only: records from
 * lsb_copy_in or lsb_load_columns fail it (lsb_check_sorted is the check for
 * those). */
int  lsb_verify(lsb_ctx_t* ctx, int64_t* first_bad);
/* == checkSorted (shmem/shmem_lsbsort.cpp:180-219): key order inside every
 * rank and across rank boundaries.  *sorted = 1 / 0. */
int  lsb_check_sorted(lsb_ctx_t* ctx, int* sorted);

/* ---- measurement -------------------------------------------------------- */
/* With LSB_OPT_TIMING on: launches recorded and their summed device time
 * (HIP events on the stream each kernel runs on) since the last reset. */
int  lsb_get_kernel_stats(lsb_ctx_t* ctx, int kernel_id, int64_t* launches, double* total_ms);
int  lsb_reset_kernel_stats(lsb_ctx_t* ctx);
/* Elements one launch of the scatter kernel processed, summed like the stats. */
int  lsb_get_scatter_elems(lsb_ctx_t* ctx, int64_t* elems);
/* The same stats per local pass (the reference times only the
 * whole sort, mpi/mpi_lsbsort.cpp:688-699).  Pass p is the p-th 8-bit local
 * pass a sort ran (0-based; constant digits are skipped, so p counts passes
 * that ran, not digits; lsb_pass files a digit's passes under its own index).
 * A sort's first count read is filed under its first pass, and an exchange
 * (all-gather, plan, all-to-all, placement or merge) under the local pass
 * before it.  Summed over the launches since the last reset, every local
 * rank included: *shift = the pass's key shift (-1: no launch), *launches /
 * *elems = scatter launches and the records they processed, and the device
 * milliseconds of its count kernels (k_subhist / k_upsweep + k_scan), its
 * scatter (k_onesweep or k_scatter), its exchange and its placement. */
#define LSB_MAX_PASSES 16
int  lsb_get_pass_stats(lsb_ctx_t* ctx, int pass, int* shift, int64_t* launches, int64_t* elems,
                        double* ms_count, double* ms_scatter, double* ms_exchange, double* ms_place);
/* Element payload this context handed to its all-to-all collective
 * (ncclAllToAllv, grouped ncclSend/ncclRecv or the caller's alltoallv) since
 * the context was created: calls, bytes sent (self segment included when
 * LSB_OPT_EXCHANGE_SELF is on) and the largest one call sent.  Loopback
 * contexts (device copies) report 0. */
int  lsb_get_exchange_bytes(lsb_ctx_t* ctx, int64_t* calls, int64_t* bytes, int64_t* max_call_bytes);
/* The exchange steps since the last lsb_reset_kernel_stats, this context's
 * local ranks summed: the xGMI side of a pass that SURVEY §8(d) asks to
 * report beside the local passes (the reference's all-to-all and placement,
 * mpi/mpi_lsbsort.cpp:562-575).  Bytes are the element collective's payload
 * (ncclAllToAllv / grouped send-recv / the caller's alltoallv; the self
 * segment only with LSB_OPT_EXCHANGE_SELF; loopback device copies count 0),
 * per peer.  Times need LSB_OPT_TIMING (HIP events):
 *   wire_ms       the all-to-all calls on the rank's stream (LSB_K_WIRE);
 *   plan_ms       counts all-gather + device plan + tile descriptors, or the
 *                 whole key's splitter search (LSB_K_EXCHANGE);
 *   place_ms      the placement stream: k_place, or the merge (LSB_K_PLACE);
 *   place_tail_ms placement still running once the last slice had arrived
 *                 (LSB_K_PLACE_TAIL): the part not overlapped with the wire.
 * place_bytes: algorithmic bytes of the placement kernels: 32 per placed
 * record (16 read + 16 written), 16 per record a count-only k_place reads,
 * 32 per record per merge level. */
typedef struct lsb_exchange_stats {
  int64_t exchanges;                   /* exchange steps (digits, or 1 per whole-key sort) */
  int64_t calls;                       /* all-to-all calls (slices) */
  int64_t sent_bytes[LSB_MAX_RANKS];   /* payload to each destination rank */
  int64_t recv_bytes[LSB_MAX_RANKS];   /* payload from each source rank */
  double wire_ms, plan_ms, place_ms, place_tail_ms;
  int64_t place_bytes;
  int64_t placed_records;              /* records written by the placement */
  int64_t counted_records;             /* records only counted (gathered passes follow) */
} lsb_exchange_stats_t;
int  lsb_get_exchange_stats(lsb_ctx_t* ctx, lsb_exchange_stats_t* out);
/* Per local pass (as lsb_get_pass_stats files an exchange under the local
 * pass before it): payload bytes handed to the all-to-all, its wire time and
 * the placement tail, summed since the last reset. */
int  lsb_get_pass_exchange(lsb_ctx_t* ctx, int pass, int64_t* bytes, double* wire_ms,
                           double* place_tail_ms);

/* How the local rank's record buffers A and B were placed.  Record buffers of
 * at least 1 GiB are built from 1 GiB physical pieces (HIP virtual memory;
 * LSB_RECORD_ALLOC=malloc: hipMalloc) -- except in an RCCL context created
 * after an earlier RCCL context of the process released such buffers: such
 * contexts returned wrong data over pieces mapped at reused addresses (a
 * HIP VMM fault, reproduced with a copy kernel alone), so those take
 * hipMalloc'd buffers (LSB_RCCL_VMM=1: pieces regardless).
 * Such a buffer can still be a slow
 * pass destination as a whole, so a rank whose buffers hold
 * >= 4 GiB and that shares its device with no other rank of the context
 * tries 4 candidate buffers (LSB_PLACEMENT_CANDIDATES = K: K of them, at
 * most 8, for buffers of >= 1 GiB; 0: none) when three fit in half the free
 * memory (90 % when K is set).  Each candidate is timed once as the
 * destination of one k_onesweep pass over uniform keys (the speed that
 * differs); the two fastest destinations are kept and every other candidate
 * is freed as soon as it loses, so the probe holds at most one record buffer
 * more than A and B (see lsb_rank_footprint).  candidates = the candidates
 * timed, 0: no probe ran.  Milliseconds per pass as a destination: the mean
 * of the chosen two, the mean of the first two allocated (what a plain
 * allocation would have kept) and the slowest candidate. */
int  lsb_get_placement(lsb_ctx_t* ctx, int rank, int* candidates, double* chosen_ms,
                       double* first_pair_ms, double* worst_ms);

/* ---- device memory ------------------------------------------------------ */
/* Device bytes one rank of a context lsb_create(n_total, num_ranks,
 * radix_bits) holds (pure host arithmetic, no device needed): A and B (each
 * `per` records, rounded up to whole 1 GiB pieces when built from them), the
 * receive buffer R when with_recv (any exchange: num_ranks > 1 or forced; the
 * hybrid local sort), the single-read passes' look-back rows (4 B per bucket
 * per 4096-record tile), the gathered passes' tile descriptors (exchanges),
 * and the count and plan tables.  *probe_bytes: what the placement probe
 * (by default 4 candidates for buffers of >= 4 GiB; LSB_PLACEMENT_CANDIDATES,
 * read from the environment now) holds on top while it runs, at most: one
 * record buffer (a rank
 * that shares its device with another rank of its context runs none); 0 when
 * no probe would run.  A model of
 * init_rank's allocations, checked against the device's own free-memory
 * count by tests/test_footprint_gpu.py. */
int  lsb_rank_footprint(int64_t n_total, int num_ranks, int radix_bits, int with_recv,
                        int64_t* bytes, int64_t* probe_bytes);

/* Free and total device memory of device dev (hipMemGetInfo). */
int  lsb_device_memory(int dev, int64_t* free_bytes, int64_t* total_bytes);

/* ---- build --------------------------------------------------------------- */
/* "sha256=<digest of the sources the library was built from> host=<build
 * host> rccl=<ncclGetVersion of the RCCL loaded>" (static string).  tests/
 * compare the digest with the tree. */
const char* lsb_build_info(void);

/* ---- host planner (pure host code; used by the runtime when P > 1) ------- */
/* Given hist[s*nbuckets + b] = number of elements of bucket b that rank s
 * holds after its local stable pass (bucket order), compute rank `rank`'s
 * side of the exchange under the digit-major, rank-minor global order of
 * copyCountsToGlobalCounts / exclusiveScan (mpi/mpi_lsbsort.cpp:350,378,401):
 *   send_counts[q], send_displs[q]  elements of my bucket-ordered buffer for q
 *   recv_counts[s], recv_displs[s]  elements arriving from s, in s order
 *   place_off[s*nbuckets + b]       local slot = place_off[s][b] + recv index
 * All arrays are caller-allocated (P or P*nbuckets int64). */
int  lsb_plan_exchange(int64_t n_total, int num_ranks, int rank, int nbuckets,
                       const int64_t* hist,
                       int64_t* send_counts, int64_t* send_displs,
                       int64_t* recv_counts, int64_t* recv_displs,
                       int64_t* place_off);

/* The same plan computed by the device kernels the runtime uses (it keeps
 * place_off on the GPU and fetches only the 2P counts); host arrays in and
 * out, on device `dev_id`.  For testing the two planners against each other. */
int  lsb_plan_exchange_device(int dev_id, int64_t n_total, int num_ranks, int rank, int nbuckets,
                              const int64_t* hist,
                              int64_t* send_counts, int64_t* send_displs,
                              int64_t* recv_counts, int64_t* recv_displs,
                              int64_t* place_off);

/* Plan of the whole-key exchange (radix_bits = 64), host side.  After every
 * rank has sorted its block on the whole key, let k*_q be the key at global
 * position T_q = q * per (q = 1 .. P-1, the q with T_q < n) and
 *   below[s * (P-1) + q-1] = #records of rank s with key <  k*_q
 *   upto [s * (P-1) + q-1] = #records of rank s with key <= k*_q
 * (entries of targets T_q >= n are ignored).  Records of equal key keep rank
 * order, so source s's cut at T_q is below + min(equal, what T_q still
 * needs after the lower ranks).  Rank `rank` then sends its sorted range
 * [cut_q, cut_{q+1}) to q and receives [cut_rank, cut_{rank+1}) of every s:
 * counts and displacements (records) as for lsb_plan_exchange.  This is the
 * rule the runtime applies to the all-gathered counts of its device splitter
 * search (k_split_*), replacing copyCountsToGlobalCounts / exclusiveScan /
 * copyStartsFromGlobalStarts (mpi/mpi_lsbsort.cpp:327-479) for a digit of
 * 2^64 buckets.  LSB_ERR_INVALID when the counts do not bracket a target. */
int  lsb_plan_merge(int64_t n_total, int num_ranks, int rank, const int64_t* below,
                    const int64_t* upto, int64_t* send_counts, int64_t* send_displs,
                    int64_t* recv_counts, int64_t* recv_displs);

const char* lsb_strerror(int code);

#ifdef __cplusplus
}
#endif

#endif /* LSB_H */
