"""Python front end of the MI355X-native distributed LSD radix sort.

A thin ctypes binding of the C ABI in ``include/lsb.h`` (library
``distributed-lsb_amd/build/liblsb.so``), mirroring the reference's own
seams so tests read like the reference program:

  ==========================  ==============================================
  reference                   here
  ==========================  ==============================================
  DistributedArray::create    ``World(n, ranks)`` / ``World.rank(...)``
  (mpi/mpi_lsbsort.cpp:137)   (block partition per = ceil(n/P))
  PCG init (:643-666)         ``World.generate()``
  mySort(A, B) (:580-585)     ``World.my_sort()``   (alias ``mySort``)
  globalShuffle (:481-577)    ``World.global_shuffle(d)`` (alias ``globalShuffle``)
  verify (:710-738)           ``World.verify()``
  checkSorted (shmem :180)    ``World.check_sorted()``
  A.print(10) (:171-200)      ``World.print_lines("A", 10)``
  ==========================  ==============================================

A caller that holds keys and values on the GPU (1-D torch CUDA tensors; typed
keys, either order, values or argsort) uses ``sort(keys, values)``, or
``World.load_columns`` / ``World.store_columns`` around ``my_sort()``; the
groups of equal keys come from ``unique(keys)``, or ``World.count_runs`` /
``World.store_runs`` after the sort, and one number per group from the value
column (sum, min, max) from ``group_reduce(keys, values)``, or
``World.plan_reduce`` / ``World.store_reduce``, and the group of every record
(unique's inverse, a dense rank) from ``unique(keys, return_inverse=True)`` or
``dense_rank(keys)``, or ``World.label_runs``, and one number per record from
the records in front of it in its group (a running sum, min or max, its place
in the group, the group's start) from ``group_scan(keys, values)``,
``cumcount(keys)`` and ``rank(keys)``, or ``World.plan_scan`` /
``World.store_scan`` / ``World.scan_runs``.  The k-th key and the k best
records need no sort: ``kth(keys, k)`` and ``topk(keys, k)``, or ``World.select`` /
``World.store_select``.  A second column is searched against the sorted one
(where each key would go, whether and how often it occurs) with
``searchsorted(keys, queries)``, ``count_of`` and ``isin``, or ``World.search``;
the matches themselves come from ``lookup(keys, values, queries)`` (the value
stored with each query's key) and ``join(left_keys, right_keys)`` (all pairs of
equal keys), or ``World.lookup`` / ``World.join_count`` / ``World.store_join``.
torch is imported only inside those functions.  A process that uses them imports torch before the first call into
this module: the library then binds to the HIP runtime torch brought, and both
see the same device memory.

Errors from the library raise :class:`LsbError` (the reference aborts on
MPI errors, mpi/mpi_lsbsort.cpp:17-19).  There is no CPU fallback: if the
HIP library is missing or no GPU is present, calls fail loudly.
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import Optional, Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(PKG_DIR)
# LSB_LIBRARY: another build of the same ABI (A/B timing of kernel variants).
LIB_PATH = os.environ.get("LSB_LIBRARY") or os.path.join(ROOT_DIR, "build", "liblsb.so")
HARNESS_PATH = os.path.join(ROOT_DIR, "build", "hip_lsbsort")
HEADER_PATH = os.path.join(os.path.dirname(ROOT_DIR), "include", "lsb.h")

ELEM_DTYPE = np.dtype([("key", "<u8"), ("val", "<u8")])
UNIQUE_ID_BYTES = 128

LSB_OK = 0
LSB_ERR_VERIFY = 5
DIST_UNIFORM, DIST_ZIPF = 0, 1
K_UPSWEEP, K_SCAN, K_SCATTER, K_EXCHANGE, K_PLACE, K_SORT, K_SEGSORT, K_WIRE, K_PLACE_TAIL = range(9)
KERNEL_NAMES = ("upsweep", "scan", "scatter", "exchange", "place", "sort", "segsort", "wire", "place_tail")
MAX_RANKS = 64
OPT_TIMING, OPT_FORCE_EXCHANGE, OPT_SKIP_CONSTANT_DIGITS, OPT_EXCHANGE_SLICES, OPT_EXCHANGE_P2P = 0, 1, 2, 3, 4
OPT_EXCHANGE_PEER = 5
OPT_ONESWEEP = 6
OPT_EXCHANGE_SELF = 7
OPT_ONESWEEP_SPLIT = 8
OPT_HYBRID = 9
OPT_EXCHANGE_GATHER = 10
OPT_FAIL_ONESWEEP = 11
OPT_REGION_FIRST = 12
OPT_EXCHANGE_CHUNKS = 13
OPT_PACK_VALUES = 14
RECORDS_FULL, RECORDS_PACKED, RECORDS_PACKED_REDONE = 0, 1, 2
FIRST_COUNT, FIRST_REGIONAL, FIRST_REGIONAL_REDONE = 0, 1, 2
MAX_PASSES = 16
# Key forms of caller-owned columns (LSB_KEY_*, LSB_ORDER_DESCENDING).
KEY_U64, KEY_I64, KEY_F64, KEY_U32, KEY_I32, KEY_F32 = range(6)
ORDER_DESCENDING = 1
# Reductions over the runs' values (LSB_REDUCE_*).
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = range(3)
# What a labelled record becomes (LSB_LABEL_*): {key, id} or {old value, id}.
LABEL_KEEP, LABEL_BY_VALUE = 0, 1
# Scans within the runs (LSB_SCAN_*): the reductions' ops per record, its place
# in its run, and its run's first global position.
SCAN_SUM, SCAN_MIN, SCAN_MAX, SCAN_COUNT, SCAN_START = range(5)
# What a search counts per query (LSB_SEARCH_*): the records below it, not
# above it, equal to it; SEARCH_ADD or-ed in adds to the output column.
SEARCH_LOWER, SEARCH_UPPER, SEARCH_COUNT, SEARCH_ADD = 0, 1, 2, 4


class LsbError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = _lib().lsb_strerror(code).decode()
        super().__init__(f"{where}: lsb error {code}: {msg}")
        self.code = code


_L = None


# -- host collectives (lsb_comm_ops_t) -------------------------------------
_ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_size_t)
_ALLTOALLV = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                              ctypes.POINTER(ctypes.c_size_t))
_ALLREDUCE_MIN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))
_BARRIER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)


class ExchangeStats(ctypes.Structure):
    """lsb_exchange_stats_t."""
    _fields_ = [("exchanges", ctypes.c_int64), ("calls", ctypes.c_int64),
                ("sent_bytes", ctypes.c_int64 * 64), ("recv_bytes", ctypes.c_int64 * 64),
                ("wire_ms", ctypes.c_double), ("plan_ms", ctypes.c_double), ("place_ms", ctypes.c_double),
                ("place_tail_ms", ctypes.c_double), ("place_bytes", ctypes.c_int64),
                ("placed_records", ctypes.c_int64), ("counted_records", ctypes.c_int64)]


class CommOps(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allgather", _ALLGATHER), ("alltoallv", _ALLTOALLV),
                ("allreduce_min_i64", _ALLREDUCE_MIN), ("barrier", _BARRIER)]


def _bytes_at(ptr, n):
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr))


def _make_comm_ops(comm, P):
    """lsb_comm_ops_t whose callbacks call the Python object `comm`."""
    def guard(fn):
        def wrapped(*a):
            try:
                fn(*a)
                return 0
            except Exception as e:  # a failed collective is an error code, not a crash
                print(f"lsbsort comm callback failed: {e!r}", file=sys.stderr)
                return 1
        return wrapped

    def allgather(_u, send, recv, nbytes):
        _bytes_at(recv, nbytes * P)[:] = comm.allgather(_bytes_at(send, nbytes).copy())

    def alltoallv(_u, send, sc, sd, recv, rc, rd):
        scn = [sc[i] for i in range(P)]
        sdn = [sd[i] for i in range(P)]
        rcn = [rc[i] for i in range(P)]
        rdn = [rd[i] for i in range(P)]
        send_len = max([d + c for d, c in zip(sdn, scn) if c] or [0])
        recv_len = max([d + c for d, c in zip(rdn, rcn) if c] or [0])
        comm.alltoallv(_bytes_at(send, send_len), scn, sdn, _bytes_at(recv, recv_len), rcn, rdn)

    def allreduce_min(_u, v):
        v[0] = int(comm.allreduce_min(int(v[0])))

    def barrier(_u):
        comm.barrier()

    keep = (_ALLGATHER(guard(allgather)), _ALLTOALLV(guard(alltoallv)),
            _ALLREDUCE_MIN(guard(allreduce_min)), _BARRIER(guard(barrier)))
    ops = CommOps(None, *keep)
    return ops, keep


def _lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"HIP library {LIB_PATH} is not built; run `make -C distributed-lsb_amd` "
                "(or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        i64, i32, vp, cp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
        P64 = ctypes.POINTER(ctypes.c_int64)
        sig = {
            "lsb_per_rank": (i64, [i64, i32]),
            "lsb_here": (i64, [i64, i32, i32]),
            "lsb_create": (i32, [ctypes.POINTER(vp), i64, i32, ctypes.POINTER(ctypes.c_int), i32]),
            "lsb_get_unique_id": (i32, [ctypes.c_char_p]),
            "lsb_device_count": (i32, [ctypes.POINTER(ctypes.c_int)]),
            "lsb_create_rank": (i32, [ctypes.POINTER(vp), i64, i32, i32, i32, i32, ctypes.c_char_p]),
            "lsb_create_rank_ops": (i32, [ctypes.POINTER(vp), i64, i32, i32, i32, i32,
                                          ctypes.POINTER(CommOps)]),
            "lsb_destroy": (None, [vp]),
            "lsb_set_option": (i32, [vp, i32, i64]),
            "lsb_get_last_sort": (i32, [vp, vp, vp, vp]),
            "lsb_get_first_pass": (i32, [vp, vp]),
            "lsb_get_last_records": (i32, [vp, vp]),
            "lsb_get_last_packed_tile": (i32, [vp, vp]),
            "lsb_get_last_pass_tiles": (i32, [vp, vp, i32, vp]),
            "lsb_local_ranks": (i32, [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
            "lsb_generate": (i32, [vp]),
            "lsb_generate_ex": (i32, [vp, i32, ctypes.c_double]),
            "lsb_copy_in": (i32, [vp, i32, i64, i64, vp]),
            "lsb_copy_out": (i32, [vp, i32, i64, i64, vp]),
            "lsb_key_encode": (ctypes.c_uint64, [ctypes.c_uint64, i32, i32]),
            "lsb_key_decode": (ctypes.c_uint64, [ctypes.c_uint64, i32, i32]),
            "lsb_load_columns": (i32, [vp, i32, i64, i64, vp, i32, vp, i32, i32]),
            "lsb_store_columns": (i32, [vp, i32, i64, i64, vp, i32, vp, i32, i32]),
            "lsb_rekey_columns": (i32, [vp, i32, vp, i64, i32, i32]),
            "lsb_rekey_index": (i32, [vp, i32, ctypes.c_uint64]),
            "lsb_plan_runs": (i32, [i64, i32, vp, vp, vp, vp, vp, P64]),
            "lsb_count_runs": (i32, [vp, P64, vp, vp]),
            "lsb_store_runs": (i32, [vp, i32, i64, vp, i32, i32, vp, vp, vp, i32, P64]),
            "lsb_plan_run_tails": (i32, [i64, i32, vp, i32, i32, vp, vp]),
            "lsb_plan_reduce": (i32, [vp, i32, i32]),
            "lsb_store_reduce": (i32, [vp, i32, i64, vp, P64]),
            "lsb_label_runs": (i32, [vp, i32]),
            "lsb_plan_run_carries": (i32, [i64, i32, vp, i32, i32, vp, vp]),
            "lsb_plan_scan": (i32, [vp, i32, i32]),
            "lsb_store_scan": (i32, [vp, i32, i64, vp, P64]),
            "lsb_scan_runs": (i32, [vp, i32]),
            "lsb_plan_select": (i32, [i64, i32, i64, vp, vp, vp, vp]),
            "lsb_select": (i32, [vp, i64, ctypes.POINTER(ctypes.c_uint64), P64, P64, vp, vp]),
            "lsb_store_select": (i32, [vp, i32, i64, vp, i32, i32, vp, i32, P64]),
            "lsb_get_last_select": (i32, [vp, ctypes.POINTER(ctypes.c_int), P64]),
            "lsb_search": (i32, [vp, i32, i64, vp, i32, i32, i32, vp]),
            "lsb_lookup": (i32, [vp, i32, i64, vp, i32, i32, vp, i32, vp]),
            "lsb_join_count": (i32, [vp, i32, i64, vp, i32, i32, vp, P64]),
            "lsb_store_join": (i32, [vp, i32, i64, i64, vp, vp, i32, vp, P64]),
            "lsb_sort": (i32, [vp]),
            "lsb_pass": (i32, [vp, i32]),
            "lsb_sync": (i32, [vp]),
            "lsb_barrier": (i32, [vp]),
            "lsb_verify": (i32, [vp, P64]),
            "lsb_check_sorted": (i32, [vp, ctypes.POINTER(ctypes.c_int)]),
            "lsb_get_kernel_stats": (i32, [vp, i32, P64, ctypes.POINTER(ctypes.c_double)]),
            "lsb_reset_kernel_stats": (i32, [vp]),
            "lsb_get_scatter_elems": (i32, [vp, P64]),
            "lsb_get_pass_stats": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int), P64, P64,
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
            "lsb_get_exchange_bytes": (i32, [vp, P64, P64, P64]),
            "lsb_get_exchange_stats": (i32, [vp, ctypes.POINTER(ExchangeStats)]),
            "lsb_get_placement": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
            "lsb_get_pass_exchange": (i32, [vp, i32, P64, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double)]),
            "lsb_build_info": (cp, []),
            "lsb_rank_footprint": (i32, [i64, i32, i32, i32, P64, P64]),
            "lsb_device_memory": (i32, [i32, P64, P64]),
            "lsb_plan_exchange": (i32, [i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
            "lsb_plan_exchange_device": (i32, [i32, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
            "lsb_plan_merge": (i32, [i64, i32, i32, vp, vp, vp, vp, vp, vp]),
            "lsb_strerror": (cp, [i32]),
        }
        for name, (res, args) in sig.items():
            # An older build given through LSB_LIBRARY (A/B timing against the
            # parent commit) lacks the newest entry points; calling them there raises.
            if name in ("lsb_get_last_packed_tile", "lsb_get_last_pass_tiles", "lsb_search", "lsb_lookup",
                        "lsb_join_count", "lsb_store_join", "lsb_rekey_columns", "lsb_rekey_index") \
                    and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _L = L
    return _L


def _check(code: int, where: str) -> None:
    if code != LSB_OK:
        raise LsbError(code, where)


def per_rank(n: int, P: int) -> int:
    return int(_lib().lsb_per_rank(n, P))


def here(n: int, P: int, r: int) -> int:
    return int(_lib().lsb_here(n, P, r))


def rank_footprint(n: int, P: int, radix_bits: int = 8, with_recv: bool = False) -> dict:
    """lsb_rank_footprint: device bytes one rank of lsb_create(n, P, radix_bits)
    holds ({"bytes"}), and the optional placement probe's transient on top
    ({"probe_bytes"}, from LSB_PLACEMENT_CANDIDATES as set now).  Host
    arithmetic only."""
    b, pb = ctypes.c_int64(), ctypes.c_int64()
    _check(_lib().lsb_rank_footprint(n, P, radix_bits, int(with_recv), ctypes.byref(b), ctypes.byref(pb)),
           "lsb_rank_footprint")
    return {"bytes": b.value, "probe_bytes": pb.value}


def device_memory(dev: int = 0) -> tuple:
    """(free, total) device bytes of device dev (lsb_device_memory)."""
    f, t = ctypes.c_int64(), ctypes.c_int64()
    _check(_lib().lsb_device_memory(dev, ctypes.byref(f), ctypes.byref(t)), "lsb_device_memory")
    return f.value, t.value


def build_info() -> dict:
    """{"sha256": digest of the sources the loaded library was built from,
    "host": build host, "rccl": ncclGetVersion of the loaded RCCL}
    (lsb_build_info)."""
    info = _lib().lsb_build_info().decode()
    return dict(kv.split("=", 1) for kv in info.split())


def source_files() -> list:
    """The library's sources, in the order the Makefile hashes them (its
    SOURCES line, with the RT list of runtime units expanded)."""
    import re
    mk = open(os.path.join(ROOT_DIR, "Makefile")).read()
    rt = re.search(r"^RT\s*:=\s*(.*)$", mk, re.M).group(1).split()
    files = []
    for tok in re.search(r"^SOURCES\s*:=\s*(.*)$", mk, re.M).group(1).split():
        if tok.startswith("$(RT:"):
            files += [f"csrc/{u}.cpp" for u in rt]
        else:
            files.append(tok)
    return files


def source_digest() -> str:
    """sha256 of the library's sources as they are in this tree, in the
    order the Makefile hashes them (SOURCES)."""
    import hashlib
    h = hashlib.sha256()
    for rel in source_files():
        with open(os.path.join(ROOT_DIR, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def key_encode(bits: int, key_type: int, descending: bool = False) -> int:
    """lsb_key_encode: the unsigned 64-bit key the passes sort a typed key's
    raw bits by (0 on an unknown type).  Host arithmetic only."""
    return int(_lib().lsb_key_encode(bits, key_type, ORDER_DESCENDING if descending else 0))


def key_decode(key: int, key_type: int, descending: bool = False) -> int:
    """lsb_key_decode: the inverse of key_encode."""
    return int(_lib().lsb_key_decode(key, key_type, ORDER_DESCENDING if descending else 0))


def _key_type_of(t, key_type=None) -> int:
    """The LSB_KEY_* of a torch tensor's dtype (key_type given: checked
    against the element size instead, for dtypes torch has no name for)."""
    import torch
    if key_type is not None:
        if key_type not in range(6) or t.element_size() != (4 if key_type >= KEY_U32 else 8):
            raise ValueError(f"key_type {key_type} does not fit {t.dtype}")
        return key_type
    table = {torch.int64: KEY_I64, torch.float64: KEY_F64, torch.int32: KEY_I32, torch.float32: KEY_F32}
    for name, kt in (("uint64", KEY_U64), ("uint32", KEY_U32)):
        if hasattr(torch, name):
            table[getattr(torch, name)] = kt
    if t.dtype not in table:
        raise ValueError(f"no key type for {t.dtype}; pass key_type=")
    return table[t.dtype]


def _check_column(t, what: str, device=None):
    """A column the library can take: a 1-D contiguous CUDA torch tensor of 4-
    or 8-byte elements (on `device`, when given).  ValueError otherwise."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: not a torch tensor")
    if not t.is_cuda:
        raise ValueError(f"{what}: not on a GPU")
    if t.dim() != 1:
        raise ValueError(f"{what}: not 1-D")
    if not t.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    if t.element_size() not in (4, 8):
        raise ValueError(f"{what}: elements of {t.element_size()} bytes")
    if device is not None and t.device != device:
        raise ValueError(f"{what}: on {t.device}, not {device}")


def sort(keys, values=None, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
         key_type: Optional[int] = None):
    """Stable sort of device columns: (sorted_keys, sorted_values), or with
    values=None (sorted_keys, indices), indices the int64 stable argsort.

    keys: 1-D contiguous CUDA tensor (int64, float64, int32, float32, uint64,
    uint32; key_type= for other dtypes of 4 or 8 bytes); values: any 4- or
    8-byte dtype, same length.  Floats sort in the order of lsb.h (NaNs at both
    ends by sign, -0.0 before +0.0); equal keys keep their input order in both
    directions.  The inputs are left untouched; the outputs are fresh tensors.
    One World(n, ranks) on the keys' device does the work, rank r holding block
    [r * per, r * per + here(r))."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if values is not None:
        _check_column(values, "values", keys.device)
        if values.numel() != keys.numel():
            raise ValueError("keys and values differ in length")
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    out_k = torch.empty_like(keys)
    out_v = torch.empty_like(values) if values is not None else torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out_k, out_v
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, keys[lo:lo + h], None if values is None else values[lo:lo + h],
                           descending=descending, key_type=kt)
        w.my_sort()
        for r, lo, h in blocks:
            w.store_columns(r, out_k[lo:lo + h], out_v[lo:lo + h], descending=descending, key_type=kt)
    return out_k, out_v


def _check_sort_columns(columns, descending):
    """sort_by's arguments -> (columns, key types, one descending flag per
    column).  ValueError on anything sort_by refuses."""
    import torch
    if isinstance(columns, torch.Tensor) or not isinstance(columns, (list, tuple)):
        raise ValueError("columns: not a sequence of 1-D tensors")
    cols = list(columns)
    if not cols:
        raise ValueError("columns: empty")
    for i, c in enumerate(cols):
        if not isinstance(c, torch.Tensor) or c.dim() != 1:
            raise ValueError(f"columns[{i}]: not a 1-D torch tensor")
    if any(c.numel() != cols[0].numel() for c in cols):
        raise ValueError("columns differ in length")
    if any(c.device != cols[0].device for c in cols):
        raise ValueError("columns on different devices")
    if isinstance(descending, (bool, np.bool_)):
        desc = [bool(descending)] * len(cols)
    else:
        desc = [bool(d) for d in descending]
        if len(desc) != len(cols):
            raise ValueError("descending: one flag per column")
    for i, c in enumerate(cols):
        _check_column(c, f"columns[{i}]")
    return cols, [_key_type_of(c) for c in cols], desc


def _sort_world_by(w, cols, kts, desc) -> list:
    """The LSD sort over columns in w (n = the columns' length): the last
    column loaded with index values and sorted, then every earlier column,
    last to first, rekeyed into the records and sorted again.  -> the
    non-empty ranks' (rank, first index, records)."""
    blocks = [(r, r * w.per, w.here(r)) for r in range(w.P) if w.here(r)]
    for r, lo, h in blocks:
        w.load_columns(r, cols[-1][lo:lo + h], None, descending=desc[-1], key_type=kts[-1])
    w.my_sort()
    for c, kt, d in reversed(list(zip(cols[:-1], kts[:-1], desc[:-1]))):
        for r, _, _ in blocks:
            w.rekey(r, c, descending=d, key_type=kt)
        w.my_sort()
    return blocks


def sort_by(columns, descending=False, ranks: int = 1, radix_bits: int = 8):
    """The stable lexicographic argsort of device columns: int64 indices i
    such that (columns[0][i], columns[1][i], ...) ascends, columns[0] the
    primary (ORDER BY a, b, c; numpy.lexsort with the columns reversed).

    columns: one or more 1-D contiguous CUDA tensors of equal length on one
    device, any mix of sort()'s key dtypes; descending: one bool, or one per
    column.  Rows equal on every column keep their input order.  Float order
    and equality (of bits) are those of lsb.h.  With one column the result is
    sort(x)[1].  The inputs are left untouched.  One World(n, ranks) on the
    columns' device sorts by the last column, then rekeys by and sorts on each
    earlier one; every rank reads the whole columns."""
    import torch
    cols, kts, desc = _check_sort_columns(columns, descending)
    if ranks < 1:
        raise ValueError("ranks")
    n = cols[0].numel()
    out = torch.empty(n, dtype=torch.int64, device=cols[0].device)
    if n == 0:
        return out
    dev = cols[0].device.index if cols[0].device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r, lo, h in _sort_world_by(w, cols, kts, desc):
            w.store_columns(r, None, out[lo:lo + h])
    return out


def sort_rows(keys2d, descending: bool = False, ranks: int = 1, radix_bits: int = 8):
    """Every row of a 2-D tensor sorted stably: (sorted_keys, indices), both
    [R, L], indices int64 within the row (torch.sort(stable=True, dim=-1)).

    keys2d: a contiguous 2-D CUDA tensor of one of sort()'s key dtypes, left
    untouched.  One World(R * L, ranks) sorts the flattened keys with index
    values, rekeys every record by its row (index // L) and sorts again: the
    second sort runs only the passes the row numbers need."""
    import torch
    if not isinstance(keys2d, torch.Tensor) or keys2d.dim() != 2:
        raise ValueError("keys2d: not a 2-D torch tensor")
    if not keys2d.is_cuda:
        raise ValueError("keys2d: not on a GPU")
    if not keys2d.is_contiguous():
        raise ValueError("keys2d: not contiguous")
    flat = keys2d.reshape(-1)
    _check_column(flat, "keys2d")
    kt = _key_type_of(flat)
    if ranks < 1:
        raise ValueError("ranks")
    R, L = keys2d.shape
    n = R * L
    v = torch.empty(n, dtype=torch.int64, device=keys2d.device)
    if n == 0:
        return torch.empty_like(keys2d), v.reshape(R, L)
    dev = keys2d.device.index if keys2d.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, flat[lo:lo + h], None, descending=descending, key_type=kt)
        w.my_sort()
        for r, _, _ in blocks:
            w.rekey_index(r, L)
        w.my_sort()
        for r, lo, h in blocks:
            w.store_columns(r, None, v[lo:lo + h])
    return flat[v].reshape(R, L), (v % L).reshape(R, L)


def segment_sort(keys, offsets, descending: bool = False, ranks: int = 1, radix_bits: int = 8):
    """Keys sorted stably inside caller-given segments (CSR rows, ragged
    batches): (sorted_keys, indices), indices the int64 global input indices.

    keys: as for sort(); offsets: int64 tensor of S + 1 non-decreasing offsets
    from 0 to len(keys), segment s being keys[offsets[s]:offsets[s + 1]]
    (empty segments allowed).  The segment ids are built with torch, then it
    is sort_by([segment_ids, keys]).  The inputs are left untouched."""
    import torch
    if not isinstance(keys, torch.Tensor) or keys.dim() != 1:
        raise ValueError("keys: not a 1-D torch tensor")
    if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.dtype != torch.int64:
        raise ValueError("offsets: not a 1-D int64 torch tensor")
    n = keys.numel()
    if offsets.numel() < 1 or int(offsets[0]) != 0 or int(offsets[-1]) != n:
        raise ValueError("offsets: not from 0 to len(keys)")
    if offsets.numel() > 1 and int((offsets[1:] - offsets[:-1]).min()) < 0:
        raise ValueError("offsets: decreasing")
    _check_column(keys, "keys")
    _key_type_of(keys)
    if ranks < 1:
        raise ValueError("ranks")
    off = offsets.to(keys.device)
    counts = off[1:] - off[:-1]
    if n == 0:
        return torch.empty_like(keys), torch.empty(0, dtype=torch.int64, device=keys.device)
    S = counts.numel()
    ids = torch.repeat_interleave(torch.arange(S, dtype=torch.int64, device=keys.device), counts)
    if S <= 1 << 31:  # a 32-bit primary column: its upper digits are skipped
        ids = ids.to(torch.int32)
    idx = sort_by([ids, keys], [False, descending], ranks=ranks, radix_bits=radix_bits)
    return keys[idx], idx


def group_quantile(keys, values, q: float = 0.5, descending: bool = False, ranks: int = 1, radix_bits: int = 8):
    """One order statistic per group of equal keys: (unique_keys,
    quantile_values), the first answer here to PARTITION BY key ORDER BY value.

    unique_keys: the distinct keys in sorted order (descending: reversed), as
    unique(); quantile_values[j]: of the group's values sorted ascending in the
    value dtype's key order, the element at position floor(q * (count - 1))
    (float64 arithmetic): q = 0 the minimum, 0.5 the lower median, 1 the
    maximum.  keys and values: as sort()'s keys, equal length, one device.
    The inputs are left untouched.  One World(n, ranks) sorts by [keys,
    values], counts the runs and stores their keys, starts and counts; one
    gather picks the values."""
    import torch
    if not (isinstance(q, (int, float)) and 0.0 <= float(q) <= 1.0):
        raise ValueError("q: not in [0, 1]")
    cols, kts, _ = _check_sort_columns([keys, values], False)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    if n == 0:
        return torch.empty_like(keys), torch.empty_like(values)
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = _sort_world_by(w, cols, kts, [descending, False])
        idx = torch.empty(n, dtype=torch.int64, device=keys.device)
        for r, lo, h in blocks:
            w.store_columns(r, None, idx[lo:lo + h])
        plan = w.count_runs()
        total = plan["total"]
        out_k = torch.empty(total, dtype=keys.dtype, device=keys.device)
        starts = torch.empty(total, dtype=torch.int64, device=keys.device)
        counts = torch.empty(total, dtype=torch.int64, device=keys.device)
        for r in range(ranks):
            lo, m = plan["bases"][r], plan["runs"][r]
            if m:
                w.store_runs(r, keys=out_k[lo:lo + m], starts=starts[lo:lo + m], counts=counts[lo:lo + m],
                             descending=descending, key_type=kts[0])
    pos = starts + torch.floor(float(q) * (counts - 1).to(torch.float64)).to(torch.int64)
    return out_k, values[idx[pos]]


def _store_inverse(w, inverse) -> None:
    """The run plan of w's sorted records, loaded with index values, into the
    run id of every input record: label by value, sort by the index again,
    store each rank's values into its block of `inverse` (int64, n)."""
    w.label_runs(LABEL_BY_VALUE)
    w.my_sort()
    for r in range(w.P):
        lo, h = r * w.per, w.here(r)
        if h:
            w.store_columns(r, None, inverse[lo:lo + h])


def unique(keys, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
           key_type: Optional[int] = None, return_inverse: bool = False):
    """The distinct keys of a device column: (unique_keys, first_index, counts),
    or with return_inverse=True (unique_keys, first_index, counts, inverse).

    unique_keys: the distinct keys in sorted order (descending: reversed), in
    the input's dtype; first_index: int64, the input index of each key's first
    occurrence; counts: int64, how often it occurs; inverse: int64 of the
    input's length, the index of each input key in unique_keys, so that
    unique_keys[inverse] is the input bit for bit.  Keys are equal when their
    bits are: -0.0 and +0.0 are two keys, NaNs with different payloads too.
    keys as for sort(); the input is left untouched, the outputs are fresh
    tensors.  One World(n, ranks) loads the keys with index values, sorts,
    counts the runs and stores each rank's into its part of the outputs; the
    inverse then labels every record with its run, sorts the records back by
    their index and stores the labels."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    if n == 0:
        out = (torch.empty_like(keys), torch.empty(0, dtype=torch.int64, device=keys.device),
               torch.empty(0, dtype=torch.int64, device=keys.device))
        return out + (torch.empty(0, dtype=torch.int64, device=keys.device),) if return_inverse else out
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, keys[lo:lo + h], None, descending=descending, key_type=kt)
        w.my_sort()
        plan = w.count_runs()
        total = plan["total"]
        out_k = torch.empty(total, dtype=keys.dtype, device=keys.device)
        out_i = torch.empty(total, dtype=torch.int64, device=keys.device)
        out_c = torch.empty(total, dtype=torch.int64, device=keys.device)
        starts = torch.empty(total, dtype=torch.int64, device=keys.device)
        for r in range(ranks):
            lo, m = plan["bases"][r], plan["runs"][r]
            if m:
                w.store_runs(r, keys=out_k[lo:lo + m], starts=starts[lo:lo + m], counts=out_c[lo:lo + m],
                             firsts=out_i[lo:lo + m], descending=descending, key_type=kt)
        if return_inverse:
            inverse = torch.empty(n, dtype=torch.int64, device=keys.device)
            _store_inverse(w, inverse)
            return out_k, out_i, out_c, inverse
    return out_k, out_i, out_c


def dense_rank(keys, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
               key_type: Optional[int] = None):
    """The 0-based dense rank of every key of a device column: int64 of the
    input's length, rank[i] = the number of distinct keys below keys[i]
    (descending: above it), in the float order of lsb.h; equal keys (equal
    bits) share a rank and the ranks have no gaps (SQL DENSE_RANK() - 1,
    factorize codes of the sorted distinct keys, unique()'s inverse alone).
    keys as for sort(); the input is left untouched."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    inverse = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return inverse
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, keys[lo:lo + h], None, descending=descending, key_type=kt)
        w.my_sort()
        w.count_runs()
        _store_inverse(w, inverse)
    return inverse


def _value_type_of(t) -> int:
    """The LSB_KEY_* a value column's 64 bits are reduced as."""
    import torch
    table = {torch.int64: KEY_I64, torch.float64: KEY_F64}
    if hasattr(torch, "uint64"):
        table[torch.uint64] = KEY_U64
    if t.dtype not in table:
        raise ValueError(f"no reduction over {t.dtype} values (int64, float64, uint64)")
    return table[t.dtype]


def group_reduce(keys, values, op: str = "sum", descending: bool = False, ranks: int = 1, radix_bits: int = 8,
                 key_type: Optional[int] = None):
    """Group-by with one reduction: (unique_keys, reduced).

    unique_keys: the distinct keys in sorted order (descending: reversed), in
    the keys' dtype, as unique(); reduced[j]: op ("sum", "min", "max") over the
    values of every record whose key is unique_keys[j], in the values' dtype
    (int64, float64, or uint64 where torch has it).  Integer sums wrap; a
    float64 sum is reproducible for given inputs and ranks; min and max follow
    lsb.h's float order.  keys as for sort(); values the same length.  The
    inputs are left untouched, the outputs are fresh tensors.  One
    World(n, ranks) loads the columns, sorts, counts the runs, plans the
    reduction and stores each rank's keys and values into its part of the
    outputs."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    _check_column(values, "values", keys.device)
    vt = _value_type_of(values)
    if values.numel() != keys.numel():
        raise ValueError("keys and values differ in length")
    ops = {"sum": REDUCE_SUM, "min": REDUCE_MIN, "max": REDUCE_MAX}
    if op not in ops:
        raise ValueError(f"op {op!r}: not one of {sorted(ops)}")
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    if n == 0:
        return torch.empty_like(keys), torch.empty_like(values)
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, keys[lo:lo + h], values[lo:lo + h], descending=descending, key_type=kt)
        w.my_sort()
        plan = w.count_runs()
        w.plan_reduce(ops[op], vt)
        total = plan["total"]
        out_k = torch.empty(total, dtype=keys.dtype, device=keys.device)
        out_v = torch.empty(total, dtype=values.dtype, device=keys.device)
        for r in range(ranks):
            lo, m = plan["bases"][r], plan["runs"][r]
            if m:
                w.store_runs(r, keys=out_k[lo:lo + m], descending=descending, key_type=kt)
                w.store_reduce(r, out_v[lo:lo + m])
    return out_k, out_v


def group_scan(keys, values, op: str = "sum", descending: bool = False, ranks: int = 1, radix_bits: int = 8,
               key_type: Optional[int] = None):
    """A running reduction inside every group, in input order: out[i] = op
    ("sum", "min", "max") over values[j] of every j <= i whose key has the bits
    of keys[i] (groupby(keys).cumsum(), cummin(), cummax()), in the values'
    dtype (int64, float64, or uint64 where torch has it).

    Integer sums wrap; a float64 sum is reproducible for given inputs and
    ranks; min and max follow lsb.h's float order.  keys as for sort(); values
    the same length.  The inputs are left untouched, the output is a fresh
    tensor.  sort() gives the sorted keys and the stable argsort, torch gathers
    the values by it, one World(n, ranks) loads the two sorted columns, counts
    the runs, plans the scan and stores each rank's results, and torch
    scatters them back by the argsort."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    _check_column(values, "values", keys.device)
    vt = _value_type_of(values)
    if values.numel() != keys.numel():
        raise ValueError("keys and values differ in length")
    ops = {"sum": SCAN_SUM, "min": SCAN_MIN, "max": SCAN_MAX}
    if op not in ops:
        raise ValueError(f"op {op!r}: not one of {sorted(ops)}")
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    out = torch.empty_like(values)
    if n == 0:
        return out
    sorted_keys, idx = sort(keys, None, descending=descending, ranks=ranks, radix_bits=radix_bits, key_type=kt)
    # torch indexes int64 where it does not uint64: the gather and the scatter move bits
    gathered = values.view(torch.int64)[idx]
    scanned = torch.empty(n, dtype=torch.int64, device=keys.device)
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, sorted_keys[lo:lo + h], gathered[lo:lo + h], descending=descending, key_type=kt)
        w.count_runs()
        w.plan_scan(ops[op], vt)
        for r, lo, h in blocks:
            w.store_scan(r, scanned[lo:lo + h])
    out.view(torch.int64)[idx] = scanned
    return out


def _scan_positions(keys, op: int, descending: bool, ranks: int, radix_bits: int, key_type: Optional[int]):
    """SCAN_COUNT or SCAN_START of every key, in input order (int64): the
    inverse's route with the scan's result in place of the run id."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    out = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, keys[lo:lo + h], None, descending=descending, key_type=kt)
        w.my_sort()
        w.count_runs()
        w.plan_scan(op, KEY_U64)
        w.scan_runs(LABEL_BY_VALUE)
        w.my_sort()
        for r, lo, h in blocks:
            w.store_columns(r, None, out[lo:lo + h])
    return out


def cumcount(keys, descending: bool = False, ranks: int = 1, radix_bits: int = 8, key_type: Optional[int] = None):
    """The number of earlier records with the same key, for every key of a
    device column: int64 of the input's length (groupby(keys).cumcount(),
    ROW_NUMBER() OVER (PARTITION BY key) - 1).  Keys are equal when their bits
    are.  keys as for sort(); the input is left untouched."""
    return _scan_positions(keys, SCAN_COUNT, descending, ranks, radix_bits, key_type)


def rank(keys, descending: bool = False, ranks: int = 1, radix_bits: int = 8, key_type: Optional[int] = None):
    """The 0-based competition rank of every key of a device column: int64 of
    the input's length, rank[i] = the number of records whose key is strictly
    below keys[i] (descending: above it), in the float order of lsb.h; ties
    share the lowest rank (SQL RANK() - 1, rankdata(method="min") - 1).  keys
    as for sort(); the input is left untouched."""
    return _scan_positions(keys, SCAN_START, descending, ranks, radix_bits, key_type)


def _key_tensor(bits: int, like):
    """A 1-element tensor of like's dtype and device whose bits are `bits`."""
    import torch
    wide = like.element_size() == 8
    width = 64 if wide else 32
    bits &= (1 << width) - 1
    signed = bits - (1 << width) if bits >> (width - 1) else bits
    t = torch.tensor([signed], dtype=torch.int64 if wide else torch.int32, device=like.device)
    return t.view(like.dtype)


def kth(keys, k: int, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
        key_type: Optional[int] = None):
    """The k-th smallest key of a device column (descending: the k-th
    largest), k counted from 0: (value, below, equal).

    value: a 1-element tensor of the keys' dtype on their device, the key the
    stable sort would put at position k, bit for bit (NaN payloads, the sign
    of zero); below, equal: how many keys lie before it in the order and how
    many have its bits, so below <= k < below + equal.  The order is sort()'s
    (lsb.h's float order).  No sort is run: one World(n, ranks) loads the keys
    and selects.  keys as for sort(); the input is left untouched.
    ValueError unless 0 <= k < len(keys)."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    if not 0 <= k < n:
        raise ValueError(f"k = {k} outside [0, {n})")
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, keys[lo:lo + h], None, descending=descending, key_type=kt)
        plan = w.select(k)
    return _key_tensor(key_decode(plan["key"], kt, descending), keys), plan["below"], plan["equal"]


def topk(keys, k: int, largest: bool = True, sorted: bool = True, ranks: int = 1, radix_bits: int = 8,  # noqa: A002
         key_type: Optional[int] = None):
    """The k largest keys of a device column (largest=False: the k smallest)
    and where they were: (values, indices), the first k records of the stable
    sort in that direction, so among equal keys the lowest input indices are
    taken (a rule torch.topk does not promise).

    values: the keys' dtype, bit for bit; indices: int64 input indices.
    sorted=True gives them in the sort's order (sort() over the k records),
    sorted=False in input order.  The order is sort()'s (lsb.h's float order:
    NaNs with the sign clear are the largest).  One World(n, ranks) loads the
    keys with index values, selects position k - 1 and stores each rank's part
    of the selection; no full sort is run.  keys as for sort(); the input is
    left untouched.  k == 0 or no keys: empty tensors; k > len(keys):
    ValueError."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    if ranks < 1:
        raise ValueError("ranks")
    n = keys.numel()
    if k < 0 or k > n:
        raise ValueError(f"k = {k} outside [0, {n}]")
    values = torch.empty(k, dtype=keys.dtype, device=keys.device)
    indices = torch.empty(k, dtype=torch.int64, device=keys.device)
    if k == 0:
        return values, indices
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        for r in range(ranks):
            lo, h = r * w.per, w.here(r)
            if h:
                w.load_columns(r, keys[lo:lo + h], None, descending=largest, key_type=kt)
        plan = w.select(k - 1)
        for r in range(ranks):
            lo, m = plan["bases"][r], plan["take"][r]
            if m:
                w.store_select(r, values[lo:lo + m], indices[lo:lo + m], descending=largest, key_type=kt)
    if sorted:
        return sort(values, indices, descending=largest, radix_bits=radix_bits, key_type=kt)
    return values, indices


_SEARCH_SIDES = {"left": SEARCH_LOWER, "right": SEARCH_UPPER, "count": SEARCH_COUNT}


def _search(keys, queries, side: str, descending: bool, ranks: int, radix_bits: int, key_type: Optional[int],
            assume_sorted: bool):
    """One number per query (int64) from the sorted keys: World.search of every
    non-empty rank, added up."""
    import torch
    if side not in _SEARCH_SIDES:
        raise ValueError(f"side {side!r}: not one of {sorted(_SEARCH_SIDES)}")
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    _check_column(queries, "queries", keys.device)
    if _key_type_of(queries, key_type) != kt:
        raise ValueError(f"queries of {queries.dtype} against keys of {keys.dtype}")
    if ranks < 1:
        raise ValueError("ranks")
    n, m = keys.numel(), queries.numel()
    out = torch.zeros(m, dtype=torch.int64, device=keys.device)
    if n == 0 or m == 0:
        return out
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, keys[lo:lo + h], None, descending=descending, key_type=kt)
        if not assume_sorted:
            w.my_sort()
        for i, (r, _, _) in enumerate(blocks):
            w.search(r, queries, out, side=side, add=i > 0, descending=descending, key_type=kt)
    return out


def searchsorted(keys, queries, side: str = "left", descending: bool = False, ranks: int = 1, radix_bits: int = 8,
                 key_type: Optional[int] = None, assume_sorted: bool = False):
    """The position of every query in the stable sort of a device column:
    int64 of the queries' length, out[i] = the number of keys below queries[i]
    (side="left") or not above it (side="right"); descending: above, not below.

    The order and equality are sort()'s, on the bits: -0.0 is below +0.0, NaNs
    lie at both ends by sign and a NaN equals only its own bits, which is not
    torch.searchsorted's float behaviour.  keys as for sort(); queries: a 1-D
    contiguous CUDA tensor on the same device whose dtype maps to the same key
    type (ValueError otherwise).  The inputs are left untouched.  One
    World(n, ranks) loads the keys, sorts them unless assume_sorted says they
    are sorted already (in that order; not checked), and searches every
    non-empty rank, adding from the second on.  No keys: zeros."""
    if side not in ("left", "right"):
        raise ValueError(f"side {side!r}: not 'left' or 'right'")
    return _search(keys, queries, side, descending, ranks, radix_bits, key_type, assume_sorted)


def count_of(keys, queries, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
             key_type: Optional[int] = None, assume_sorted: bool = False):
    """How often every query occurs among the keys of a device column: int64 of
    the queries' length.  Keys are equal when their bits are.  Arguments as
    searchsorted()."""
    return _search(keys, queries, "count", descending, ranks, radix_bits, key_type, assume_sorted)


def isin(queries, keys, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
         key_type: Optional[int] = None, assume_sorted: bool = False):
    """Whether every query occurs among the keys of a device column: a bool
    tensor of the queries' length, count_of(keys, queries) > 0 (note the
    argument order, torch.isin's).  No keys: all False."""
    return _search(keys, queries, "count", descending, ranks, radix_bits, key_type, assume_sorted) > 0


def lookup(keys, values, queries, default=0, descending: bool = False, ranks: int = 1, radix_bits: int = 8,
           key_type: Optional[int] = None, assume_sorted: bool = False):
    """The value stored with every query's key: (out, found).  out has the
    values' dtype and the queries' length, prefilled with `default`; where the
    key occurs, out[i] = the value of its first occurrence (among equal keys
    the one that comes first in keys; with assume_sorted the first in the given
    order) and found[i] (bool) is True.  values=None looks up the input index
    of that first occurrence (int64).  Keys are equal when their bits are;
    the remaining arguments are searchsorted()'s.  One World(n, ranks) loads
    keys and values, sorts them unless assume_sorted, and looks the queries up
    on every non-empty rank, from the last to the first, so that the lowest
    rank's match stands."""
    import torch
    _check_column(keys, "keys")
    kt = _key_type_of(keys, key_type)
    _check_column(queries, "queries", keys.device)
    if _key_type_of(queries, key_type) != kt:
        raise ValueError(f"queries of {queries.dtype} against keys of {keys.dtype}")
    if values is not None:
        _check_column(values, "values", keys.device)
        if values.numel() != keys.numel():
            raise ValueError("keys and values differ in length")
    if ranks < 1:
        raise ValueError("ranks")
    n, m = keys.numel(), queries.numel()
    out = torch.full((m,), default, dtype=torch.int64 if values is None else values.dtype, device=keys.device)
    found = torch.zeros(m, dtype=torch.uint8, device=keys.device)
    if n == 0 or m == 0:
        return out, found.bool()
    dev = keys.device.index if keys.device.index is not None else torch.cuda.current_device()
    with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
        blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
        for r, lo, h in blocks:
            w.load_columns(r, keys[lo:lo + h], None if values is None else values[lo:lo + h],
                           descending=descending, key_type=kt)
        if not assume_sorted:
            w.my_sort()
        for r, _, _ in reversed(blocks):
            w.lookup(r, queries, out, found, descending=descending, key_type=kt)
    return out, found.bool()


_JOIN_HOW = ("inner", "left")


def join(left_keys, right_keys, how: str = "inner", descending: bool = False, ranks: int = 1, radix_bits: int = 8,
         key_type: Optional[int] = None, assume_sorted: bool = False):
    """All pairs of equal keys of two device columns: (left_index, right_index),
    both int64, left_keys[left_index[j]] == right_keys[right_index[j]] on the
    bits, every such pair once.  One World(n, ranks) loads right_keys with
    their indices and sorts them (unless assume_sorted says they are sorted in
    that order already), then counts and stores the pairs of every non-empty
    rank, in rank order.  ranks=1: ordered by left index, then by right index;
    more ranks: each rank's pairs in that order, rank after rank.
    how="left" appends (i, -1) for every left key without a match, after the
    matched pairs and in left order.  No keys on either side: no matched
    pair.  The remaining arguments are searchsorted()'s, right_keys being the
    sorted side."""
    import torch
    if how not in _JOIN_HOW:
        raise ValueError(f"how {how!r}: not one of {_JOIN_HOW}")
    _check_column(right_keys, "right_keys")
    kt = _key_type_of(right_keys, key_type)
    _check_column(left_keys, "left_keys", right_keys.device)
    if _key_type_of(left_keys, key_type) != kt:
        raise ValueError(f"left keys of {left_keys.dtype} against right keys of {right_keys.dtype}")
    if ranks < 1:
        raise ValueError("ranks")
    n, m = right_keys.numel(), left_keys.numel()
    device = right_keys.device
    lefts, rights = [], []
    matched = torch.zeros(m, dtype=torch.int64, device=device)
    if n > 0 and m > 0:
        dev = device.index if device.index is not None else torch.cuda.current_device()
        with World(n, ranks=ranks, devices=[dev] * ranks, radix_bits=radix_bits) as w:
            blocks = [(r, r * w.per, w.here(r)) for r in range(ranks) if w.here(r)]
            for r, lo, h in blocks:
                w.load_columns(r, right_keys[lo:lo + h], None, descending=descending, key_type=kt)
            if not assume_sorted:
                w.my_sort()
            counts = torch.empty(m, dtype=torch.int64, device=device) if how == "left" else None
            for r, _, _ in blocks:
                total = w.join_count(r, left_keys, counts, descending=descending, key_type=kt)
                if counts is not None:
                    matched += counts
                if total == 0:
                    continue
                li = torch.empty(total, dtype=torch.int64, device=device)
                ri = torch.empty(total, dtype=torch.int64, device=device)
                w.store_join(r, left=li, right=ri)
                lefts.append(li)
                rights.append(ri)
    if how == "left":
        lone = torch.nonzero(matched == 0).flatten()
        lefts.append(lone)
        rights.append(torch.full_like(lone, -1))
    if not lefts:
        empty = torch.empty(0, dtype=torch.int64, device=device)
        return empty, empty.clone()
    return torch.cat(lefts), torch.cat(rights)


def plan_select(n: int, P: int, count: int, below: np.ndarray, equal: np.ndarray) -> dict:
    """lsb_plan_select, the host planner of the select: below[r], equal[r] =
    rank r's records below and equal to the pivot, count = k + 1 wanted
    records -> {"take", "bases"} (P each): what each rank gives and where its
    part starts."""
    below = np.ascontiguousarray(below, dtype=np.int64)
    equal = np.ascontiguousarray(equal, dtype=np.int64)
    if below.shape != (P,) or equal.shape != (P,):
        raise ValueError("below and equal must hold P entries")
    out = {k: np.zeros(P, dtype=np.int64) for k in ("take", "bases")}
    _check(_lib().lsb_plan_select(n, P, count, below.ctypes.data, equal.ctypes.data, out["take"].ctypes.data,
                                  out["bases"].ctypes.data), "lsb_plan_select")
    return out


def plan_runs(n: int, P: int, summary: np.ndarray) -> dict:
    """lsb_plan_runs, the host planner of the runs of equal keys: summary is
    P x 4 uint64 (first key, last key, inner heads, leading run's length of
    each rank) -> {"head0", "runs", "bases", "ends"} (P each) and "total"."""
    summary = np.ascontiguousarray(summary, dtype=np.uint64)
    if summary.shape != (P, 4):
        raise ValueError("summary must be P x 4")
    out = {k: np.zeros(P, dtype=np.int64) for k in ("runs", "bases", "ends")}
    head0 = np.zeros(P, dtype=np.intc)
    total = ctypes.c_int64()
    _check(_lib().lsb_plan_runs(n, P, summary.ctypes.data, head0.ctypes.data, out["runs"].ctypes.data,
                                out["bases"].ctypes.data, out["ends"].ctypes.data, ctypes.byref(total)),
           "lsb_plan_runs")
    out["head0"] = head0.astype(np.int64)
    out["total"] = int(total.value)
    return out


def plan_run_tails(n: int, P: int, summary: np.ndarray, op: int, val_type: int, lead: np.ndarray) -> np.ndarray:
    """lsb_plan_run_tails, the host planner of the reductions over the runs'
    values: summary as for plan_runs, lead[s] = op over the values of rank
    s's leading run (uint64 bits) -> tail[P] (uint64 bits), what the ranks
    after r add to r's last run."""
    summary = np.ascontiguousarray(summary, dtype=np.uint64)
    lead = np.ascontiguousarray(lead, dtype=np.uint64)
    if summary.shape != (P, 4) or lead.shape != (P,):
        raise ValueError("summary must be P x 4, lead P")
    tail = np.zeros(P, dtype=np.uint64)
    _check(_lib().lsb_plan_run_tails(n, P, summary.ctypes.data, op, val_type, lead.ctypes.data, tail.ctypes.data),
           "lsb_plan_run_tails")
    return tail


def plan_run_carries(n: int, P: int, summary: np.ndarray, op: int, val_type: int, trail: np.ndarray) -> np.ndarray:
    """lsb_plan_run_carries, the host planner of the scans within the runs:
    summary as for plan_runs, trail[s] = op over the operands of rank s's
    records from its last head on (uint64 bits) -> carry[P] (uint64 bits),
    what the ranks before r add to r's leading run."""
    summary = np.ascontiguousarray(summary, dtype=np.uint64)
    trail = np.ascontiguousarray(trail, dtype=np.uint64)
    if summary.shape != (P, 4) or trail.shape != (P,):
        raise ValueError("summary must be P x 4, trail P")
    carry = np.zeros(P, dtype=np.uint64)
    _check(_lib().lsb_plan_run_carries(n, P, summary.ctypes.data, op, val_type, trail.ctypes.data,
                                       carry.ctypes.data), "lsb_plan_run_carries")
    return carry


def get_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(_lib().lsb_get_unique_id(buf), "lsb_get_unique_id")
    return buf.raw


def plan_exchange(n: int, P: int, rank: int, hist: np.ndarray, device: Optional[int] = None) -> dict:
    """Exchange plan of rank `rank` for a P x nbuckets count matrix: the host
    planner, or (device=d) the device kernels the runtime runs."""
    hist = np.ascontiguousarray(hist, dtype=np.int64)
    if hist.ndim != 2 or hist.shape[0] != P:
        raise ValueError("hist must be P x nbuckets")
    nb = hist.shape[1]
    out = {k: np.zeros(P, dtype=np.int64) for k in
           ("send_counts", "send_displs", "recv_counts", "recv_displs")}
    out["place_off"] = np.zeros((P, nb), dtype=np.int64)
    args = (n, P, rank, nb, hist.ctypes.data, out["send_counts"].ctypes.data,
            out["send_displs"].ctypes.data, out["recv_counts"].ctypes.data,
            out["recv_displs"].ctypes.data, out["place_off"].ctypes.data)
    if device is None:
        _check(_lib().lsb_plan_exchange(*args), "lsb_plan_exchange")
    else:
        _check(_lib().lsb_plan_exchange_device(device, *args), "lsb_plan_exchange_device")
    return out


def plan_merge(n: int, P: int, rank: int, below: np.ndarray, upto: np.ndarray) -> dict:
    """Whole-key exchange plan of rank `rank` (lsb_plan_merge): below/upto are
    P x (P-1) counts of keys <, <= the key at global position q * per."""
    below = np.ascontiguousarray(below, dtype=np.int64).reshape(P, max(P - 1, 0))
    upto = np.ascontiguousarray(upto, dtype=np.int64).reshape(P, max(P - 1, 0))
    out = {k: np.zeros(P, dtype=np.int64) for k in
           ("send_counts", "send_displs", "recv_counts", "recv_displs")}
    _check(_lib().lsb_plan_merge(n, P, rank, below.ctypes.data, upto.ctypes.data,
                                 out["send_counts"].ctypes.data, out["send_displs"].ctypes.data,
                                 out["recv_counts"].ctypes.data, out["recv_displs"].ctypes.data),
           "lsb_plan_merge")
    return out


class World:
    """One sort context: a block-distributed pair of arrays A, B over P ranks.

    ``World(n, ranks=P)`` drives all P ranks from this process (logical
    ranks; ``devices[r]`` per rank, default all on device 0).
    ``World.rank(n, P, r, device, uid)`` is one rank of a multi-process RCCL
    world (one process per GPU).
    """

    def __init__(self, n: int, ranks: int = 1, devices: Optional[Sequence[int]] = None,
                 radix_bits: int = 8, _handle=None, _P=None):
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
            self.P = _P
        else:
            devs = None
            if devices is not None:
                if len(devices) != ranks:
                    raise ValueError("one device per rank")
                devs = (ctypes.c_int * ranks)(*devices)
            _check(_lib().lsb_create(ctypes.byref(self._h), n, ranks, devs, radix_bits),
                   "lsb_create")
            self.P = ranks
        self.n = n
        self.per = per_rank(n, self.P)
        self.radix_bits = radix_bits
        first, nl = ctypes.c_int(), ctypes.c_int()
        _check(_lib().lsb_local_ranks(self._h, ctypes.byref(first), ctypes.byref(nl)),
               "lsb_local_ranks")
        self.local_ranks = list(range(first.value, first.value + nl.value))

    @classmethod
    def rank(cls, n: int, num_ranks: int, rank: int, device: int, unique_id: bytes,
             radix_bits: int = 8) -> "World":
        h = ctypes.c_void_p()
        _check(_lib().lsb_create_rank(ctypes.byref(h), n, num_ranks, rank, device, radix_bits,
                                      unique_id), "lsb_create_rank")
        return cls(n, _handle=h, _P=num_ranks, radix_bits=radix_bits)

    @classmethod
    def rank_ops(cls, n: int, num_ranks: int, rank: int, device: int, comm,
                 radix_bits: int = 8) -> "World":
        """One rank per process with host collectives instead of RCCL.

        `comm` provides (numpy uint8 buffers, host memory):
          allgather(send) -> P * len(send) bytes, rank-major
          alltoallv(send, send_counts, send_displs, recv, recv_counts, recv_displs)  (bytes)
          allreduce_min(int) -> int
          barrier()
        Any transport works (MPI, gloo, sockets); see lsb_create_rank_ops.
        """
        ops, keep = _make_comm_ops(comm, num_ranks)
        h = ctypes.c_void_p()
        _check(_lib().lsb_create_rank_ops(ctypes.byref(h), n, num_ranks, rank, device, radix_bits,
                                          ctypes.byref(ops)), "lsb_create_rank_ops")
        w = cls(n, _handle=h, _P=num_ranks, radix_bits=radix_bits)
        w._comm_keep = (ops, keep)  # the callbacks must outlive the context
        return w

    # -- lifecycle --------------------------------------------------------
    def close(self) -> None:
        if self._h:
            _lib().lsb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int) -> None:
        _check(_lib().lsb_set_option(self._h, opt, value), "lsb_set_option")

    # -- data ---------------------------------------------------------------
    def here(self, r: int) -> int:
        return here(self.n, self.P, r)

    def generate(self, dist: str = "uniform", s: float = 1.1) -> None:
        """pcg64(rank) input; dist "zipf" maps each draw to a skewed key."""
        if dist == "uniform":
            _check(_lib().lsb_generate(self._h), "lsb_generate")
        elif dist == "zipf":
            _check(_lib().lsb_generate_ex(self._h, DIST_ZIPF, s), "lsb_generate_ex")
        else:
            raise ValueError(dist)

    def copy_in(self, rank: int, arr: np.ndarray, off: int = 0) -> None:
        arr = np.ascontiguousarray(arr, dtype=ELEM_DTYPE)
        _check(_lib().lsb_copy_in(self._h, rank, off, arr.size, arr.ctypes.data if arr.size else None),
               "lsb_copy_in")

    def copy_out(self, rank: int, off: int = 0, cnt: Optional[int] = None) -> np.ndarray:
        if cnt is None:
            cnt = self.here(rank) - off
        out = np.empty(cnt, dtype=ELEM_DTYPE)
        _check(_lib().lsb_copy_out(self._h, rank, off, cnt, out.ctypes.data if cnt else None),
               "lsb_copy_out")
        return out

    def load_columns(self, rank: int, keys, values=None, off: int = 0, descending: bool = False,
                     key_type: Optional[int] = None) -> None:
        """lsb_load_columns: slots [off, off + len(keys)) of `rank` from device
        columns (1-D contiguous CUDA torch tensors).  The keys' dtype gives the
        key type (key_type= overrides it); values: any 4- or 8-byte dtype, or
        None for the records' global indices (the sort is then an argsort).
        torch's current stream is synchronized first; the call returns when
        the records are in place."""
        import torch
        _check_column(keys, "keys")
        kt = _key_type_of(keys, key_type)
        vb, vp = 0, None
        if values is not None:
            _check_column(values, "values", keys.device)
            if values.numel() != keys.numel():
                raise ValueError("keys and values differ in length")
            vb, vp = values.element_size(), values.data_ptr()
        torch.cuda.current_stream(keys.device).synchronize()
        _check(_lib().lsb_load_columns(self._h, rank, off, keys.numel(), keys.data_ptr(), kt, vp, vb,
                                       ORDER_DESCENDING if descending else 0), "lsb_load_columns")

    def store_columns(self, rank: int, keys=None, values=None, off: int = 0, descending: bool = False,
                      key_type: Optional[int] = None) -> None:
        """lsb_store_columns: slots [off, off + len) of `rank` into device
        columns, with the key type and order the load was given.  keys or
        values may be None (not both); 4-byte values get the low word."""
        import torch
        if keys is None and values is None:
            raise ValueError("no output column")
        cols = [t for t in (keys, values) if t is not None]
        for t, what in ((keys, "keys"), (values, "values")):
            if t is not None:
                _check_column(t, what, cols[0].device)
        if len(cols) == 2 and keys.numel() != values.numel():
            raise ValueError("keys and values differ in length")
        kt = _key_type_of(keys, key_type) if keys is not None else (KEY_U64 if key_type is None else key_type)
        vb, vp = (values.element_size(), values.data_ptr()) if values is not None else (0, None)
        torch.cuda.current_stream(cols[0].device).synchronize()
        _check(_lib().lsb_store_columns(self._h, rank, off, cols[0].numel(),
                                        None if keys is None else keys.data_ptr(), kt, vp, vb,
                                        ORDER_DESCENDING if descending else 0), "lsb_store_columns")

    def rekey(self, rank: int, column, descending: bool = False, key_type: Optional[int] = None) -> None:
        """lsb_rekey_columns: every record of `rank` gets the key of
        column[its value], in place; the values stay.  column: the WHOLE
        column (a 1-D contiguous CUDA torch tensor on the rank's device, dtype
        and key_type= as for load_columns), since the values are global input
        indices.  A value that is no index into it fails with LSB_ERR_INVALID
        and leaves that record as it was.  torch's current stream is
        synchronized first; the call returns when the records are rekeyed."""
        import torch
        _check_column(column, "column")
        kt = _key_type_of(column, key_type)
        torch.cuda.current_stream(column.device).synchronize()
        _check(_lib().lsb_rekey_columns(self._h, rank, column.data_ptr() if column.numel() else None,
                                        column.numel(), kt, ORDER_DESCENDING if descending else 0),
               "lsb_rekey_columns")

    def rekey_index(self, rank: int, divisor: int = 1) -> None:
        """lsb_rekey_index: every record of `rank` gets the key value //
        divisor, in place (1: the input index itself; L: the row of a
        row-major [R, L] array)."""
        if not 0 <= divisor < 1 << 64:
            raise ValueError("divisor")
        _check(_lib().lsb_rekey_index(self._h, rank, divisor), "lsb_rekey_index")

    def count_runs(self) -> dict:
        """lsb_count_runs: the runs of equal keys of the whole array (a
        collective in a one-rank-per-process world).  {"total": runs of the
        array, "runs": [P] runs each rank owns, "bases": [P] global index of
        each rank's first run}; store_runs needs it, after the last change of
        the records."""
        total = ctypes.c_int64()
        runs = np.zeros(self.P, dtype=np.int64)
        bases = np.zeros(self.P, dtype=np.int64)
        _check(_lib().lsb_count_runs(self._h, ctypes.byref(total), runs.ctypes.data, bases.ctypes.data),
               "lsb_count_runs")
        return {"total": int(total.value), "runs": [int(x) for x in runs], "bases": [int(x) for x in bases]}

    def store_runs(self, rank: int, keys=None, starts=None, counts=None, firsts=None, descending: bool = False,
                   key_type: Optional[int] = None) -> int:
        """lsb_store_runs: the runs that start on `rank` into device columns
        (1-D contiguous CUDA torch tensors, any of them None): keys with the
        key type and order the load was given, starts and counts int64, firsts
        any 4- or 8-byte dtype (4: the value's low word).  counts needs
        starts.  Every column holds at least the rank's runs; -> that
        number."""
        import torch
        cols = [(t, what) for t, what in ((keys, "keys"), (starts, "starts"), (counts, "counts"),
                                          (firsts, "firsts")) if t is not None]
        if not cols:
            raise ValueError("no output column")
        if counts is not None and starts is None:
            raise ValueError("counts need starts")
        for t, what in cols:
            _check_column(t, what, cols[0][0].device)
        for t, what in ((starts, "starts"), (counts, "counts")):
            if t is not None and t.dtype != torch.int64:
                raise ValueError(f"{what}: not int64")
        cap = min(t.numel() for t, _ in cols)
        kt = _key_type_of(keys, key_type) if keys is not None else (KEY_U64 if key_type is None else key_type)
        if cap == 0:  # an empty tensor has no address: stand-ins say which outputs are meant (cap 0: never written)
            keys, starts, counts, firsts = (None if t is None else t.new_empty(1)
                                            for t in (keys, starts, counts, firsts))
        vb, fp = (firsts.element_size(), firsts.data_ptr()) if firsts is not None else (0, None)
        torch.cuda.current_stream(cols[0][0].device).synchronize()
        runs = ctypes.c_int64()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _check(_lib().lsb_store_runs(self._h, rank, cap, ptr(keys), kt, ORDER_DESCENDING if descending else 0,
                                     ptr(starts), ptr(counts), fp, vb, ctypes.byref(runs)), "lsb_store_runs")
        return int(runs.value)

    def plan_reduce(self, op: int, val_type: int) -> None:
        """lsb_plan_reduce: after count_runs, what the later ranks add to each
        rank's last run under op (REDUCE_SUM, REDUCE_MIN, REDUCE_MAX) over the
        records' values read as val_type (KEY_U64, KEY_I64, KEY_F64); a
        collective in a one-rank-per-process world.  store_reduce needs it."""
        _check(_lib().lsb_plan_reduce(self._h, op, val_type), "lsb_plan_reduce")

    def store_reduce(self, rank: int, out) -> int:
        """lsb_store_reduce: out[j] = the planned reduction over the values of
        the j-th run that starts on `rank`, the indices of store_runs.  out: a
        1-D contiguous CUDA torch tensor of 8-byte elements that holds at
        least the rank's runs; -> that number."""
        import torch
        _check_column(out, "out")
        if out.element_size() != 8:
            raise ValueError("out: not 8-byte elements")
        cap = out.numel()
        if cap == 0:  # an empty tensor has no address (cap 0: never written)
            out = out.new_empty(1)
        torch.cuda.current_stream(out.device).synchronize()
        runs = ctypes.c_int64()
        _check(_lib().lsb_store_reduce(self._h, rank, cap, out.data_ptr(), ctypes.byref(runs)), "lsb_store_reduce")
        return int(runs.value)

    def label_runs(self, mode: int) -> None:
        """lsb_label_runs: after count_runs, every record of every local rank
        gets the global index of its run as its value: LABEL_KEEP leaves the
        key, LABEL_BY_VALUE makes the old value the key (with index values, a
        my_sort() after it puts the ids in input order: the inverse).  The
        records change, so the plans end: count_runs again before a store."""
        _check(_lib().lsb_label_runs(self._h, mode), "lsb_label_runs")

    def plan_scan(self, op: int, val_type: int) -> None:
        """lsb_plan_scan: after count_runs, what the earlier tiles and ranks
        add to every record's run under op (SCAN_SUM, SCAN_MIN, SCAN_MAX over
        the values read as KEY_U64, KEY_I64 or KEY_F64; SCAN_COUNT, SCAN_START
        with KEY_U64); a collective in a one-rank-per-process world.
        store_scan and scan_runs need it."""
        _check(_lib().lsb_plan_scan(self._h, op, val_type), "lsb_plan_scan")

    def store_scan(self, rank: int, out) -> int:
        """lsb_store_scan: out[i] = the planned scan's result for the record
        at slot i of `rank`.  out: a 1-D contiguous CUDA torch tensor of
        8-byte elements that holds at least the rank's records; -> that
        number."""
        import torch
        _check_column(out, "out")
        if out.element_size() != 8:
            raise ValueError("out: not 8-byte elements")
        cap = out.numel()
        if cap == 0:  # an empty tensor has no address (cap 0: never written)
            out = out.new_empty(1)
        torch.cuda.current_stream(out.device).synchronize()
        count = ctypes.c_int64()
        _check(_lib().lsb_store_scan(self._h, rank, cap, out.data_ptr(), ctypes.byref(count)), "lsb_store_scan")
        return int(count.value)

    def scan_runs(self, mode: int) -> None:
        """lsb_scan_runs: after plan_scan, every record of every local rank
        gets the scan's result as its value: LABEL_KEEP leaves the key,
        LABEL_BY_VALUE makes the old value the key (with index values, a
        my_sort() after it puts the results in input order).  The records
        change, so the plans end."""
        _check(_lib().lsb_scan_runs(self._h, mode), "lsb_scan_runs")

    def select(self, k: int) -> dict:
        """lsb_select: the key the stable sort would put at global position k
        and the plan of the first k + 1 records, without sorting (a collective
        in a one-rank-per-process world; every A stays as it is, every B is
        scratch).  {"key": the mapped uint64 key (key_decode gives the typed
        bits), "below", "equal": records of the array below and equal to it,
        "take": [P] records each rank gives, "bases": [P] where each rank's
        part starts}; store_select needs it, after the last change of the
        records."""
        key = ctypes.c_uint64()
        below, equal = ctypes.c_int64(), ctypes.c_int64()
        take = np.zeros(self.P, dtype=np.int64)
        bases = np.zeros(self.P, dtype=np.int64)
        _check(_lib().lsb_select(self._h, k, ctypes.byref(key), ctypes.byref(below), ctypes.byref(equal),
                                 take.ctypes.data, bases.ctypes.data), "lsb_select")
        return {"key": int(key.value), "below": int(below.value), "equal": int(equal.value),
                "take": [int(x) for x in take], "bases": [int(x) for x in bases]}

    def store_select(self, rank: int, keys=None, values=None, descending: bool = False,
                     key_type: Optional[int] = None, val_bytes: Optional[int] = None) -> int:
        """lsb_store_select: `rank`'s part of the selection into device columns
        (1-D contiguous CUDA torch tensors, either may be None), in slot
        order: keys with the key type and order the load was given, values any
        4- or 8-byte dtype (4: the value's low word; val_bytes= overrides the
        element size).  Every column holds at least the rank's part; -> its
        length."""
        import torch
        cols = [(t, what) for t, what in ((keys, "keys"), (values, "values")) if t is not None]
        if not cols:
            raise ValueError("no output column")
        for t, what in cols:
            _check_column(t, what, cols[0][0].device)
        cap = min(t.numel() for t, _ in cols)
        kt = _key_type_of(keys, key_type) if keys is not None else (KEY_U64 if key_type is None else key_type)
        if cap == 0:  # an empty tensor has no address: stand-ins say which outputs are meant (cap 0: never written)
            keys, values = (None if t is None else t.new_empty(1) for t in (keys, values))
        vb, vp = (values.element_size() if val_bytes is None else val_bytes, values.data_ptr()) \
            if values is not None else (0 if val_bytes is None else val_bytes, None)
        torch.cuda.current_stream(cols[0][0].device).synchronize()
        count = ctypes.c_int64()
        _check(_lib().lsb_store_select(self._h, rank, cap, None if keys is None else keys.data_ptr(), kt,
                                       ORDER_DESCENDING if descending else 0, vp, vb, ctypes.byref(count)),
               "lsb_store_select")
        return int(count.value)

    def last_select(self) -> tuple:
        """(histogram rounds, records read on the local ranks) of the last
        select (lsb_get_last_select)."""
        rounds, read = ctypes.c_int(), ctypes.c_int64()
        _check(_lib().lsb_get_last_select(self._h, ctypes.byref(rounds), ctypes.byref(read)), "lsb_get_last_select")
        return int(rounds.value), int(read.value)

    def search(self, rank: int, queries, out, side: str = "left", add: bool = False, descending: bool = False,
               key_type: Optional[int] = None) -> None:
        """lsb_search: for every query, the records of `rank` (sorted) whose
        key is below it (side="left"), not above it ("right") or equal to it
        ("count"), in the mapped keys' order, into out (add=True: added to
        it).  queries: a 1-D contiguous CUDA torch tensor read with the key
        type and order the load was given; out: int64, the same length and
        device, no byte shared with queries.  Local, no collective: the sum
        over the ranks is the answer for the whole array."""
        import torch
        if side not in _SEARCH_SIDES:
            raise ValueError(f"side {side!r}: not one of {sorted(_SEARCH_SIDES)}")
        _check_column(queries, "queries")
        kt = _key_type_of(queries, key_type)
        _check_column(out, "out", queries.device)
        if out.dtype != torch.int64:
            raise ValueError("out: not int64")
        if out.numel() != queries.numel():
            raise ValueError("queries and out differ in length")
        m = queries.numel()
        torch.cuda.current_stream(queries.device).synchronize()
        _check(_lib().lsb_search(self._h, rank, m, queries.data_ptr() if m else None, kt,
                                 ORDER_DESCENDING if descending else 0,
                                 _SEARCH_SIDES[side] | (SEARCH_ADD if add else 0), out.data_ptr() if m else None),
               "lsb_search")

    def lookup(self, rank: int, queries, values=None, found=None, descending: bool = False,
               key_type: Optional[int] = None, val_bytes: Optional[int] = None) -> None:
        """lsb_lookup: for every query with a record of its key on `rank`
        (sorted), values[i] = the value of the first such record (a 4-byte
        dtype gets the low word; val_bytes= overrides the element size) and
        found[i] = 1 (a uint8 or bool column); a query without one leaves both
        elements as they are.  queries as for search(); values and found the
        queries' length, on their device, no byte shared; either may be None,
        not both.  Local, no collective: called from the last rank to the
        first, the lowest rank's match stands."""
        import torch
        _check_column(queries, "queries")
        kt = _key_type_of(queries, key_type)
        if values is None and found is None:
            raise ValueError("no output column")
        m = queries.numel()
        if values is not None:
            _check_column(values, "values", queries.device)
            if values.numel() != m:
                raise ValueError("queries and values differ in length")
        if found is not None:
            if not isinstance(found, torch.Tensor) or not found.is_cuda or found.device != queries.device:
                raise ValueError("found: not a tensor on the queries' GPU")
            if found.dtype not in (torch.uint8, torch.bool) or found.dim() != 1 or not found.is_contiguous():
                raise ValueError("found: not a 1-D contiguous uint8 or bool column")
            if found.numel() != m:
                raise ValueError("queries and found differ in length")
        vb = 0 if values is None else (values.element_size() if val_bytes is None else val_bytes)
        torch.cuda.current_stream(queries.device).synchronize()
        _check(_lib().lsb_lookup(self._h, rank, m, queries.data_ptr() if m else None, kt,
                                 ORDER_DESCENDING if descending else 0,
                                 None if values is None else (values.data_ptr() if m else values.new_empty(1).data_ptr()),
                                 vb, None if found is None else (found.data_ptr() if m else found.new_empty(1).data_ptr())),
               "lsb_lookup")

    def join_count(self, rank: int, queries, counts=None, descending: bool = False,
                   key_type: Optional[int] = None) -> int:
        """lsb_join_count: `rank`'s join plan for these queries (kept by the
        library until the records change or the rank counts again) -> the
        pairs it holds.  counts (optional): int64, the queries' length and
        device, no byte shared: the matches of every query on this rank."""
        import torch
        _check_column(queries, "queries")
        kt = _key_type_of(queries, key_type)
        m = queries.numel()
        if counts is not None:
            _check_column(counts, "counts", queries.device)
            if counts.dtype != torch.int64:
                raise ValueError("counts: not int64")
            if counts.numel() != m:
                raise ValueError("queries and counts differ in length")
        torch.cuda.current_stream(queries.device).synchronize()
        total = ctypes.c_int64()
        _check(_lib().lsb_join_count(self._h, rank, m, queries.data_ptr() if m else None, kt,
                                     ORDER_DESCENDING if descending else 0,
                                     counts.data_ptr() if counts is not None and m else None, ctypes.byref(total)),
               "lsb_join_count")
        return int(total.value)

    def store_join(self, rank: int, left=None, right=None, pos=None, query_base: int = 0,
                   val_bytes: Optional[int] = None) -> int:
        """lsb_store_join: the pairs of `rank`'s join plan into device columns
        (1-D contiguous CUDA torch tensors, any may be None, not all): left =
        query_base + the query's index and pos = the record's global position
        (both int64), right = the record's value (any 4- or 8-byte dtype; 4:
        the low word; val_bytes= overrides the element size).  Ordered by
        query, then by record.  Every column holds at least the rank's pairs;
        -> their number."""
        import torch
        cols = [(t, what) for t, what in ((left, "left"), (right, "right"), (pos, "pos")) if t is not None]
        if not cols:
            raise ValueError("no output column")
        for t, what in cols:
            _check_column(t, what, cols[0][0].device)
            if what != "right" and t.dtype != torch.int64:
                raise ValueError(f"{what}: not int64")
        cap = min(t.numel() for t, _ in cols)
        if cap == 0:  # an empty tensor has no address: stand-ins say which outputs are meant (cap 0: never written)
            left, right, pos = (None if t is None else t.new_empty(1) for t in (left, right, pos))
        vb = 0 if right is None else (right.element_size() if val_bytes is None else val_bytes)
        torch.cuda.current_stream(cols[0][0].device).synchronize()
        count = ctypes.c_int64()
        _check(_lib().lsb_store_join(self._h, rank, cap, query_base, None if left is None else left.data_ptr(),
                                     None if right is None else right.data_ptr(), vb,
                                     None if pos is None else pos.data_ptr(), ctypes.byref(count)),
               "lsb_store_join")
        return int(count.value)

    def scatter_global(self, arr: np.ndarray) -> None:
        """Load a global array of n records into the block partition."""
        arr = np.ascontiguousarray(arr, dtype=ELEM_DTYPE)
        if arr.size != self.n:
            raise ValueError("need exactly n records")
        for r in self.local_ranks:
            h = self.here(r)
            if h:
                self.copy_in(r, arr[r * self.per: r * self.per + h])

    def gather_global(self) -> np.ndarray:
        """A[0:n] in global order (every rank must be local)."""
        if len(self.local_ranks) != self.P:
            raise RuntimeError("gather_global needs all ranks in this process")
        parts = [self.copy_out(r) for r in range(self.P)]
        return np.concatenate(parts) if parts else np.empty(0, dtype=ELEM_DTYPE)

    # -- the hot path -------------------------------------------------------
    def my_sort(self) -> None:
        _check(_lib().lsb_sort(self._h), "lsb_sort")

    def global_shuffle(self, digit: int) -> None:
        _check(_lib().lsb_pass(self._h, digit), "lsb_pass")

    mySort = my_sort
    globalShuffle = global_shuffle

    def sync(self) -> None:
        _check(_lib().lsb_sync(self._h), "lsb_sync")

    def barrier(self) -> None:
        _check(_lib().lsb_barrier(self._h), "lsb_barrier")

    # -- checks ---------------------------------------------------------------
    def verify(self):
        """(ok, first_bad_global_index) of the O(n) stable-sort invariant."""
        bad = ctypes.c_int64(-1)
        rc = _lib().lsb_verify(self._h, ctypes.byref(bad))
        if rc not in (LSB_OK, LSB_ERR_VERIFY):
            _check(rc, "lsb_verify")
        return rc == LSB_OK, int(bad.value)

    def check_sorted(self) -> bool:
        s = ctypes.c_int(0)
        _check(_lib().lsb_check_sorted(self._h, ctypes.byref(s)), "lsb_check_sorted")
        return bool(s.value)

    checkSorted = check_sorted

    def print_lines(self, name: str = "A", n_per_rank: int = 10):
        """The lines DistributedArray::print emits (mpi/mpi_lsbsort.cpp:171-200)."""
        lines = []
        if n_per_rank * self.P >= self.n:
            lines.append(f"{name}: displaying all {self.n} elements")
        else:
            lines.append(f"{name}: displaying first {n_per_rank} elements on each rank"
                         f" out of {self.n} elements")
        for r in self.local_ranks:
            h = self.here(r)
            k = min(n_per_rank, h)
            for i, e in enumerate(self.copy_out(r, 0, k)):
                lines.append(f"{name}[{r * self.per + i}] = ({int(e['key']):016x},{int(e['val'])})")
            if k < h:
                lines.append("...")
        return lines

    # -- measurement ----------------------------------------------------------
    def set_timing(self, on: bool = True) -> None:
        self.set_option(OPT_TIMING, 1 if on else 0)

    def last_sort(self) -> tuple:
        """(local 8-bit passes, exchanges, varying key bits) of the last my_sort."""
        lp, ex, vb = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        _check(_lib().lsb_get_last_sort(self._h, ctypes.byref(lp), ctypes.byref(ex), ctypes.byref(vb)),
               "lsb_get_last_sort")
        return int(lp.value), int(ex.value), int(vb.value)

    def first_pass(self) -> int:
        """How the last my_sort began (lsb_get_first_pass): FIRST_COUNT,
        FIRST_REGIONAL or FIRST_REGIONAL_REDONE."""
        f = ctypes.c_int()
        _check(_lib().lsb_get_first_pass(self._h, ctypes.byref(f)), "lsb_get_first_pass")
        return int(f.value)

    def last_records(self) -> int:
        """The records the last my_sort's passes handed each other
        (lsb_get_last_records): RECORDS_FULL, RECORDS_PACKED or
        RECORDS_PACKED_REDONE."""
        f = ctypes.c_int()
        _check(_lib().lsb_get_last_records(self._h, ctypes.byref(f)), "lsb_get_last_records")
        return int(f.value)

    def last_packed_tile(self) -> int:
        """Records per tile of the last my_sort's packed middle passes
        (lsb_get_last_packed_tile; LSB_PACKED_TILE): 0 when none ran."""
        f = ctypes.c_int()
        _check(_lib().lsb_get_last_packed_tile(self._h, ctypes.byref(f)), "lsb_get_last_packed_tile")
        return int(f.value)

    def last_pass_tiles(self) -> list:
        """Records per tile of each local pass of the last my_sort, in pass
        order (lsb_get_last_pass_tiles; LSB_PACKED_TILE, LSB_EDGE_TILES):
        0 for a pass that was no k_onesweep launch."""
        t = (ctypes.c_int * 16)()
        n = ctypes.c_int()
        _check(_lib().lsb_get_last_pass_tiles(self._h, t, 16, ctypes.byref(n)), "lsb_get_last_pass_tiles")
        return [int(t[i]) for i in range(n.value)]

    def kernel_stats(self) -> dict:
        out = {}
        for kid, name in enumerate(KERNEL_NAMES):
            n = ctypes.c_int64()
            ms = ctypes.c_double()
            _check(_lib().lsb_get_kernel_stats(self._h, kid, ctypes.byref(n), ctypes.byref(ms)),
                   "lsb_get_kernel_stats")
            out[name] = (int(n.value), float(ms.value))
        return out

    def pass_stats(self) -> list:
        """Per local pass that ran since the last reset (lsb_get_pass_stats):
        dicts with pass, shift, launches, elems and the device ms of its count,
        scatter, exchange and placement work, summed over launches."""
        out = []
        for p in range(MAX_PASSES):
            sh, la, el = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
            ms = [ctypes.c_double() for _ in range(4)]
            _check(_lib().lsb_get_pass_stats(self._h, p, ctypes.byref(sh), ctypes.byref(la), ctypes.byref(el),
                                             *[ctypes.byref(x) for x in ms]), "lsb_get_pass_stats")
            if sh.value < 0:
                continue
            xb, wire, tail = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _check(_lib().lsb_get_pass_exchange(self._h, p, ctypes.byref(xb), ctypes.byref(wire),
                                                ctypes.byref(tail)), "lsb_get_pass_exchange")
            out.append({"pass": p, "shift": int(sh.value), "launches": int(la.value), "elems": int(el.value),
                        "ms_count": ms[0].value, "ms_scatter": ms[1].value, "ms_exchange": ms[2].value,
                        "ms_place": ms[3].value, "exchange_bytes": int(xb.value), "ms_wire": wire.value,
                        "ms_place_tail": tail.value})
        return out

    def placement(self, rank: Optional[int] = None) -> dict:
        """lsb_get_placement: how rank's A and B were chosen among candidate
        buffers (candidates 0: allocated as they came) and the probe copy's ms
        for the chosen pair, the first two allocated and the slowest pair."""
        r = self.local_ranks[0] if rank is None else rank
        k = ctypes.c_int()
        ms = [ctypes.c_double() for _ in range(3)]
        _check(_lib().lsb_get_placement(self._h, r, ctypes.byref(k), *[ctypes.byref(x) for x in ms]),
               "lsb_get_placement")
        return {"candidates": int(k.value), "chosen_ms": round(ms[0].value, 4),
                "first_pair_ms": round(ms[1].value, 4), "worst_ms": round(ms[2].value, 4)}

    def exchange_stats(self) -> dict:
        """lsb_get_exchange_stats: the exchange steps since the last reset
        (bytes per peer, wire / plan / placement / tail ms, placement bytes)."""
        st = ExchangeStats()
        _check(_lib().lsb_get_exchange_stats(self._h, ctypes.byref(st)), "lsb_get_exchange_stats")
        return {"exchanges": int(st.exchanges), "calls": int(st.calls),
                "sent_bytes": [int(x) for x in st.sent_bytes[:self.P]],
                "recv_bytes": [int(x) for x in st.recv_bytes[:self.P]],
                "wire_ms": st.wire_ms, "plan_ms": st.plan_ms, "place_ms": st.place_ms,
                "place_tail_ms": st.place_tail_ms, "place_bytes": int(st.place_bytes),
                "placed_records": int(st.placed_records), "counted_records": int(st.counted_records)}

    def reset_kernel_stats(self) -> None:
        _check(_lib().lsb_reset_kernel_stats(self._h), "lsb_reset_kernel_stats")

    def scatter_elems(self) -> int:
        e = ctypes.c_int64()
        _check(_lib().lsb_get_scatter_elems(self._h, ctypes.byref(e)), "lsb_get_scatter_elems")
        return int(e.value)

    def exchange_bytes(self) -> tuple:
        """(calls, bytes, largest call's bytes) handed to the all-to-all collective."""
        c, b, mx = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(_lib().lsb_get_exchange_bytes(self._h, ctypes.byref(c), ctypes.byref(b), ctypes.byref(mx)),
               "lsb_get_exchange_bytes")
        return int(c.value), int(b.value), int(mx.value)


def mySort(world: World) -> None:  # noqa: N802 - reference name
    world.my_sort()


def globalShuffle(world: World, digit: int) -> None:  # noqa: N802 - reference name
    world.global_shuffle(digit)
