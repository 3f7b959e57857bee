#!/usr/bin/env python3
"""Rate of lsb_search against torch.searchsorted on the key
column the library's caller would otherwise have to store.

One process, one GPU, n = 2^28 records and m = 2^24 queries by default.  The
keys are uniform in [0, 2^63), loaded as u64 and sorted by the library: below
2^63 the unsigned order is torch's int64 order, so torch can search the same
column.  Query sets, m each:
  uniform   uniform in [0, 2^63): nearly all misses, no two near each other
  sorted    the same queries, sorted: adjacent lanes probe adjacent records
  hits      keys drawn from the sorted column at uniform positions
  one       one key of the column, repeated
Every round times, with torch CUDA events around the blocking calls,
  fence     the first search after a change of A (m = 1: k_search_fence, one
            read of n / 4096 records, and a one-query search) and the same
            search again (the table kept); their difference is the build
  store     lsb_store_columns of the sorted keys into an 8-byte column, which
            torch needs and the library's caller does not
and per query set
  lower     lsb_search LSB_SEARCH_LOWER
  count     lsb_search LSB_SEARCH_COUNT
  torch     torch.searchsorted(column, queries) into a preallocated result
The rounds interleave the query sets; after one warm-up round the median of at
least 7 is taken.  Round 0 also checks the answers: lower against torch's
left, count against torch's right minus left.  Prints one JSON line.

LSB_LIBRARY names another build of the same ABI, as everywhere; --label names
it in the output (an alternative index form measured against the tree's).

torch is imported before the library is loaded: the two then share one HIP
runtime.
"""
import argparse
import json
import os
import statistics
import sys

import torch  # before lsbsort loads the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-lsb_amd"))
import lsbsort as L  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--log2m", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="tree", help="names the library build in the output")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    n, m = 1 << args.log2n, 1 << args.log2m
    rounds = max(7, args.rounds)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(28)
    col = torch.empty(n, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int64, device=dev)
    tout = torch.empty(m, dtype=torch.int64, device=dev)
    one_q = torch.zeros(1, dtype=torch.int64, device=dev)
    one_out = torch.zeros(1, dtype=torch.int64, device=dev)
    times = {"first_search": [], "repeat_search": [], "store": []}
    checked = {}
    with L.World(n, ranks=1) as w:
        keys = torch.randint(0, (1 << 63) - 1, (n,), dtype=torch.int64, device=dev, generator=gen)
        w.load_columns(0, keys, None, key_type=L.KEY_U64)
        del keys
        w.my_sort()
        w.store_columns(0, col, None, key_type=L.KEY_U64)
        first_record = w.copy_out(0, 0, 1)
        uniform = torch.randint(0, (1 << 63) - 1, (m,), dtype=torch.int64, device=dev, generator=gen)
        queries = {
            "uniform": uniform,
            "sorted": torch.sort(uniform).values,
            "hits": col[torch.randint(0, n, (m,), device=dev, generator=gen)],
            "one": col[n // 3].repeat(m),
        }
        qtimes = {name: {"lower": [], "count": [], "torch": []} for name in queries}
        for rnd in range(rounds + 1):  # round 0 warms up
            w.copy_in(0, first_record)  # the same record again: A is unchanged, its fence table is dropped
            t = {"first_search": timed(lambda: w.search(0, one_q, one_out, key_type=L.KEY_U64)),
                 "repeat_search": timed(lambda: w.search(0, one_q, one_out, key_type=L.KEY_U64)),
                 "store": timed(lambda: w.store_columns(0, col, None, key_type=L.KEY_U64))}
            if rnd:
                for k, v in t.items():
                    times[k].append(v)
            for name, q in queries.items():
                tq = {"lower": timed(lambda: w.search(0, q, out, side="left", key_type=L.KEY_U64))}
                if rnd == 0:
                    left = torch.searchsorted(col, q)
                    ok = bool(torch.equal(out, left))
                tq["count"] = timed(lambda: w.search(0, q, out, side="count", key_type=L.KEY_U64))
                if rnd == 0:
                    checked[name] = ok and bool(torch.equal(out, torch.searchsorted(col, q, right=True) - left))
                    del left
                tq["torch"] = timed(lambda: torch.searchsorted(col, q, out=tout))
                if rnd:
                    for k, v in tq.items():
                        qtimes[name][k].append(v)
    md = {k: statistics.median(times[k]) for k in ("first_search", "repeat_search", "store")}
    res = {"tool": "search_rate", "library": args.label, "n": n, "m": m, "rounds": rounds,
           "device": torch.cuda.get_device_name(0),
           "first_search_ms": round(md["first_search"], 4), "repeat_search_ms": round(md["repeat_search"], 4),
           "fence_build_ms": round(md["first_search"] - md["repeat_search"], 4),
           "store_columns_ms": round(md["store"], 4), "queries": {}}
    for name in queries:
        mq = {k: statistics.median(v) for k, v in qtimes[name].items()}
        res["queries"][name] = {
            "matches_torch": checked[name],
            "lower_ms": round(mq["lower"], 4), "count_ms": round(mq["count"], 4), "torch_ms": round(mq["torch"], 4),
            "lower_mq_per_s": round(m / mq["lower"] / 1e3, 1), "torch_mq_per_s": round(m / mq["torch"] / 1e3, 1),
            "torch_over_lower": round(mq["torch"] / mq["lower"], 4),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
