#!/usr/bin/env python3
"""Rate of lsb_lookup and of lsb_join_count + lsb_store_join
against their torch formulations on the columns lsb_store_columns writes.

One process, one GPU, n = 2^28 records and m = 2^24 queries by default.  Three
sets of records, each loaded as u64 keys with index values and sorted by the
library (keys below 2^63, so torch's int64 order is the library's):
  unique   keys uniform in [0, 2^63); queries = keys drawn from the column:
           every query hits one record.  lsb_lookup (8-byte values and the
           found bytes) against torch.searchsorted + gather + compare.
  four     keys uniform in [0, n / 4): about 4 records per value; queries
           uniform in the same range: about 4 pairs per query.
  skewed   the same keys with one value written over n / 64 records; 16
           queries of that value, m / 256 queries that hit elsewhere and all
           others missing: the pairs of 16 queries are nearly all of them.
four and skewed time lsb_join_count, lsb_store_join (left, right and pos) and
their sum against torch's two searchsorted, cumsum, repeat_interleave, index
arithmetic and gather.  Every set also times the lsb_store_columns of the key
and value columns, which torch needs and the library's caller does not.
Per set: one warm-up round, which also checks the library's answers against
torch's, then the median of at least 7 rounds that alternate the library and
torch, with torch CUDA events around the blocking calls.  Prints one JSON line.

LSB_LIBRARY names another build of the same ABI, as everywhere; --label names
it in the output (another tile of outputs measured against the tree's).

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


def torch_lookup(col, vals, q, default):
    idx = torch.searchsorted(col, q).clamp_(max=col.numel() - 1)
    found = col[idx] == q
    return torch.where(found, vals[idx], default), found


def torch_join(col, vals, q):
    lo = torch.searchsorted(col, q)
    c = torch.searchsorted(col, q, right=True) - lo
    off = torch.cumsum(c, 0)
    total = int(off[-1])
    left = torch.repeat_interleave(torch.arange(q.numel(), device=q.device), c, output_size=total)
    p = lo[left] + torch.arange(total, device=q.device) - (off - c)[left]
    return left, vals[p], p


def medians(times):
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


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
    gen.manual_seed(29)
    col = torch.empty(n, dtype=torch.int64, device=dev)
    vals = torch.empty(n, dtype=torch.int64, device=dev)
    res = {"tool": "join_rate", "library": args.label, "n": n, "m": m, "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "sets": {}}
    values = max(1, n // 4)
    hot = values // 3

    def make(name):
        if name == "unique":
            return torch.randint(0, (1 << 63) - 1, (n,), dtype=torch.int64, device=dev, generator=gen)
        keys = torch.randint(0, values, (n,), dtype=torch.int64, device=dev, generator=gen)
        if name == "skewed":
            keys[:max(1, n // 64)] = hot
        return keys

    def queries(name):
        if name == "unique":
            return col[torch.randint(0, n, (m,), device=dev, generator=gen)]
        if name == "four":
            return torch.randint(0, values, (m,), dtype=torch.int64, device=dev, generator=gen)
        q = torch.randint(values, 2 * values, (m,), dtype=torch.int64, device=dev, generator=gen)  # all miss
        at = torch.randperm(m, device=dev, generator=gen)
        few = max(1, m // 256)
        q[at[:few]] = torch.randint(0, values, (few,), dtype=torch.int64, device=dev, generator=gen)
        q[at[few:few + 16]] = hot
        return q

    for name in ("unique", "four", "skewed"):
        with L.World(n, ranks=1) as w:
            keys = make(name)
            w.load_columns(0, keys, None, key_type=L.KEY_U64)
            del keys
            w.my_sort()
            q = None
            times = {"store_columns": []}
            checked = None
            for rnd in range(rounds + 1):  # round 0 warms up and checks
                t = {"store_columns": timed(lambda: w.store_columns(0, col, vals, key_type=L.KEY_U64))}
                if q is None:
                    q = queries(name)
                if name == "unique":
                    out = torch.full((m,), -1, dtype=torch.int64, device=dev)
                    found = torch.zeros(m, dtype=torch.uint8, device=dev)
                    t["lookup"] = timed(lambda: w.lookup(0, q, out, found, key_type=L.KEY_U64))
                    default = torch.full((), -1, dtype=torch.int64, device=dev)
                    got = []
                    t["torch"] = timed(lambda: got.append(torch_lookup(col, vals, q, default)))
                    if rnd == 0:
                        checked = bool(torch.equal(out, got[0][0])) and bool(torch.equal(found.bool(), got[0][1]))
                        hits = int(found.sum())
                    del got, out, found
                else:
                    totals = []
                    t["join_count"] = timed(lambda: totals.append(w.join_count(0, q, key_type=L.KEY_U64)))
                    total = totals[0]
                    left = torch.empty(total, dtype=torch.int64, device=dev)
                    right = torch.empty(total, dtype=torch.int64, device=dev)
                    pos = torch.empty(total, dtype=torch.int64, device=dev)
                    t["store_join"] = timed(lambda: w.store_join(0, left=left, right=right, pos=pos))
                    t["join"] = t["join_count"] + t["store_join"]
                    got = []
                    t["torch"] = timed(lambda: got.append(torch_join(col, vals, q)))
                    if rnd == 0:
                        checked = all(bool(torch.equal(a, b)) for a, b in zip((left, right, pos), got[0]))
                        hits = total
                    del got, left, right, pos
                if rnd:
                    for k, v in t.items():
                        times.setdefault(k, []).append(v)
            md = medians(times)
            entry = {"matches_torch": checked, ("hits" if name == "unique" else "pairs"): hits}
            entry.update({k + "_ms": v for k, v in md.items()})
            mine = md["lookup"] if name == "unique" else md["join"]
            entry["torch_over_library"] = round(md["torch"] / mine, 4)
            entry["torch_with_store_over_library"] = round((md["torch"] + md["store_columns"]) / mine, 4)
            res["sets"][name] = entry
            del q
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
