#!/usr/bin/env python3
"""Times of lsb_select and lsb_store_select against one
streaming read of A by this library, the full sort a caller runs today, and
torch.kthvalue / torch.topk on the key column.

One process, one GPU, n = 2^28 records by default, P = 1, k = n / 2.  Inputs,
loaded with index values:
  uniform64  int64 keys of 64 random bits (the mapped keys are uniform u64)
  d65536     2^16 distinct values in a random order
  one        one value
  uniform32  int32 keys of 32 random bits (the mapped keys are uniform u32)
  top3       three values of the top byte over 56 random bits: the chosen
             bucket holds a third of the records, the compaction's dense case
Every round times, with torch CUDA events around the blocking calls,
  load       lsb_load_columns
  select     lsb_select(k = n / 2): every round's kernel, its gather and the
             host's choice of the bucket
  select_lo  lsb_select(k = 1023), what topk(1024) runs
  store      lsb_store_select of those 1024 records (keys and values)
  count      lsb_count_runs on the same records: one streaming read of A by
             this library and a trip to the host
  sort       lsb_sort (with load: what a caller pays today for one slot of
             the result)
  kthvalue   torch.kthvalue(keys, n / 2 + 1)
  topk       torch.topk(keys, 1024, largest=False)
The rounds interleave the inputs and the yardsticks; after one warm-up round
the median of at least 5 is taken.  Prints one JSON line: per input the medians
in ms, the select's rounds and records read, and the ratios select / count
(the bytes predict about 2 for uniform 64-bit keys; 3 is the line),
(load + sort) / select, kthvalue / select and topk / (select_lo + store).

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

TOP = 1024


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    n = 1 << args.log2n
    k = n // 2
    rounds = max(5, args.rounds)
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    perm = torch.randperm(n, dtype=torch.int64, device=dev)

    def word():
        return torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=dev)

    inputs = {
        "uniform64": (word() << 32) | word(),
        "d65536": perm >> max(args.log2n - 16, 0),
        "one": torch.zeros_like(perm),
        "top3": (torch.randint(0, 3, (n,), dtype=torch.int64, device=dev) << 56) | (word() << 24) | (word() >> 8),
        "uniform32": torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device=dev),
    }
    del perm
    out_k = {name: torch.empty(TOP, dtype=keys.dtype, device=dev) for name, keys in inputs.items()}
    out_v = torch.empty(TOP, dtype=torch.int64, device=dev)
    names = ("load", "select", "select_lo", "store", "count", "sort", "kthvalue", "topk")
    times = {name: {t: [] for t in names} for name in inputs}
    ran, checked = {}, {}
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, keys in inputs.items():
                t, plan, lo = {}, {}, {}
                t["load"] = timed(lambda: w.load_columns(0, keys, None))
                t["select"] = timed(lambda: plan.update(w.select(k)))
                ran[name] = w.last_select()
                t["select_lo"] = timed(lambda: lo.update(w.select(TOP - 1)))
                t["store"] = timed(lambda: w.store_select(0, out_k[name], out_v))
                t["count"] = timed(lambda: w.count_runs())
                t["sort"] = timed(lambda: (w.my_sort(), w.sync()))
                kv, tk = [], []
                t["kthvalue"] = timed(lambda: kv.append(torch.kthvalue(keys, k + 1).values))
                t["topk"] = timed(lambda: tk.append(torch.topk(keys, TOP, largest=False).values))
                if rnd == 0:  # the library's answers are torch's
                    kt = L.KEY_I64 if keys.dtype == torch.int64 else L.KEY_I32
                    bits = L.key_decode(plan["key"], kt)
                    width = 64 if kt == L.KEY_I64 else 32
                    mine = bits - (1 << width) if bits >> (width - 1) else bits
                    checked[name] = bool(mine == int(kv[0]) and lo["take"] == [TOP] and
                                         torch.equal(torch.sort(out_k[name]).values, tk[0]))
                else:
                    for x in names:
                        times[name][x].append(t[x])
                del kv, tk
    res = {"tool": "select_rate", "n": n, "k": k, "top": TOP, "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "library": os.path.relpath(L.LIB_PATH, ROOT), "inputs": {}}
    for name in inputs:
        md = {x: statistics.median(v) for x, v in times[name].items()}
        row = {f"{x}_ms": round(md[x], 4) for x in names}
        row.update({
            "rounds": ran[name][0], "records_read": ran[name][1], "reads_of_A": round(ran[name][1] / n, 4),
            "matches_torch": checked[name],
            "select_over_count": round(md["select"] / md["count"], 4),
            "load_sort_over_select": round((md["load"] + md["sort"]) / md["select"], 4),
            "kthvalue_over_select": round(md["kthvalue"] / md["select"], 4),
            "topk_over_select_lo_store": round(md["topk"] / (md["select_lo"] + md["store"]), 4),
        })
        res["inputs"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
