#!/usr/bin/env python3
"""Rates of lsb_count_runs / lsb_store_runs against a device
copy of the same bytes and against torch.unique_consecutive.

One process, one GPU, n = 2^28 records by default.  Inputs: sorted u64 keys
  distinct   every key once (n runs)
  d65536     2^16 distinct values (runs of n / 2^16)
  one        one value (one run)
loaded with index values.  Every round times, with torch CUDA events around
the blocking calls, count_runs (k_run_count + k_run_scan, the summary's trip
to the host and the planner), store_runs with all four outputs (k_run_write +
k_run_diff), beside each a torch.Tensor.copy_ that moves as many bytes as the
kernels' algorithmic bytes (count: 16 n read; store: 16 n read + 40 bytes per
run: k_run_write writes key, start and first value, 24 bytes, k_run_diff
reads the start and writes the count, 16), half of them read and half
written, and torch.unique_consecutive(return_counts=True) on the same key
column.  The rounds interleave the inputs and the copies; after one warm-up
round the median of at least 5 is taken.  Prints one JSON line:
per input the medians in ms, ratio = copy time / call time (1.0: parity with
the copy) and the speed-up over unique_consecutive for count + store.

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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    n = 1 << args.log2n
    rounds = max(5, args.rounds)
    dev = torch.device("cuda", 0)
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    inputs = {"distinct": pos, "d65536": pos >> max(args.log2n - 16, 0), "one": torch.zeros_like(pos)}
    runs_of = {"distinct": n, "d65536": min(n, 1 << 16), "one": 1}
    outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    src = torch.empty(32 * n, dtype=torch.uint8, device=dev).fill_(1)  # the largest copy: 56 n bytes moved
    dst = torch.empty_like(src)
    names = ("count", "copy_count", "store", "copy_store", "unique_consecutive")
    times = {name: {k: [] for k in names} for name in inputs}
    checked = {}
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, keys in inputs.items():
                m = runs_of[name]
                cb, sb = 16 * n // 2, (16 * n + 40 * m) // 2
                w.load_columns(0, keys, None, key_type=L.KEY_U64)
                t, plan = {}, {}
                t["count"] = timed(lambda: plan.update(w.count_runs()))
                t["copy_count"] = timed(lambda: dst[:cb].copy_(src[:cb]))
                t["store"] = timed(lambda: w.store_runs(0, *[o[:m] for o in outs], key_type=L.KEY_U64))
                t["copy_store"] = timed(lambda: dst[:sb].copy_(src[:sb]))
                uc = []
                t["unique_consecutive"] = timed(lambda: uc.extend(torch.unique_consecutive(keys, return_counts=True)))
                if rnd == 0:  # the library's answer is torch's
                    k, s, c, f = (o[:m] for o in outs)
                    checked[name] = bool(plan["total"] == m and torch.equal(k, uc[0]) and torch.equal(c, uc[1]) and
                                         torch.equal(s, f) and torch.equal(s, torch.cumsum(c, 0) - c))
                else:
                    for k, v in t.items():
                        times[name][k].append(v)
                del uc
    res = {"tool": "runs_rate", "n": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "inputs": {}}
    for name in inputs:
        md = {k: statistics.median(v) for k, v in times[name].items()}
        m = runs_of[name]
        res["inputs"][name] = {
            "runs": m, "matches_torch": checked[name],
            "count_ms": round(md["count"], 4), "copy_count_ms": round(md["copy_count"], 4),
            "store_ms": round(md["store"], 4), "copy_store_ms": round(md["copy_store"], 4),
            "unique_consecutive_ms": round(md["unique_consecutive"], 4),
            "count_gbs": round(16 * n / md["count"] / 1e6, 1),
            "store_gbs": round((16 * n + 40 * m) / md["store"] / 1e6, 1),
            "count_ratio": round(md["copy_count"] / md["count"], 4),
            "store_ratio": round(md["copy_store"] / md["store"], 4),
            "vs_unique_consecutive": round(md["unique_consecutive"] / (md["count"] + md["store"]), 4),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
