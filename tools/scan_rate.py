#!/usr/bin/env python3
"""Rates of lsb_plan_scan / lsb_store_scan / lsb_scan_runs
over their algorithmic bytes, and the same answers from torch.

One process, one GPU, n = 2^28 records by default.  Inputs, as
tools/reduce_rate.py: sorted u64 keys
  distinct   every key once (n runs)
  d65536     2^16 distinct values (runs of n / 2^16)
  one        one value (one run)
with the position as the value (int64, or the same number as a double).
Forms: sum over u64, sum over f64, count (cumcount).  Every round times, with
torch CUDA events around the blocking calls, per input and form
  plan     lsb_plan_scan (k_run_scan_tile + k_run_scan_chain, the trail
           word's and the error word's trips to the host): 16 n bytes read
  store    lsb_store_scan (k_run_scan_write into a column and the error
           word's trip): 16 n read, 8 n written
  records  lsb_scan_runs(KEEP) (k_run_scan_write into B): 16 n read, 16 n
           written
  torch    the answer from what the library gave before the scan: the runs'
           starts (lsb_store_runs) and the run id of every record (the key
           column is the run id in all three inputs).  Sums: torch.cumsum over
           the sorted values minus each run's offset spread back through the
           run ids; count: arange - starts[ids].  4 rounds.
The rounds interleave the inputs and forms; after one warm-up round the median
of at least 5 is taken.  Prints one JSON line: the medians in ms, GB/s over
the algorithmic bytes, whether the library's answer is torch's (integers: equal;
doubles: rtol 1e-12 against torch's integer answer, because torch's own cumsum
of the doubles passes 2^53 over 2^28 positions and loses the low bits when a
run's offset is taken off it), and torch's time over plan + store.

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


def torch_cumsum(vals, ids, starts):
    c = torch.cumsum(vals, 0)
    return c - (c[starts] - vals[starts])[ids]


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
    fpos = pos.to(torch.float64)
    inputs = {"distinct": pos, "d65536": pos >> max(args.log2n - 16, 0), "one": torch.zeros_like(pos)}
    runs_of = {"distinct": n, "d65536": min(n, 1 << 16), "one": 1}
    # form -> (op, value type, the value column, torch's answer from (values, run ids, starts))
    forms = {
        "sum_u64": (L.SCAN_SUM, L.KEY_U64, pos, torch_cumsum),
        "sum_f64": (L.SCAN_SUM, L.KEY_F64, fpos, torch_cumsum),
        "count": (L.SCAN_COUNT, L.KEY_U64, pos, lambda vals, ids, starts: pos - starts[ids]),
    }
    out = torch.empty(n, dtype=torch.int64, device=dev)
    starts = torch.empty(n, dtype=torch.int64, device=dev)
    times = {name: {f: {k: [] for k in ("plan", "store", "records", "torch")} for f in forms} for name in inputs}
    checked = {name: {} for name in inputs}
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, keys in inputs.items():
                m = runs_of[name]
                for fname, (op, vt, vals, torch_scan) in forms.items():
                    w.load_columns(0, keys, vals, key_type=L.KEY_U64)
                    assert w.count_runs()["total"] == m
                    w.store_runs(0, starts=starts[:m])
                    t = {}
                    t["plan"] = timed(lambda: w.plan_scan(op, vt))
                    t["store"] = timed(lambda: w.store_scan(0, out))
                    if rnd <= 4:
                        t["torch"] = timed(lambda: torch_scan(vals, keys, starts[:m]))
                    if rnd == 0:  # the library's answer is torch's
                        # The doubles are checked against the integer answer: torch's cumsum of doubles
                        # over all n positions passes 2^53, and taking a run's offset off it cancels.
                        want = torch_scan(pos, keys, starts[:m]).to(vals.dtype)
                        got = out.view(vals.dtype)
                        checked[name][fname] = bool(torch.equal(got, want) if vals.dtype == torch.int64 else
                                                    torch.allclose(got, want, rtol=1e-12, atol=0.0))
                        del want, got
                    t["records"] = timed(lambda: w.scan_runs(L.LABEL_KEEP))
                    if rnd:
                        for k, v in t.items():
                            times[name][fname][k].append(v)
    res = {"tool": "scan_rate", "n": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "inputs": {}}
    for name in inputs:
        res["inputs"][name] = {"runs": runs_of[name], "forms": {}}
        for fname in forms:
            md = {k: statistics.median(v) for k, v in times[name][fname].items()}
            res["inputs"][name]["forms"][fname] = {
                "matches_torch": checked[name][fname],
                "plan_ms": round(md["plan"], 4), "store_ms": round(md["store"], 4),
                "records_ms": round(md["records"], 4), "torch_ms": round(md["torch"], 4),
                "plan_gbs": round(16 * n / md["plan"] / 1e6, 1),
                "store_gbs": round(24 * n / md["store"] / 1e6, 1),
                "records_gbs": round(32 * n / md["records"] / 1e6, 1),
                "plan_store_gbs": round(40 * n / (md["plan"] + md["store"]) / 1e6, 1),
                "torch_ratio": round(md["torch"] / (md["plan"] + md["store"]), 4),
            }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
