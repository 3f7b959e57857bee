#!/usr/bin/env python3
"""Rates of lsb_plan_reduce / lsb_store_reduce against a
device copy of the same bytes, against lsb_store_runs on the same input and
against torch's own per-group reduction.

One process, one GPU, n = 2^28 records by default.  Inputs: sorted u64 keys
  distinct   every key once (n runs)
  d65536     2^16 distinct values (runs of n / 2^16)
  one        one value (one run)
with the position as the value (int64, or the same number as a double).
Forms: sum over u64, sum over f64, min over i64.  Every round times, with
torch CUDA events around the blocking calls, per input and form
  plan     lsb_plan_reduce (one rank: no leading run, nothing launched)
  store    lsb_store_reduce (k_run_reduce + k_run_carry and the error word's
           trip to the host)
  copy     (a) a torch.Tensor.copy_ that moves as many bytes as the kernels'
           algorithmic bytes: 16 n read, 8 written and 8 read-modified per
           run, 16 per 4096-record tile; half of them read, half written
  torch    (c) torch's reduction of the value column by run id (the key
           column is the run id in all three inputs): index_add_ for the
           sums, scatter_reduce_("amin") for the minimum; 3 rounds, or one
           where a call takes over a second (atomics on one address)
and per input
  runs     (b) lsb_store_runs with all four outputs: the same read of A and
           the same head logic without the reduction.
The rounds interleave the inputs, forms and yardsticks; after one warm-up
round the median of at least 5 is taken.  Prints one JSON line: the medians
in ms and the ratios yardstick time / store time (1.0: parity).

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

TILE = 4096


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
    ap.add_argument("--no-torch", action="store_true",
                    help="skip yardstick (c) and the check against it (its contended inputs take minutes)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    n = 1 << args.log2n
    rounds = max(5, args.rounds)
    dev = torch.device("cuda", 0)
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    fpos = pos.to(torch.float64)
    inputs = {"distinct": pos, "d65536": pos >> max(args.log2n - 16, 0), "one": torch.zeros_like(pos)}
    runs_of = {"distinct": n, "d65536": min(n, 1 << 16), "one": 1}
    # form -> (op, value type, the value column, its torch reduction into `out` by run id)
    big = torch.iinfo(torch.int64).max
    forms = {
        "sum_u64": (L.REDUCE_SUM, L.KEY_U64, pos, lambda out, ids, v: out.zero_().index_add_(0, ids, v)),
        "sum_f64": (L.REDUCE_SUM, L.KEY_F64, fpos, lambda out, ids, v: out.zero_().index_add_(0, ids, v)),
        "min_i64": (L.REDUCE_MIN, L.KEY_I64, pos,
                    lambda out, ids, v: out.fill_(big).scatter_reduce_(0, ids, v, "amin")),
    }
    outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    red = torch.empty(n, dtype=torch.int64, device=dev)
    ref = {torch.int64: torch.empty(n, dtype=torch.int64, device=dev),
           torch.float64: torch.empty(n, dtype=torch.float64, device=dev)}
    tiles = -(-n // TILE)
    src = torch.empty((32 * n + 16 * tiles) // 2, dtype=torch.uint8, device=dev).fill_(1)  # the largest copy
    dst = torch.empty_like(src)
    times = {name: {f: {k: [] for k in ("plan", "store", "copy", "torch")} for f in forms} for name in inputs}
    runs_ms = {name: [] for name in inputs}
    checked = {name: {} for name in inputs}
    slow = set()  # (input, form) whose torch yardstick took over a second: timed once
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, keys in inputs.items():
                m = runs_of[name]
                nbytes = (16 * n + 16 * m + 16 * tiles) // 2
                for fname, (op, vt, vals, torch_reduce) in forms.items():
                    w.load_columns(0, keys, vals, key_type=L.KEY_U64)
                    assert w.count_runs()["total"] == m
                    t = {}
                    t["plan"] = timed(lambda: w.plan_reduce(op, vt))
                    t["store"] = timed(lambda: w.store_reduce(0, red[:m]))
                    t["copy"] = timed(lambda: dst[:nbytes].copy_(src[:nbytes]))
                    if rnd <= 3 and not args.no_torch and (name, fname) not in slow:
                        want = ref[vals.dtype][:m]
                        t["torch"] = timed(lambda: torch_reduce(want, keys, vals))
                        if rnd and t["torch"] > 1000.0:
                            slow.add((name, fname))
                    if rnd == 0 and args.no_torch:
                        checked[name][fname] = None
                    elif rnd == 0:  # the library's answer is torch's
                        got = red[:m].view(vals.dtype)
                        checked[name][fname] = bool(torch.equal(got, want) if vals.dtype == torch.int64 else
                                                    torch.allclose(got, want, rtol=1e-12, atol=0.0))
                    else:
                        for k, v in t.items():
                            times[name][fname][k].append(v)
                    if fname == "sum_u64":
                        ms = timed(lambda: w.store_runs(0, *[o[:m] for o in outs], key_type=L.KEY_U64))
                        if rnd:
                            runs_ms[name].append(ms)
    res = {"tool": "reduce_rate", "n": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "inputs": {}}
    for name in inputs:
        m = runs_of[name]
        b_ms = statistics.median(runs_ms[name])
        res["inputs"][name] = {"runs": m, "store_runs_ms": round(b_ms, 4), "forms": {}}
        for fname in forms:
            md = {k: statistics.median(v) if v else None for k, v in times[name][fname].items()}
            tm = md["torch"]
            res["inputs"][name]["forms"][fname] = {
                "matches_torch": checked[name][fname],
                "plan_ms": round(md["plan"], 4), "store_ms": round(md["store"], 4),
                "copy_ms": round(md["copy"], 4), "torch_ms": tm and round(tm, 4),
                "store_gbs": round((16 * n + 16 * m + 16 * tiles) / md["store"] / 1e6, 1),
                "copy_ratio": round(md["copy"] / md["store"], 4),
                "store_runs_ratio": round(b_ms / md["store"], 4),
                "torch_ratio": tm and round(tm / md["store"], 4),
                "plan_share": round(md["plan"] / (md["plan"] + md["store"]), 4),
            }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
