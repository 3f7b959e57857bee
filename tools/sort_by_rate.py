#!/usr/bin/env python3
"""Rate of the rekey (k_rekey) and of lsbsort.sort_by against
its torch formulation.  One process, one GPU.

--part kernel   n = 2^28 records over an int64 column of n keys (2 GiB):
  lsb_rekey_columns with permuted values (every gather its own cache line),
  with values in order (the streaming case), lsb_rekey_index with divisor 1,
  and lsb_load_columns of the same column at the same count as the streaming
  yardstick.  Median of at least 7 blocking calls between torch CUDA events,
  after one warm-up call whose keys are checked against torch's gather.
  GB/s counts the bytes the call must move: 16 read + 16 written per record,
  plus 8 gathered (rekey by column), or 8 read + 16 written (load).
  LSB_LIBRARY names another build (another E, LSB_REKEY_GROUP); --label
  names it in the output.

--part sort_by  two int64 columns, and (int32, int64), at 2^26 and 2^28 rows:
  lsbsort.sort_by (its World included) against stable torch.sort of the last
  column, gather, stable torch.sort of the primary, gather; and the recipe
  sort_by runs (load, sort, rekey, sort, store) in a World that is kept, which
  leaves out the World's creation (at 2^28 rows its record buffers are large
  enough for the placement probe of DESIGN.md §4).  One warm-up round that
  compares both answers with torch's, then the median of at least 7 rounds
  that alternate the three.  last_round_steps_ms: the kept World's steps,
  each followed by lsb_sync.

Prints one JSON line per part.  torch is imported before the library is
loaded: the two then share one HIP runtime.
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


def median_of(fn, rounds):
    fn()  # warm-up
    return statistics.median(timed(fn) for _ in range(rounds))


def stored_keys(w, n, dev):
    out = torch.empty(n, dtype=torch.int64, device=dev)
    w.store_columns(0, out, None)
    return out


def part_kernel(args, dev, gen):
    n = 1 << args.log2n
    rounds = max(7, args.rounds)
    col = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev, generator=gen)
    res = {"tool": "sort_by_rate", "part": "kernel", "library": args.label, "n": n, "n_col": n, "rounds": rounds,
           "device": torch.cuda.get_device_name(0)}
    with L.World(n, ranks=1) as w:
        for name in ("permuted", "in_order"):
            vals = torch.randperm(n, device=dev, generator=gen) if name == "permuted" else None
            w.load_columns(0, col, vals)
            ms = median_of(lambda: w.rekey(0, col), rounds)
            want = col if vals is None else col[vals]
            res[name] = {"ms": round(ms, 4), "GBps": round(n * 40 / ms / 1e6, 1),
                         "matches_torch": bool(torch.equal(stored_keys(w, n, dev), want))}
            del vals, want
        ms = median_of(lambda: w.rekey_index(0, 1), rounds)
        res["index"] = {"ms": round(ms, 4), "GBps": round(n * 32 / ms / 1e6, 1)}
        ms = median_of(lambda: w.load_columns(0, col, None), rounds)
        res["load_columns"] = {"ms": round(ms, 4), "GBps": round(n * 24 / ms / 1e6, 1)}
    return res


def torch_sort_by(a, b):
    _, i = torch.sort(b, stable=True)
    _, j = torch.sort(a[i], stable=True)
    return i[j]


def part_sort_by(args, dev, gen):
    rounds = max(7, args.rounds)
    res = {"tool": "sort_by_rate", "part": "sort_by", "library": args.label, "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "sets": {}}
    for log2n in args.log2rows:
        n = 1 << log2n
        for prim in ("int64", "int32"):
            if prim == "int64":
                a = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev, generator=gen)
            else:  # few enough values that the second column decides most pairs
                a = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int32, device=dev, generator=gen)
            b = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev, generator=gen)
            out = torch.empty(n, dtype=torch.int64, device=dev)
            got = L.sort_by([a, b])
            same = bool(torch.equal(got, torch_sort_by(a, b)))
            del got
            t = {"sort_by": [], "kept_world": [], "torch": []}
            with L.World(n, ranks=1) as w:
                def step(fn):  # lsb_sort returns before its kernels have finished
                    return timed(lambda: (fn(), w.sync()))

                def recipe():
                    return {"load": step(lambda: w.load_columns(0, b, None)), "sort_last": step(w.my_sort),
                            "rekey": step(lambda: w.rekey(0, a)), "sort_primary": step(w.my_sort),
                            "store": step(lambda: w.store_columns(0, None, out))}
                recipe()
                same = same and bool(torch.equal(out, torch_sort_by(a, b)))
                for _ in range(rounds):
                    t["sort_by"].append(timed(lambda: L.sort_by([a, b])))
                    steps = recipe()
                    t["kept_world"].append(sum(steps.values()))
                    t["torch"].append(timed(lambda: torch_sort_by(a, b)))
                steps["passes_primary"] = w.last_sort()[0]
            md = {k: statistics.median(v) for k, v in t.items()}
            res["sets"]["%s,int64 2^%d" % (prim, log2n)] = {
                "matches_torch": same, "sort_by_ms": round(md["sort_by"], 3),
                "kept_world_ms": round(md["kept_world"], 3), "torch_ms": round(md["torch"], 3),
                "torch_over_sort_by": round(md["torch"] / md["sort_by"], 4),
                "torch_over_kept_world": round(md["torch"] / md["kept_world"], 4),
                "last_round_steps_ms": {k: round(v, 3) if isinstance(v, float) else v for k, v in steps.items()}}
            del a, b, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "sort_by"), required=True)
    ap.add_argument("--log2n", type=int, default=28, help="kernel: records and column elements")
    ap.add_argument("--log2rows", type=int, nargs="+", default=[26, 28], help="sort_by: rows")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="tree", help="names the library build in the output")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sort_by_rate: no GPU")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    res = part_kernel(args, dev, gen) if args.part == "kernel" else part_sort_by(args, dev, gen)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
