#!/usr/bin/env python3
"""Rates of lsb_label_runs and of the whole inverse index
against a device copy of the same bytes, torch.unique(return_inverse=True)
and a torch scatter of the same ids.

One process, one GPU, n = 2^28 records by default.  Inputs: u64 keys, the
three of tools/runs_rate.py in a random order (one permutation for all)
  distinct   every key once (n runs)
  d65536     2^16 distinct values (runs of n / 2^16)
  one        one value (one run)
loaded with index values.  Every round times, with torch CUDA events around
the blocking calls,
  front     what unique() does before the inverse: lsb_load_columns, the first
            lsb_sort, lsb_count_runs, lsb_store_runs with all four outputs
  label     lsb_label_runs(LSB_LABEL_BY_VALUE): k_run_label, the error word's
            trip to the host and the swap; beside it a torch.Tensor.copy_ of
            its algorithmic bytes (16 n read, 16 n written)
  sort2     the second lsb_sort, by the index
  store     lsb_store_columns of the values: the inverse column
  unique    (a) torch.unique(return_inverse=True) on the key column
  scatter   (b) inv[idx] = ids by torch, idx and ids the two columns of the
            labelled records: at one rank the single-pass alternative to
            sort2 + store
The rounds interleave the inputs and the yardsticks; after one warm-up round
the median of at least 5 is taken.  Prints one JSON line: per input the
medians in ms, label_ratio = copy time / label time (1.0: parity with the
copy), yardstick time / (label + sort2 + store) for (a) and (b), and (a)
over front + label + sort2 + store, the whole of unique(return_inverse=True)
inside one World, which is the work torch.unique does.

--label-only times label and its copy alone (no yardsticks, no second sort):
for comparing builds of k_run_label (LSB_LIBRARY).

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
    ap.add_argument("--label-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    n = 1 << args.log2n
    rounds = max(5, args.rounds)
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    perm = torch.randperm(n, dtype=torch.int64, device=dev)
    inputs = {"distinct": perm, "d65536": perm >> max(args.log2n - 16, 0), "one": torch.zeros_like(perm)}
    runs_of = {"distinct": n, "d65536": min(n, 1 << 16), "one": 1}
    src = torch.empty(16 * n, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    inverse = torch.empty(n, dtype=torch.int64, device=dev)
    idx, ids, inv_b = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    names = ("label", "copy_label") if args.label_only else ("front", "label", "copy_label", "sort2", "store", "unique", "scatter")
    times = {name: {k: [] for k in names} for name in inputs}
    checked, passes = {}, {}
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, keys in inputs.items():
                m, t, plan = runs_of[name], {}, {}

                def front():
                    w.load_columns(0, keys, None, key_type=L.KEY_U64)
                    w.my_sort()
                    plan.update(w.count_runs())
                    if not args.label_only:
                        w.store_runs(0, *[o[:m] for o in outs], key_type=L.KEY_U64)

                t["front"] = timed(front)
                t["label"] = timed(lambda: w.label_runs(L.LABEL_BY_VALUE))
                t["copy_label"] = timed(lambda: dst.copy_(src))
                if not args.label_only:
                    w.store_columns(0, idx, ids, key_type=L.KEY_U64)  # the labelled records' columns, for (b)
                    t["sort2"] = timed(lambda: (w.my_sort(), w.sync()))
                    passes[name] = w.last_sort()[0]
                    t["store"] = timed(lambda: w.store_columns(0, None, inverse))
                    tu = []
                    t["unique"] = timed(lambda: tu.extend(torch.unique(keys, return_inverse=True)))
                    t["scatter"] = timed(lambda: inv_b.scatter_(0, idx, ids))
                    if rnd == 0:  # the library's answer is torch's, and so is the scatter's
                        checked[name] = bool(plan["total"] == runs_of[name] == tu[0].numel() and
                                             torch.equal(inverse, tu[1]) and torch.equal(inv_b, tu[1]))
                    del tu
                if rnd > 0:
                    for k in names:
                        times[name][k].append(t[k])
    res = {"tool": "labels_rate", "n": n, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(L.LIB_PATH, ROOT), "inputs": {}}
    for name in inputs:
        md = {k: statistics.median(v) for k, v in times[name].items()}
        row = {"runs": runs_of[name], "label_ms": round(md["label"], 4), "copy_label_ms": round(md["copy_label"], 4),
               "label_gbs": round(32 * n / md["label"] / 1e6, 1), "label_ratio": round(md["copy_label"] / md["label"], 4)}
        if not args.label_only:
            whole = md["label"] + md["sort2"] + md["store"]
            row.update({
                "matches_torch": checked[name], "sort2_passes": passes[name],
                "sort2_ms": round(md["sort2"], 4), "store_ms": round(md["store"], 4), "inverse_ms": round(whole, 4),
                "front_ms": round(md["front"], 4), "unique_over_front_and_inverse": round(md["unique"] / (md["front"] + whole), 4),
                "torch_unique_ms": round(md["unique"], 4), "torch_scatter_ms": round(md["scatter"], 4),
                "unique_over_inverse": round(md["unique"] / whole, 4),
                "scatter_over_inverse": round(md["scatter"] / whole, 4),
                "scatter_over_sort2_store": round(md["scatter"] / (md["sort2"] + md["store"]), 4),
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
