#!/usr/bin/env python3
"""Rates of lsb_load_columns / lsb_store_columns against a device copy of the
same bytes (DESIGN.md "Caller-owned columns").

One process, one GPU, n = 2^28 records by default.  For each form
  u64_v8       u64 keys, 8-byte values
  u32_v4       u32 keys, 4-byte values
  u64_argsort  u64 keys, no values in, int64 indices out
every round times load_columns, the my_sort() after it and store_columns with
torch CUDA events, and beside each of the two a torch.Tensor.copy_ that moves
as many bytes: n x (bytes read + bytes written per record), half of them read
and half written.  The rounds interleave the forms and the copies; after one
warm-up round the median of at least 5 is taken.  Prints one JSON line:
per form the medians in ms, ratio = copy time / kernel time (1.0: parity with
the copy; the kernels move the same bytes and do nothing else) and share =
(load + store) / (load + sort + store).

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

# form -> (key type, key tensor dtype, value dtype or None, bytes a load moves per record, a store)
FORMS = {
    "u64_v8": (L.KEY_U64, torch.int64, torch.int64, 8 + 8 + 16, 16 + 8 + 8),
    "u32_v4": (L.KEY_U32, torch.int32, torch.int32, 4 + 4 + 16, 16 + 4 + 4),
    "u64_argsort": (L.KEY_U64, torch.int64, None, 8 + 16, 16 + 8 + 8),
}


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
    g = torch.Generator(device=dev).manual_seed(1)
    cols = {}
    for name, (kt, kdt, vdt, _, _) in FORMS.items():
        keys = torch.randint(-2**31, 2**31, (n,), dtype=kdt, device=dev, generator=g)
        if kdt == torch.int64:  # every byte uniform
            keys = (keys << 32) | torch.randint(0, 2**32, (n,), dtype=kdt, device=dev, generator=g)
        vals = None if vdt is None else torch.randint(0, torch.iinfo(vdt).max, (n,), dtype=vdt, device=dev, generator=g)
        out_k = torch.empty_like(keys)
        out_v = torch.empty(n, dtype=torch.int64 if vdt is None else vdt, device=dev)
        cols[name] = (kt, keys, vals, out_k, out_v)
    src = torch.empty(16 * n, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    times = {name: {k: [] for k in ("load", "sort", "store", "copy_load", "copy_store")} for name in FORMS}
    with L.World(n, ranks=1) as w:
        for rnd in range(rounds + 1):  # round 0 warms up
            for name, (kt, keys, vals, out_k, out_v) in cols.items():
                lb, sb = FORMS[name][3] * n // 2, FORMS[name][4] * n // 2
                t = {}
                t["load"] = timed(lambda: w.load_columns(0, keys, vals, key_type=kt))
                t["copy_load"] = timed(lambda: dst[:lb].copy_(src[:lb]))
                t["sort"] = timed(lambda: (w.my_sort(), w.sync()))
                t["store"] = timed(lambda: w.store_columns(0, out_k, out_v, key_type=kt))
                t["copy_store"] = timed(lambda: dst[:sb].copy_(src[:sb]))
                if rnd:
                    for k, v in t.items():
                        times[name][k].append(v)
        sorted_ok = w.check_sorted()
    res = {"tool": "columns_rate", "n": n, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "sorted": bool(sorted_ok), "forms": {}}
    for name in FORMS:
        m = {k: statistics.median(v) for k, v in times[name].items()}
        lb, sb = FORMS[name][3] * n, FORMS[name][4] * n
        res["forms"][name] = {
            "load_ms": round(m["load"], 4), "copy_load_ms": round(m["copy_load"], 4),
            "store_ms": round(m["store"], 4), "copy_store_ms": round(m["copy_store"], 4),
            "sort_ms": round(m["sort"], 4),
            "load_gbs": round(lb / m["load"] / 1e6, 1), "store_gbs": round(sb / m["store"] / 1e6, 1),
            "load_ratio": round(m["copy_load"] / m["load"], 4), "store_ratio": round(m["copy_store"] / m["store"], 4),
            "ratio": round((m["copy_load"] + m["copy_store"]) / (m["load"] + m["store"]), 4),
            "share": round((m["load"] + m["store"]) / (m["load"] + m["sort"] + m["store"]), 4),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
