"""The F64 sums over the runs, bit for bit (lsb_store_reduce, lsb_store_scan
and lsb_scan_runs with SUM over F64).

The integer forms, MIN and MAX are pinned exactly by the models of
tests/test_reduce_gpu.py and tests/test_scan_gpu.py; an F64 sum is pinned
there only to within the rounding of any order of addition.  The library fixes
the order of every addition (no floating-point atomics), so its output bytes
are a function of the input alone: their SHA-256 is recorded in
tests/golden/run_f64_digests.json, and a change of the kernels that
reassociates one addition changes a digest.

Inputs: sorted u64 keys equal to the run index, run lengths cycling through
tests/test_scan_gpu.py's EDGE_CYCLE, values that are finite doubles of both
signs over 121 binades (2^-60 .. 2^60), a hash of the position.  The input
check (no GPU) shows that such an input pins the order: in every one of them
some run's left-to-right sum differs from its exactly rounded sum.

As tests/test_scan_gpu.py, the GPU tests run in one child pytest process over
this same file that imports torch before the library is loaded
(LSB_BITS_CHILD=1); here each test reports what its namesake did there.
"""
import functools
import hashlib
import inspect
import json
import math
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

IN_CHILD = os.environ.get("LSB_BITS_CHILD") == "1"
if IN_CHILD:
    import torch  # noqa: F401  before the library is loaded

from test_reduce_host import splitmix64  # noqa: E402
from test_scan_gpu import EDGE_CYCLE, TILE, cycle, host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_f64_digests.json")
SUM, F64, KEEP = 0, 2, 0
REC = np.dtype([("key", "<u8"), ("val", "<u8")])
SIZES = [65, TILE + 1, 5 * TILE + 17]  # the last: one whole cycle, runs across two tile edges
RANKS = [1, 3]


def wide_values(n):
    """Finite doubles of both signs with full mantissas and exponents in
    -60..60, a hash of the position (tests/test_scan_gpu.py's "wide", over
    121 binades: the first 65 positions already reach past 2^-40 and 2^40)
    -> their bits."""
    h = splitmix64(np.arange(n))
    mant = 1.0 + (h >> np.uint64(12)).astype(np.float64) * 2.0 ** -52
    d = np.ldexp(mant, ((h >> np.uint64(1)) % np.uint64(121)).astype(np.int64) - 60) * \
        np.where(h & np.uint64(1), -1.0, 1.0)
    return d.view(np.uint64).copy()


def inputs(n):
    """-> (run lengths, records): run j's key is j."""
    lengths = cycle(EDGE_CYCLE, n)
    rec = np.zeros(n, dtype=REC)
    rec["key"] = np.repeat(np.arange(lengths.size, dtype=np.uint64), lengths)
    rec["val"] = wide_values(n)
    return lengths, rec


def case_name(n, P):
    return f"n={n},P={P}"


def digests_of(L, n, P):
    """{output: SHA-256 of its bytes} from one count_runs over the input of
    size n on P loopback ranks: the reduction per run, the scan per record,
    and the records of B after scan_runs(KEEP), each in global order."""
    import torch
    lengths, rec = inputs(n)
    m = len(lengths)
    with L.World(n, ranks=P) as w:
        w.scatter_global(rec)
        plan = w.count_runs()
        assert plan["total"] == m
        w.plan_reduce(SUM, F64)
        red = torch.zeros(m, dtype=torch.int64, device="cuda")
        for r in range(P):
            lo, cnt = plan["bases"][r], plan["runs"][r]
            if cnt:
                assert w.store_reduce(r, red[lo:lo + cnt]) == cnt
        w.plan_scan(SUM, F64)
        scan = torch.zeros(n, dtype=torch.int64, device="cuda")
        for r in range(P):
            h = w.here(r)
            if h:
                assert w.store_scan(r, scan[r * w.per: r * w.per + h]) == h
        w.scan_runs(KEEP)
        after = w.gather_global()
    assert np.array_equal(after["key"], rec["key"])
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    return {"store_reduce": sha(host(red)), "store_scan": sha(host(scan)), "scan_runs_keep": sha(after)}


# ------------------------------------------------------------------ no GPU
@pytest.mark.parametrize("n", SIZES)
def test_inputs_pin_the_order(n):
    """The exponents reach 2^-40 and 2^40 or past them, and for at least one run the
    left-to-right sum is not the exactly rounded one (math.fsum): another
    association can give other bits, so equal digests say something."""
    lengths, rec = inputs(n)
    x = rec["val"].view(np.float64)
    assert np.all(np.isfinite(x))
    e = np.frexp(x)[1] - 1
    assert e.min() <= -40 and e.max() >= 40
    assert np.all(np.diff(rec["key"].astype(np.int64)) >= 0) and int(rec["key"][-1]) == len(lengths) - 1
    differ, lo = 0, 0
    for cnt in lengths:
        seg = x[lo:lo + cnt].tolist()
        left = 0.0
        for v in seg:
            left += v
        differ += left != math.fsum(seg)
        lo += int(cnt)
    assert differ >= 1


def test_golden_covers_the_cases():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["parent_commit"]) == 40 and gold["device"]
    assert sorted(gold["digests"]) == sorted(case_name(n, P) for n in SIZES for P in RANKS)
    for row in gold["digests"].values():
        assert sorted(row) == ["scan_runs_keep", "store_reduce", "store_scan"]
        assert all(len(v) == 64 for v in row.values())


# ------------------------------------------------------------------ the GPU
@pytest.fixture(scope="session")
def child_outcomes(tmp_path_factory):
    """{test id: (outcome, text)} of the child pytest process over this file."""
    xml = tmp_path_factory.mktemp("bits") / "child.xml"
    env = dict(os.environ, LSB_BITS_CHILD="1")
    for name in ("LSB_REGION_MIN", "LSB_PACK_VALUES", "LSB_REGION_FIRST", "LSB_SCAN_CHILD", "LSB_LABELS_CHILD"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider",
                        "-m", "gpu", "--junitxml", str(xml)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    out = {}
    if xml.exists():
        for case in ET.parse(str(xml)).getroot().iter("testcase"):
            bad = [(c.tag, (c.get("message") or "") + "\n" + (c.text or "")) for c in case
                   if c.tag in ("failure", "error", "skipped")]
            out[case.get("name")] = bad[0] if bad else ("passed", "")
    out[None] = p.stdout[-4000:] + p.stderr[-2000:]
    return out


def torch_first(fn):
    """The test as it runs in the child process; in the pytest process that
    started it, a test of the same name and parameters that passes exactly
    when the child's did."""
    if IN_CHILD:
        return fn

    @functools.wraps(fn)
    def reported(*args, request, child_outcomes, **kwargs):
        got = child_outcomes.get(request.node.name)
        assert got is not None, "the child process did not run this test:\n" + child_outcomes[None]
        assert got[0] == "passed", got[1]

    sig = inspect.signature(fn)
    extra = [inspect.Parameter(n, inspect.Parameter.KEYWORD_ONLY) for n in ("request", "child_outcomes")]
    reported.__signature__ = sig.replace(parameters=list(sig.parameters.values()) + extra)
    return reported


@pytest.mark.gpu
@pytest.mark.parametrize("P", RANKS)
@pytest.mark.parametrize("n", SIZES)
@torch_first
def test_f64_sum_bits(lsb_built, n, P):
    """Two calls give the same digests, and they are the recorded ones."""
    with open(GOLDEN) as f:
        want = json.load(f)["digests"][case_name(n, P)]
    first = digests_of(lsb_built, n, P)
    assert digests_of(lsb_built, n, P) == first
    assert first == want
