"""The hybrid local sort (LSB_OPT_HYBRID) at its kernels' limits, against the
CPU model (tests/hybrid_model.py) on the same inputs: crossing runs on both
sides of k_segfix's CAP in both of its forms, records to re-place at the cap,
segments of 63...129 records inside a tile and split by a tile boundary,
k_segsort's tail and owned range, and the stress tool's thinned and crowded
keys.  tests/test_hybrid_model.py asserts on the host what each input is.

Every input runs in modes 1 and 2 on one rank: the output must be the stable
sort bit for bit (the reference's output, mpi/mpi_lsbsort.cpp:722-737), and
the passes the sort ran (lsb_get_last_sort) and their shifts
(lsb_get_pass_stats; 64 is a k_segsort pass) must be exactly the model's, so
an input that falls on the other side of a limit than the model says fails
even though every route ends in the same order.  Mode 0 (the LSD passes)
runs once per input as the control.
"""
import numpy as np
import pytest

import hybrid_model as hm

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in hm.cases() + hm.thinned_cases()]


def _sort(lsbsort, a, mode):
    with lsbsort.World(a.size, ranks=1) as w:
        w.set_option(lsbsort.OPT_HYBRID, mode)
        w.set_timing(True)
        w.copy_in(0, a)
        w.my_sort()
        w.sync()
        return w.copy_out(0), w.last_sort(), w.pass_stats()


@pytest.fixture(scope="module")
def inputs():
    return {c.name: c for c in hm.cases() + hm.thinned_cases()}


@pytest.mark.parametrize("name", NAMES)
def test_route_passes_and_output(lsb_built, oracle_mod, inputs, name):
    a = inputs[name].a
    want = oracle_mod.stable_sort(a)
    for mode in (1, 2):
        pred = hm.predicted(name)[mode]
        out, (lp, ex, _), rows = _sort(lsb_built, a, mode)
        shifts = [r["shift"] for r in rows]
        print("%s mode %d: model %s %d %s, library %d %s" % (name, mode, pred.route, pred.passes, pred.shifts, lp,
                                                            shifts))
        assert np.array_equal(out, want), (mode, pred.route)
        assert ex == 0
        assert lp == pred.passes, (mode, pred.route, lp, pred.passes)
        assert shifts == pred.shifts, (mode, pred.route)
        assert all(r["elems"] == a.size for r in rows)
    out, (lp, ex, _), rows = _sort(lsb_built, a, 0)
    assert np.array_equal(out, want)
    digits = hm.predicted(name)[1].plan.digits
    assert (lp, ex) == (len(digits), 0) and [r["shift"] for r in rows] == [8 * b for b in digits]


def test_whole_key_local_sorts_of_crossing_runs(lsb_built, oracle_mod, inputs):
    """P = 2, radix_bits = 64, hybrid 1: each rank's local sort of the
    whole-key exchange takes a crossing-run input as its block (one merged by
    k_segfix, one whose run is over CAP)."""
    blocks = [inputs["cross256_64_64"].a, inputs["cross256_257_1"].a]
    assert blocks[0].size == blocks[1].size
    a = np.concatenate(blocks)
    a["val"] = np.arange(a.size, dtype=np.uint64)
    per = blocks[0].size
    with lsb_built.World(a.size, ranks=2, radix_bits=64) as w:
        w.set_option(lsb_built.OPT_HYBRID, 1)
        for r in range(2):
            w.copy_in(r, a[r * per:(r + 1) * per])
        w.my_sort()
        w.sync()
        out = w.gather_global()
    assert np.array_equal(out, oracle_mod.stable_sort(a))
