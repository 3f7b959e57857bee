"""Ordering by several columns (include/lsb.h "ordering by several columns",
DESIGN.md §7.9), the parts that need no GPU: the recipe sort_by runs, as a
numpy model, against numpy.lexsort over the mapped keys; and what the four
front ends refuse before they create a World.
"""
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"u64": (0, np.uint64), "i64": (1, np.int64), "f64": (2, np.float64),
        "u32": (3, np.uint32), "i32": (4, np.int32), "f32": (5, np.float32)}


def bits_of(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def encode(a, kt, descending):
    """lsb_key_encode over a typed numpy column, vectorised."""
    width = 32 if kt >= 3 else 64
    mask = np.uint64((1 << width) - 1)
    sign = np.uint64(1 << (width - 1))
    k = bits_of(a) & mask
    if kt in (1, 4):
        k = k ^ sign
    elif kt in (2, 5):
        k = np.where((k & sign) != 0, ~k & mask, k ^ sign)
    if descending:
        k = ~k & mask
    return k


def column(name, n, seed, distinct=None):
    """A column of one key type with few distinct values (ties on every
    column), floats with NaNs of both signs, both zeros and both infinities."""
    kt, dt = KEYS[name]
    rng = np.random.default_rng(seed)
    if np.issubdtype(dt, np.floating):
        pool = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3.25e10, -7e-20], dtype=dt)
        neg_nan = np.array([np.nan], dtype=dt)
        ib = neg_nan.view(np.uint32 if dt == np.float32 else np.uint64)
        ib |= ib.dtype.type(1 << (8 * dt().itemsize - 1))
        pool = np.concatenate([pool, neg_nan])
    else:
        info = np.iinfo(dt)
        pool = np.array([info.min, info.max, 0, 1, 7, info.max // 3, info.min // 2 + 5], dtype=dt)
    if distinct:
        pool = pool[:distinct]
    return pool[rng.integers(0, pool.size, n)], kt


def recipe(encoded):
    """sort_by's steps on the host: the last column sorted stably with index
    values, then for each earlier column, last to first: gather its keys by
    the values (the rekey) and sort stably again."""
    idx = np.argsort(encoded[-1], kind="stable")
    for col in encoded[-2::-1]:
        idx = idx[np.argsort(col[idx], kind="stable")]
    return idx


def test_encode_matches_the_library(lsb_built):
    L = lsb_built
    for name, (kt, _) in KEYS.items():
        col, _ = column(name, 64, 7)
        for desc in (False, True):
            want = [L.key_encode(int(b), kt, desc) for b in bits_of(col)]
            assert encode(col, kt, desc).tolist() == want, (name, desc)


@pytest.mark.parametrize("names", [("i64",), ("f32",), ("i32", "f64"), ("f32", "u64"), ("u32", "i32", "f64"),
                                   ("i64", "f32", "u32")], ids="-".join)
def test_recipe_is_lexsort(names):
    """1 to 3 columns, every combination of per-column descending."""
    n = 777
    cols = [column(nm, n, 11 + i) for i, nm in enumerate(names)]
    for desc in itertools.product((False, True), repeat=len(names)):
        enc = [encode(c, kt, d) for (c, kt), d in zip(cols, desc)]
        want = np.lexsort(enc[::-1])  # numpy: the last key is the primary
        assert np.array_equal(recipe(enc), want), (names, desc)


def test_recipe_constant_primary():
    """A primary column with all keys equal: the order is the other columns'."""
    n = 500
    prim, kt0 = column("i32", n, 3, distinct=1)
    assert np.unique(prim).size == 1
    sec, kt1 = column("f64", n, 4)
    for d0, d1 in itertools.product((False, True), repeat=2):
        enc = [encode(prim, kt0, d0), encode(sec, kt1, d1)]
        got = recipe(enc)
        assert np.array_equal(got, np.lexsort(enc[::-1]))
        assert np.array_equal(got, np.argsort(enc[1], kind="stable"))


def test_recipe_all_rows_equal_keeps_input_order():
    enc = [np.zeros(100, dtype=np.uint64), np.full(100, 5, dtype=np.uint64)]
    assert np.array_equal(recipe(enc), np.arange(100))


# ------------------------------------------------------------------ refusals
def test_sort_by_refusals(lsb_built):
    import torch
    L = lsb_built
    a = torch.arange(5, dtype=torch.int64)
    for what, args in [("no columns", ([],)),
                       ("a tensor, not a sequence", (a,)),
                       ("not tensors", ([[1, 2, 3]],)),
                       ("unequal lengths", ([a, a[:4]],)),
                       ("2-D column", ([a.reshape(5, 1)],)),
                       ("flags for another number of columns", ([a, a], [True])),
                       ("CPU tensors", ([a, a],))]:
        with pytest.raises(ValueError):
            L.sort_by(*args)
            pytest.fail(what)


def test_sort_rows_refusals(lsb_built):
    import torch
    L = lsb_built
    a = torch.arange(12, dtype=torch.int64)
    for what, x in [("1-D", a), ("3-D", a.reshape(2, 3, 2)), ("CPU", a.reshape(3, 4)), ("not a tensor", [[1, 2]])]:
        with pytest.raises(ValueError):
            L.sort_rows(x)
            pytest.fail(what)
    with pytest.raises(ValueError):
        L.sort(a.reshape(3, 4))  # sort() keeps refusing 2-D input


def test_segment_sort_refusals(lsb_built):
    import torch
    L = lsb_built
    a = torch.arange(6, dtype=torch.int64)
    off = torch.tensor([0, 3, 6], dtype=torch.int64)
    for what, args, match in [("CPU keys", (a, off), "GPU"),
                              ("keys not a tensor", ([1, 2], off), "keys"),
                              ("offsets not a tensor", (a, [0, 6]), "offsets"),
                              ("offsets not int64", (a, off.to(torch.int32)), "offsets"),
                              ("offsets 2-D", (a, off.reshape(1, 3)), "offsets"),
                              ("no offsets", (a, off[:0]), "offsets"),
                              ("not from 0", (a, torch.tensor([1, 3, 6])), "offsets"),
                              ("not to n", (a, torch.tensor([0, 3, 5])), "offsets"),
                              ("beyond n", (a, torch.tensor([0, 3, 7])), "offsets"),
                              ("decreasing", (a, torch.tensor([0, 4, 3, 6])), "offsets: decreasing")]:
        with pytest.raises(ValueError, match=match):
            L.segment_sort(*args)
            pytest.fail(what)


def test_group_quantile_refusals(lsb_built):
    import torch
    L = lsb_built
    a = torch.arange(6, dtype=torch.int64)
    for what, args in [("unequal lengths", (a, a[:5])), ("CPU tensors", (a, a)),
                       ("values not a tensor", (a, [1.0] * 6))]:
        with pytest.raises(ValueError):
            L.group_quantile(*args)
            pytest.fail(what)
    for q in (-0.01, 1.01, float("nan"), float("inf"), "0.5", None):
        with pytest.raises(ValueError, match="q"):
            L.group_quantile(a, a, q=q)
            pytest.fail(repr(q))
