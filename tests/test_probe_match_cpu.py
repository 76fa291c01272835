"""CPU: the match probe's contract as restated in probe_match_ref.py against the reference's
semi / anti KATs (worked by hand), and the C ABI's argument checks and its behaviour
without a GPU."""
import ctypes

import numpy as np
import pytest

import probe_match_ref as ref


def test_ref_null_keys_never_match():
    """[1, 2, NULL] joined with [NULL, 2, 3] (src/lib.rs:149-193): one pair, (build 1, probe 1)."""
    ob, op = ref.inner_pairs([1, 2, None], [None, 2, 3])
    assert ob.tolist() == [1] and op.tolist() == [1]
    e = ref.expected(ob, op, 3, 3)
    assert e["bitmap"].tolist() == [0b010, 0, 0, 0, 0, 0, 0, 0]
    assert e["counts"].tolist() == [0, 1, 0]
    assert e["flags"].tolist() == [0, 1, 0]
    assert (e["matched"], e["pairs"]) == (1, 1)
    assert ref.select_rows(e["bitmap"], 3, 1).tolist() == [1]
    assert ref.select_rows(e["bitmap"], 3, 0).tolist() == [0, 2]  # the null row stays in the anti join


def test_ref_left_semi_kat():
    """src/lib.rs:324-371: left [1, 2, NULL], right [1, 1, NULL] -> the left row 1 only."""
    ob, op = ref.inner_pairs([1, 2, None], [1, 1, None])
    e = ref.expected(ob, op, 3, 3)
    assert e["flags"].tolist() == [1, 0, 0]       # LeftSemi emits the flagged build rows
    assert e["counts"].tolist() == [1, 1, 0]
    assert (e["matched"], e["pairs"]) == (2, 2)
    assert e["bitmap"][0] == 0b011


def test_ref_right_anti_kat():
    """src/lib.rs:512-575: left [1, 2, NULL], right [1, 2, 3, NULL] -> right rows 3 and NULL."""
    ob, op = ref.inner_pairs([1, 2, None], [1, 2, 3, None])
    e = ref.expected(ob, op, 4, 3)
    assert ref.select_rows(e["bitmap"], 4, 0).tolist() == [2, 3]
    assert ref.select_rows(e["bitmap"], 4, 1, base=10).tolist() == [10, 11]
    assert e["flags"].tolist() == [1, 1, 0]


def test_ref_flags_accumulate_and_cut_off():
    """Flags are OR'ed into arbitrary prior contents; ids >= nflags are skipped."""
    ob, op = ref.inner_pairs([5, 5, 7, 9], [5, 9, 9])
    assert ob.tolist() == [1, 0, 3, 3] and op.tolist() == [0, 0, 1, 2]
    assert ref.expected_flags(ob, 4, before=[0, 0, 1, 0]).tolist() == [1, 1, 1, 1]
    assert ref.expected_flags(ob, 3).tolist() == [1, 1, 0]
    assert ref.expected_counts(op, 3).tolist() == [2, 1, 1]


def test_ref_select_bit_offset_and_tail():
    rng = np.random.default_rng(3)
    bits = rng.random(200) < 0.5
    bm = np.packbits(bits, bitorder="little")
    for off, n in [(0, 200), (5, 130), (64, 65), (69, 64), (199, 1), (7, 0)]:
        for want in (0, 1):
            assert np.array_equal(ref.select_rows(bm, n, want, 3, off),
                                  np.flatnonzero(bits[off:off + n] == bool(want)) + 3)


def test_null_and_bad_arguments(dfp):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    INV = _lib.HJ_ERR_INVALID
    x = np.zeros(16, np.int64)
    p = x.ctypes.data
    # a null table, as every probe
    assert L.hj_probe_match(None, p, None, 0, 8, p, None, None, 0, p, p, None) == INV
    assert b"null table" in L.hj_last_error()
    assert L.hj_probe_match_workspace_bytes(None, 8) == -1
    # hj_select_bitmap: arguments are checked before the device
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p, None, p, None) == INV       # null d_count
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p, p, None, None) == INV       # null workspace
    assert L.hj_select_bitmap(None, 0, 8, 1, 0, p, p, p, None) == INV       # null bitmap, n > 0
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, None, p, p, None) == INV       # null out_rows, n > 0
    assert L.hj_select_bitmap(p, 0, 8, 2, 0, p, p, p, None) == INV          # want is 0 or 1
    assert L.hj_select_bitmap(p, -1, 8, 1, 0, p, p, p, None) == INV         # negative bit offset
    assert L.hj_select_bitmap(p, 0, -1, 1, 0, p, p, p, None) == INV
    assert L.hj_select_bitmap(p, 0, 8, 1, 2**32 - 7, p, p, p, None) == INV  # base + n > 2^32
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p, p, p + 4, None) == INV      # misaligned workspace
    assert b"aligned" in L.hj_last_error()
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p, p + 4, p, None) == INV      # misaligned d_count
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p + 2, p, p, None) == INV      # misaligned out_rows


def test_select_bitmap_workspace_bytes(dfp):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    prev = 0
    for n in [-5, 0, 1, 63, 64, 65, 4096, 16384, 16385, 10**6, 10**8, 2**32 - 1]:
        b = L.hj_select_bitmap_workspace_bytes(n)
        assert b > 0 and b % 8 == 0 and b >= prev, (n, b, prev)
        prev = b


def test_without_a_gpu(dfp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    x = np.zeros(16, np.int64)
    p = x.ctypes.data
    assert L.hj_select_bitmap(p, 0, 8, 1, 0, p, p, p, None) == _lib.HJ_ERR_NO_DEVICE
    assert L.hj_select_bitmap(None, 0, 0, 1, 0, None, p, p, None) == _lib.HJ_ERR_NO_DEVICE
    # a table cannot exist without a GPU: hj_probe_match is reachable only with a null one
    h = ctypes.c_void_p()
    assert L.hj_build_begin(0, 1, _lib.HJ_INT64, 0, ctypes.byref(h)) == _lib.HJ_ERR_NO_DEVICE
    assert L.hj_probe_match(h, p, None, 0, 8, p, None, None, 0, p, p, None) == _lib.HJ_ERR_INVALID
