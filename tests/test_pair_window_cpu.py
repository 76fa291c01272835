"""CPU: the pair window's contract as restated in pair_window_ref.py against the reference's
null-key KAT and a duplicate-key case worked by hand, and the C ABI's argument checks and its
behaviour without a GPU."""
import ctypes

import numpy as np
import pytest

import pair_window_ref as ref
from probe_match_ref import inner_pairs


def test_ref_null_keys_kat():
    """[1, 2, NULL] joined with [NULL, 2, 3] (src/lib.rs:149-193): one pair, (build 1, probe 1)."""
    ob, op = inner_pairs([1, 2, None], [None, 2, 3])
    assert ob.tolist() == [1] and op.tolist() == [1]
    b, p, w = ref.window(ob, op, 0, 10)
    assert (b.tolist(), p.tolist(), w) == ([1], [1], 1)
    assert ref.window(ob, op, 0, 0)[2] == 0
    assert ref.window(ob, op, 1, 5)[2] == 0 and ref.window(ob, op, 4, 5)[2] == 0
    b, p, w = ref.window(ob, op, 0, 1, probe_base=40)
    assert (b.tolist(), p.tolist(), w) == ([1], [41], 1)
    b, p, w = ref.window(ob, op, 0, 1, probe_ids=np.array([7, 8, 9], np.int32))
    assert p.tolist() == [8]


def test_ref_duplicate_keys_by_hand():
    """build [5, 5, 7, 9, 5], probe [5, 9, 8, 5]: probe rows ascending, each row's build rows
    descending. S = (4,0) (1,0) (0,0) (3,1) (4,3) (1,3) (0,3)."""
    ob, op = inner_pairs([5, 5, 7, 9, 5], [5, 9, 8, 5])
    assert ob.tolist() == [4, 1, 0, 3, 4, 1, 0] and op.tolist() == [0, 0, 0, 1, 3, 3, 3]
    b, p, w = ref.window(ob, op, 2, 3)  # starts inside row 0's key, ends inside row 3's
    assert (b.tolist(), p.tolist(), w) == ([0, 3, 4], [0, 1, 3], 3)
    b, p, w = ref.window(ob, op, 5, 100)
    assert (b.tolist(), p.tolist(), w) == ([1, 0], [3, 3], 2)
    # a cover by windows of 3 gives S back
    got_b, got_p = [], []
    for lo, cap in ref.cover(len(ob), 3):
        b, p, w = ref.window(ob, op, lo, cap)
        assert w == min(3, len(ob) - lo)
        got_b += b.tolist()
        got_p += p.tolist()
    assert got_b == ob.tolist() and got_p == op.tolist()
    assert ref.cover(0, 3) == [] and ref.cover(7, 7) == [(0, 7)]
    assert ref.window(ob, op, 0, 2, probe_base=2**32 - 4)[1].tolist() == [2**32 - 4, 2**32 - 4]


def test_null_and_bad_arguments(dfp):
    """The argument checks come before any device call, so they answer the same with and
    without a GPU, whatever the table."""
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    INV = _lib.HJ_ERR_INVALID
    x = np.zeros(64, np.int64)
    p = x.ctypes.data
    assert L.hj_pair_plan_bytes(None, 8) == -1
    assert L.hj_pair_plan_bytes(None, 0) == -1
    # hj_pair_plan
    assert L.hj_pair_plan(None, p, None, 0, 8, None, p, None) == INV           # null plan
    assert b"plan" in L.hj_last_error()
    assert L.hj_pair_plan(None, p, None, 0, 8, p + 4, p, None) == INV          # misaligned plan
    assert b"aligned" in L.hj_last_error()
    assert L.hj_pair_plan(None, p, None, 0, 8, p, p + 4, None) == INV          # misaligned d_total
    assert L.hj_pair_plan(None, p, None, 0, -1, p, p, None) == INV             # negative n
    assert L.hj_pair_plan(None, p, None, 0, 2**32, p, p, None) == INV          # n outside [0, 2^32)
    assert L.hj_pair_plan(None, None, None, 0, 8, p, p, None) == INV           # null keys, n > 0
    # hj_pair_window
    ok = dict(plan=p, n=8, ids=None, base=0, lo=0, cap=4, ob=p, op=p, dw=p)

    def window(**kw):
        a = {**ok, **kw}
        return L.hj_pair_window(None, a["plan"], a["n"], a["ids"], a["base"], a["lo"], a["cap"], a["ob"], a["op"],
                                a["dw"], None)

    assert window(plan=None) == INV
    assert window(plan=p + 4) == INV
    assert window(dw=p + 4) == INV
    assert window(ob=p + 4) == INV
    assert window(op=p + 2) == INV
    assert b"aligned" in L.hj_last_error()
    assert window(ob=None) == INV and window(op=None) == INV                   # null output, capacity > 0
    assert window(lo=-1) == INV
    assert window(cap=-1) == INV
    assert window(n=-1) == INV and window(n=2**32) == INV
    assert window(ids=p, base=5) == INV                                        # ids and a base together
    assert b"exclusive" in L.hj_last_error()
    assert window(base=2**32 - 4) == INV                                       # base + n > 2^32
    # with good arguments the null table is what is wrong (or, without a GPU, the missing GPU)
    import torch

    want = INV if torch.cuda.is_available() else _lib.HJ_ERR_NO_DEVICE
    assert window() == want
    assert window(cap=0, ob=None, op=None, dw=None) == want                    # all optional at capacity 0
    assert L.hj_pair_plan(None, p, None, 0, 8, p, None, None) == want          # d_total is optional
    if torch.cuda.is_available():
        assert b"null table" in L.hj_last_error()


def test_without_a_gpu(dfp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    x = np.zeros(64, np.int64)
    p = x.ctypes.data
    ND = _lib.HJ_ERR_NO_DEVICE
    assert L.hj_pair_plan(None, p, None, 0, 8, p, p, None) == ND
    assert L.hj_pair_plan(None, None, None, 0, 0, p, p, None) == ND
    assert L.hj_pair_window(None, p, 8, None, 0, 0, 4, p, p, p, None) == ND
    assert b"no GPU" in L.hj_last_error()
    # a table cannot exist without a GPU
    h = ctypes.c_void_p()
    assert L.hj_build_begin(0, 1, _lib.HJ_INT64, 0, ctypes.byref(h)) == ND
    assert L.hj_pair_plan_bytes(h, 8) == -1


def test_abi_has_the_three_symbols(dfp):
    """tests/test_abi.py's declared <= exported <= bound, for the new entry points by name."""
    import test_abi
    from datafusion_parallelism_amd import _lib

    names = {"hj_pair_plan_bytes", "hj_pair_plan", "hj_pair_window"}
    assert names <= set(test_abi.declared_functions())
    assert names <= {n for n, _, _ in _lib.SIGNATURES}
    test_abi.test_library_exports_every_declared_symbol(dfp)


def test_operator_rejects_bad_limits():
    """max_output_rows is checked at construction, before any device is touched."""
    from datafusion_parallelism_amd import HjError, _lib
    from datafusion_parallelism_amd.operator import BuildImplementation, JoinReplacement

    for bad in (0, -3, 2.5, True):
        with pytest.raises(HjError) as e:
            BuildImplementation(JoinReplacement.Gpu, 1, max_output_rows=bad)
        assert e.value.status == _lib.HJ_ERR_INVALID
    with pytest.raises(HjError) as e:
        BuildImplementation(JoinReplacement.Gpu, 1, devices=[0], max_output_rows=10)
    assert e.value.status == _lib.HJ_ERR_INVALID and "multi-GPU" in str(e.value)
