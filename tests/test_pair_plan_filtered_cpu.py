"""CPU: the filtered pair plan's C ABI (hj_pair_plan_filtered_bytes, hj_pair_plan_filtered,
hj_pair_window_filtered) is declared, exported and bound; its argument checks answer before
any device call, so they hold without a GPU too; the operator accepts filtered_probe=."""
import numpy as np

from test_pair_filter_cpu import _Pred  # a predicate over host memory where there is no GPU

NAMES = {"hj_pair_plan_filtered_bytes", "hj_pair_plan_filtered", "hj_pair_window_filtered"}


def test_abi_has_the_three_symbols(dfp):
    import test_abi
    from datafusion_parallelism_amd import _lib

    assert NAMES <= set(test_abi.declared_functions())
    assert NAMES <= {n for n, _, _ in _lib.SIGNATURES}
    test_abi.test_library_exports_every_declared_symbol(dfp)
    import datafusion_parallelism_amd as pkg

    assert "FilteredPairPlan" in pkg.__all__ and issubclass(pkg.FilteredPairPlan, pkg.PairPlan)


def _calls(L, p):
    def plan(pred, t=None, keys=p, n=8, plan=p, bm=None, flags=None, nflags=0, st=None):
        return L.hj_pair_plan_filtered(t, keys, None, 0, n, pred, plan, bm, flags, nflags, st, None)

    def window(pred, t=None, plan=p, n=8, ids=None, base=0, lo=0, cap=4, ob=p, op=p, dw=p):
        return L.hj_pair_window_filtered(t, plan, n, pred, ids, base, lo, cap, ob, op, dw, None)

    return plan, window


def test_invalid_predicate_comes_first_and_names_the_term(dfp):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    INV = _lib.HJ_ERR_INVALID
    EQ, INT, B, P = _lib.HJ_CMP_EQ, _lib.HJ_VAL_INT, _lib.HJ_SIDE_BUILD, _lib.HJ_SIDE_PROBE
    p = np.zeros(64, np.int64).ctypes.data
    plan, window = _calls(L, p)
    bad_op = _Pred(_lib, [(EQ, INT, B, 0, P, 0, 0), (6, INT, B, 0, P, 0, 0)])
    bad_col = _Pred(_lib, [(EQ, INT, B, 0, P, 5, 0)])
    for call in (plan, window):
        assert call(bad_op.s) == INV
        assert b"term 1" in L.hj_last_error() and b"bad op" in L.hj_last_error()
        assert call(bad_col.s) == INV
        assert b"term 0" in L.hj_last_error() and b"column index" in L.hj_last_error()
        assert call(None) == INV
        assert b"predicate" in L.hj_last_error()
    # the predicate is judged before everything else that is wrong with the call
    assert plan(bad_op.s, plan=p + 4, n=-1) == INV and b"term 1" in L.hj_last_error()
    assert window(bad_op.s, op=p + 2, lo=-1) == INV and b"term 1" in L.hj_last_error()


def test_null_table_and_bad_arguments(dfp):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    INV = _lib.HJ_ERR_INVALID
    p = np.zeros(64, np.int64).ctypes.data
    plan, window = _calls(L, p)
    ok = _Pred(_lib, [(_lib.HJ_CMP_LT, _lib.HJ_VAL_INT, _lib.HJ_SIDE_BUILD, 0, _lib.HJ_SIDE_PROBE, 0, 0)],
               build_rows=8, probe_rows=8)
    # a valid predicate on a null table: what hj_probe_match_filtered answers there
    want = L.hj_probe_match_filtered(None, p, None, 0, 8, ok.s, p, None, None, 0, p, None)
    assert want == INV and b"null table" in L.hj_last_error()
    assert plan(ok.s) == want and b"null table" in L.hj_last_error()
    assert window(ok.s) == want and b"null table" in L.hj_last_error()
    assert L.hj_pair_plan_filtered_bytes(None, 10) == -1
    assert L.hj_pair_plan_filtered_bytes(None, 0) == -1
    # The table's errors come before the pointer and range checks, so with a null table every
    # line below is answered by the "null table" check: they only show that a bad argument is
    # HJ_ERR_INVALID without any device call, not which check refused it. The checks
    # themselves are exercised against a built table, message by message, in
    # tests/test_gpu_pair_plan_filtered.py::test_argument_checks_on_a_built_table.
    assert plan(ok.s, plan=p + 4) == INV
    assert plan(ok.s, plan=None) == INV
    assert plan(ok.s, bm=p + 4) == INV and plan(ok.s, st=p + 4) == INV
    assert window(ok.s, op=p + 2) == INV
    assert window(ok.s, plan=p + 4) == INV and window(ok.s, ob=p + 4) == INV and window(ok.s, dw=p + 4) == INV
    assert window(ok.s, ids=p, base=5) == INV
    assert window(ok.s, lo=-1) == INV and window(ok.s, cap=-1) == INV and window(ok.s, cap=2**42 + 1) == INV
    assert plan(ok.s, n=2**32) == INV and window(ok.s, n=-1) == INV


def test_operator_accepts_filtered_probe():
    """The flag is a constructor keyword of both classes, off by default; no device is touched."""
    import inspect

    from datafusion_parallelism_amd.operator import BuildImplementation, JoinReplacement, ParallelHashJoin

    for cls in (BuildImplementation, ParallelHashJoin):
        assert inspect.signature(cls.__init__).parameters["filtered_probe"].default is False
    assert BuildImplementation(JoinReplacement.Gpu, 1)._shared.filtered_probe is False
    assert BuildImplementation(JoinReplacement.Gpu, 1, filtered_probe=True)._shared.filtered_probe is True
    j = ParallelHashJoin([[]], [[]], on=[("a", "a")], filtered_probe=True)
    assert j._build._shared.filtered_probe is True
    assert ParallelHashJoin([[]], [[]], on=[("a", "a")])._build._shared.filtered_probe is False
