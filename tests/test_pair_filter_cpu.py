"""CPU: the pair filter's numpy restatement (tests/pair_filter_ref.py) against pyarrow, and
the parts of the C ABI that need no GPU: hj_pair_predicate_check, the order of the device
calls' checks, the workspace bound, the Python predicate's type rules."""
import ctypes
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_filter_ref as ref  # noqa: E402

PC = {ref.EQ: pc.equal, ref.NE: pc.not_equal, ref.LT: pc.less, ref.LE: pc.less_equal, ref.GT: pc.greater,
      ref.GE: pc.greater_equal}
OPS = list(PC)


def _against_pyarrow(cls, lv, rv, lvalid=None, rvalid=None):
    """Every pair (i, j) of the two small columns, all six ops."""
    nl, nr = len(lv), len(rv)
    bidx, pidx = np.repeat(np.arange(nl), nr), np.tile(np.arange(nr), nl)
    la = pa.array(lv, mask=None if lvalid is None else ~lvalid)
    ra = pa.array(rv, mask=None if rvalid is None else ~rvalid)
    for op in OPS:
        got = ref.pair_pass([ref.Term(op, cls, (ref.BUILD, 0), (ref.PROBE, 0))], [ref.Col(lv, lvalid)],
                            [ref.Col(rv, rvalid)], nl, nr, bidx, pidx)
        want = PC[op](la.take(pa.array(bidx)), ra.take(pa.array(pidx))).fill_null(False).to_numpy(zero_copy_only=False)
        assert np.array_equal(got, want), (cls, op)


def test_ref_ints_of_mixed_width_against_pyarrow():
    rng = np.random.default_rng(1)
    a = np.array([-128, -1, 0, 1, 127, 5, -7], dtype=np.int8)
    b = np.array([-2**40, -128, -1, 0, 127, 2**40, 5], dtype=np.int64)
    valid = rng.random(len(a)) < 0.7
    _against_pyarrow(ref.INT, a, b, valid, None)
    _against_pyarrow(ref.INT, b, a.astype(np.int16), None, valid)
    _against_pyarrow(ref.INT, np.array([-2**31, 2**31 - 1, 3], np.int32), np.array([-2**31, 3, 2**31], np.int64))


def test_ref_uint64_above_2_63_against_pyarrow():
    a = np.array([0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1], dtype=np.uint64)
    _against_pyarrow(ref.UINT, a, a[::-1].copy())
    _against_pyarrow(ref.UINT, np.array([0, 200, 255], np.uint8), a)
    # a constant above 2^63 travels as its bits
    got = ref.pair_pass([ref.Term(ref.GT, ref.UINT, (ref.BUILD, 0), (ref.CONST, ref.const_bits(ref.UINT, 2**63)))],
                        [ref.Col(a)], [], len(a), 1, np.arange(len(a)), np.zeros(len(a), np.uint32))
    assert got.tolist() == [False, False, False, False, True, True]


def test_ref_floats_against_pyarrow():
    """No NaN, no -0.0: there IEEE and totalOrder agree."""
    a = np.array([-np.inf, -1.5, 0.0, 1e-300, 2.5, np.inf], dtype=np.float64)
    b = np.array([-np.inf, -1.5, 0.0, 0.1, 2.5, 3e38], dtype=np.float32)
    _against_pyarrow(ref.FLOAT, a, b, None, np.array([1, 1, 0, 1, 1, 1], bool))
    _against_pyarrow(ref.FLOAT, b, b[::-1].copy())


def test_ref_float_total_order_by_the_key_formula():
    """pyarrow compares IEEE (nan == nan False, -0.0 < 0.0 False); the contract is the key."""
    nan_pos = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
    nan_neg = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    v = np.array([nan_neg, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, nan_pos])
    k = ref.float_key(v)
    assert np.all(np.diff(k) > 0)  # strictly ascending: -nan < -inf < ... < -0.0 < +0.0 < ... < +inf < +nan
    one = lambda op, x, y: bool(ref.pair_pass([ref.Term(op, ref.FLOAT, (ref.BUILD, 0), (ref.PROBE, 0))],
                                               [ref.Col(np.array([x]))], [ref.Col(np.array([y]))], 1, 1, [0], [0])[0])
    assert one(ref.EQ, nan_pos, nan_pos) and not one(ref.EQ, nan_pos, nan_neg)
    assert one(ref.LT, -0.0, 0.0) and not one(ref.EQ, -0.0, 0.0)
    assert one(ref.GT, nan_pos, np.inf) and one(ref.LT, nan_neg, -np.inf)
    assert not pc.equal(pa.array([nan_pos]), pa.array([nan_pos]))[0].as_py()
    assert not pc.less(pa.array([-0.0]), pa.array([0.0]))[0].as_py()
    # a float32 column against a double constant: the column is widened, 0.1f != 0.1
    f32 = np.array([0.1, 0.5], np.float32)
    got = ref.pair_pass([ref.Term(ref.GT, ref.FLOAT, (ref.BUILD, 0), (ref.CONST, ref.const_bits(ref.FLOAT, 0.1)))],
                        [ref.Col(f32)], [], 2, 1, [0, 1], [0, 0])
    assert got.tolist() == [True, True]


def test_ref_strings_against_pyarrow():
    s = ["", "a", "ab", "az", "aé", "b", "\x7f", "\u0080"]
    _against_pyarrow(ref.BYTES, [x.encode() for x in s], [x.encode() for x in s[::-1]])
    la, ra = pa.array(s), pa.array(s[::-1])
    want = pc.less(la, ra).to_numpy(zero_copy_only=False)
    got = ref.pair_pass([ref.Term(ref.LT, ref.BYTES, (ref.BUILD, 0), (ref.PROBE, 0))],
                        [ref.Col([x.encode() for x in s])], [ref.Col([x.encode() for x in s[::-1]])], len(s), len(s),
                        np.arange(len(s)), np.arange(len(s)))
    assert np.array_equal(got, want)
    b = [b"", b"\x7f", b"\x80", b"\x80\x00", b"\xff"]
    _against_pyarrow(ref.BYTES, b, b[::-1], np.array([1, 1, 1, 0, 1], bool), None)
    assert pc.less(pa.array([b"\x7f"]), pa.array([b"\x80"]))[0].as_py()       # unsigned bytes
    assert pc.less(pa.array(["az"]), pa.array(["aé"]))[0].as_py()              # 0x7a < 0xc3
    assert pc.less(pa.array(["a"]), pa.array(["ab"]))[0].as_py()               # a proper prefix is smaller


def test_ref_range_rule_and_bitmap():
    v = np.arange(4, dtype=np.int32)
    bidx = np.array([0, 3, 4, 2**64 - 1, 1], dtype=np.uint64)
    pidx = np.array([0, 1, 0, 0, 2**32 - 1], dtype=np.uint32)
    got = ref.pair_pass([ref.Term(ref.GE, ref.INT, (ref.BUILD, 0), (ref.CONST, 0))], [ref.Col(v)], [], 4, 2, bidx, pidx)
    assert got.tolist() == [True, True, False, False, False]
    bm = ref.bitmap(np.ones(65, bool))
    assert len(bm) == 16 and bm[:8].tolist() == [255] * 8 and bm[8:].tolist() == [1] + [0] * 7
    assert len(ref.bitmap(np.zeros(0, bool))) == 0


# ---- the C ABI without a GPU -----------------------------------------------------------------

class _Pred:
    """A predicate for hj_pair_predicate_check: over device memory where there is a GPU, else
    over a host buffer (the check cannot tell host from device memory without a GPU)."""

    def __init__(self, lib, terms, bwidths=(8,), pwidths=(8,), build_rows=4, probe_rows=4):
        if _no_gpu():
            self.buf = np.zeros(64, np.int64)
            p = self.buf.ctypes.data
        else:
            import torch

            self.buf = torch.zeros(64, dtype=torch.int64, device="cuda")
            p = self.buf.data_ptr()

        def cols(widths):
            arr = (lib.HjKeyColumn * max(len(widths), 1))()
            for i, w in enumerate(widths):
                arr[i] = lib.HjKeyColumn(p, p if w == 0 else None, None, 0, w, 4 if w == 0 else 0)
            return arr

        self.terms = (lib.HjPairTerm * max(len(terms), 1))(*[lib.HjPairTerm(*t) for t in terms])
        self.b, self.p = cols(bwidths), cols(pwidths)
        self.s = lib.HjPairPredicate(len(terms), self.terms, len(bwidths), self.b, build_rows, len(pwidths), self.p,
                                     probe_rows)


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_predicate_check(dfp):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    EQ, INT, UINT, FLT, BYT = _lib.HJ_CMP_EQ, _lib.HJ_VAL_INT, _lib.HJ_VAL_UINT, _lib.HJ_VAL_FLOAT, _lib.HJ_VAL_BYTES
    B, P, C = _lib.HJ_SIDE_BUILD, _lib.HJ_SIDE_PROBE, _lib.HJ_SIDE_CONST
    ok = [(EQ, INT, B, 0, P, 0, 0)]
    good = [
        _Pred(_lib, ok),
        _Pred(_lib, [(_lib.HJ_CMP_GE, UINT, P, 0, C, 99, -1)], bwidths=()),     # rhs_col ignored for a constant
        _Pred(_lib, [(EQ, INT, B, 0, P, 1, 0)], bwidths=(1,), pwidths=(16, 2)),  # mixed widths; an unused 16
        _Pred(_lib, [(EQ, FLT, B, 0, P, 0, 0)], bwidths=(4,), pwidths=(8,)),
        _Pred(_lib, [(EQ, BYT, B, 0, P, 0, 0)], bwidths=(0,), pwidths=(0,)),
        _Pred(_lib, ok * 16, build_rows=0, probe_rows=0),
    ]
    for g in good:
        assert L.hj_pair_predicate_check(g.s) == _lib.HJ_OK, L.hj_last_error()
    bad = {
        "op": _Pred(_lib, [(6, INT, B, 0, P, 0, 0)]),
        "op<0": _Pred(_lib, [(-1, INT, B, 0, P, 0, 0)]),
        "class": _Pred(_lib, [(EQ, 4, B, 0, P, 0, 0)]),
        "lhs side": _Pred(_lib, [(EQ, INT, 3, 0, P, 0, 0)]),
        "rhs side": _Pred(_lib, [(EQ, INT, B, 0, 3, 0, 0)]),
        "lhs const": _Pred(_lib, [(EQ, INT, C, 0, P, 0, 0)]),
        "lhs col": _Pred(_lib, [(EQ, INT, B, 1, P, 0, 0)]),
        "rhs col": _Pred(_lib, [(EQ, INT, B, 0, P, -1, 0)]),
        "col of an empty side": _Pred(_lib, [(EQ, INT, B, 0, P, 0, 0)], bwidths=()),
        "int width 16": _Pred(_lib, [(EQ, INT, B, 0, P, 0, 0)], bwidths=(16,)),
        "int width 0": _Pred(_lib, [(EQ, UINT, B, 0, P, 0, 0)], pwidths=(0,)),
        "float width 2": _Pred(_lib, [(EQ, FLT, B, 0, P, 0, 0)], bwidths=(2,)),
        "bytes width 8": _Pred(_lib, [(EQ, BYT, B, 0, P, 0, 0)], bwidths=(0,)),
        "bytes const": _Pred(_lib, [(EQ, BYT, B, 0, C, 0, 0)], bwidths=(0,)),
        "build rows": _Pred(_lib, ok, build_rows=-1),
        "probe rows": _Pred(_lib, ok, probe_rows=-1),
        "no terms": _Pred(_lib, []),
        "17 terms": _Pred(_lib, ok * 17),
        "17 cols": _Pred(_lib, ok, bwidths=(8,) * 17),
        "width 3": _Pred(_lib, ok, pwidths=(8, 3)),
        "second term": _Pred(_lib, ok + [(EQ, INT, B, 0, P, 5, 0)]),
    }
    nullcol = _Pred(_lib, ok)
    nullcol.b[0].values = None
    bad["null values"] = nullcol
    nulloff = _Pred(_lib, [(EQ, BYT, B, 0, P, 0, 0)], bwidths=(0,), pwidths=(0,))
    nulloff.p[0].offsets = None
    bad["null offsets"] = nulloff
    badoff = _Pred(_lib, [(EQ, BYT, B, 0, P, 0, 0)], bwidths=(0,), pwidths=(0,))
    badoff.b[0].offset_bytes = 2
    bad["offset width"] = badoff
    negv = _Pred(_lib, ok)
    negv.p[0].validity_offset = -1
    bad["validity offset"] = negv
    nullterms = _Pred(_lib, ok)
    nullterms.s.terms = None
    bad["null terms"] = nullterms
    nullcols = _Pred(_lib, ok)
    nullcols.s.build_cols = None
    bad["null build cols"] = nullcols
    for name, b in bad.items():
        assert L.hj_pair_predicate_check(b.s) == _lib.HJ_ERR_INVALID, name
        assert L.hj_last_error(), name
    assert L.hj_pair_predicate_check(None) == _lib.HJ_ERR_INVALID
    assert L.hj_pair_predicate_check(bad["second term"].s) == _lib.HJ_ERR_INVALID
    assert b"term 1" in L.hj_last_error()  # the message names the term
    # the device calls run the same check first, then the no-GPU check
    x = np.zeros(16, np.int64).ctypes.data
    for g in good if _no_gpu() else []:
        assert L.hj_pair_filter_test(g.s, x, x, 4, x, x, None) == _lib.HJ_ERR_NO_DEVICE
        assert L.hj_pair_filter_select(g.s, x, x, 4, x, x, x, x, None) == _lib.HJ_ERR_NO_DEVICE
    for name, b in bad.items():
        assert L.hj_pair_filter_test(b.s, x, x, 4, x, x, None) == _lib.HJ_ERR_INVALID, name
        assert L.hj_pair_filter_select(b.s, x, x, 4, x, x, x, x, None) == _lib.HJ_ERR_INVALID, name
    assert L.hj_pair_filter_test(None, x, x, 4, x, x, None) == _lib.HJ_ERR_INVALID


def test_predicate_check_rejects_without_buffers(dfp):
    """The error cases that need no column buffer at all hold on any machine."""
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    t = (_lib.HjPairTerm * 1)(_lib.HjPairTerm(0, 0, 0, 0, 1, 0, 0))
    s = _lib.HjPairPredicate(1, t, 0, None, 1, 0, None, 1)
    assert L.hj_pair_predicate_check(s) == _lib.HJ_ERR_INVALID  # column 0 of a side without columns
    assert b"term 0" in L.hj_last_error()
    t[0] = _lib.HjPairTerm(0, 0, _lib.HJ_SIDE_CONST, 0, _lib.HJ_SIDE_CONST, 0, 0)
    assert L.hj_pair_predicate_check(s) == _lib.HJ_ERR_INVALID
    s.nterms = 0
    assert L.hj_pair_predicate_check(s) == _lib.HJ_ERR_INVALID
    assert L.hj_pair_predicate_check(None) == _lib.HJ_ERR_INVALID
    assert L.hj_pair_filter_test(s, None, None, 0, None, None, None) == _lib.HJ_ERR_INVALID
    assert L.hj_pair_filter_select(s, None, None, 0, None, None, None, None, None) == _lib.HJ_ERR_INVALID


def test_workspace_bound(dfp):
    """About one bit per pair, for the pair filter and for hj_filter_equal_pairs alike (both
    keep one ballot word per 64 pairs and share the ordered compaction)."""
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    assert 0 < L.hj_pair_filter_workspace_bytes(1 << 24) < (1 << 24)
    assert L.hj_pair_filter_workspace_bytes(0) > 0 and L.hj_pair_filter_workspace_bytes(-5) > 0
    for n in (1, 4096, 4097, 10**7):
        w = L.hj_pair_filter_workspace_bytes(n)
        assert n // 8 <= w <= n // 8 + n // 256 + 2048, (n, w)
        e = L.hj_equal_pairs_workspace_bytes(n)
        assert n // 8 <= e <= n // 8 + n // 256 + 2048, (n, e)


def test_struct_layout_matches_the_header(dfp):
    from datafusion_parallelism_amd import _lib

    assert ctypes.sizeof(_lib.HjPairTerm) == 32 and _lib.HjPairTerm.rhs_const.offset == 24
    assert ctypes.sizeof(_lib.HjPairPredicate) == 64
    assert [_lib.HjPairPredicate.terms.offset, _lib.HjPairPredicate.build_cols.offset,
            _lib.HjPairPredicate.build_rows.offset, _lib.HjPairPredicate.probe_rows.offset] == [8, 24, 32, 56]


# ---- the Python predicate's type rules (no device memory: the checks come first) ----------------

class _FakeCol:
    def __init__(self, t, n=4):
        self.type, self.length = t, n


@pytest.mark.parametrize("lt,rt", [
    (pa.float16(), pa.float16()), (pa.decimal128(10, 2), pa.decimal128(10, 2)), (pa.int32(), pa.uint32()),
    (pa.int64(), pa.float64()), (pa.bool_(), pa.uint8()), (pa.timestamp("us"), pa.timestamp("ms")),
    (pa.date32(), pa.int32()), (pa.string(), pa.int8()), (pa.list_(pa.int8()), pa.list_(pa.int8())),
])
def test_unsupported_types_raise_type_error(dfp, lt, rt):
    from datafusion_parallelism_amd.columns import PairPredicate

    with pytest.raises(TypeError):
        PairPredicate([_FakeCol(lt)], [_FakeCol(rt)], [(("build", 0), "<", ("probe", 0))])


@pytest.mark.parametrize("t,const", [
    (pa.string(), "x"), (pa.binary(), b"x"), (pa.int32(), 1.5), (pa.int32(), True), (pa.uint8(), -1),
    (pa.int64(), 2**63), (pa.uint64(), 2**64), (pa.float64(), "1"), (pa.bool_(), 1), (pa.float16(), 1.0),
])
def test_unsupported_constants_raise_type_error(dfp, t, const):
    from datafusion_parallelism_amd.columns import PairPredicate

    with pytest.raises(TypeError):
        PairPredicate([_FakeCol(t)], [], [(("build", 0), "==", const)], probe_rows=4)


def test_compare_filter_terms_and_callable():
    """CompareFilter normalises constant-first terms and as_callable evaluates with pyarrow."""
    from datafusion_parallelism_amd.operator import CompareFilter, JoinFilter, L, R

    f = CompareFilter([(L("v"), "!=", R("v")), (5, "<", R("x")), (R("x"), "<=", L("hi"))])
    assert [(repr(a), op, repr(b)) for a, op, b in f.terms] == [
        ("L('v')", "!=", "R('v')"), ("R('x')", ">", "5"), ("R('x')", "<=", "L('hi')")]
    jf = f.as_callable()
    assert isinstance(jf, JoinFilter) and jf.left_columns == ["v", "hi"] and jf.right_columns == ["v", "x"]
    left = pa.RecordBatch.from_pydict({"v": ["a", "b", None, "q"], "hi": [10, 10, 10, 7]})
    right = pa.RecordBatch.from_pydict({"v": ["a", "c", "d", "r"], "x": [9, 9, 9, 8]})
    assert jf.expression(left, right).fill_null(False).to_pylist() == [False, True, False, False]
    with pytest.raises(ValueError):
        CompareFilter([(1, "<", 2)])
    with pytest.raises(ValueError):
        CompareFilter([(L("a"), "~", R("b"))])
    with pytest.raises(ValueError):
        CompareFilter([])
