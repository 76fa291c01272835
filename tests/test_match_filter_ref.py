"""CPU: the filtered match probe's contract as restated in match_filter_ref.py on KATs worked
by hand (all four semi / anti joins; a null operand, a null key, an id >= build_rows), and
hj_probe_match_filtered's argument checks without a table."""
import re
import subprocess

import numpy as np

import match_filter_ref as ref
import pair_filter_ref as pf
import probe_match_ref as pm

# build side: key, v (row 4's v is null); probe side: key, v. Predicate: L.v < R.v.
BUILD_K = [1, 1, 2, None, 2]
BUILD_V = pf.Col(np.array([10, 20, 30, 40, 0], np.int64), np.array([1, 1, 1, 1, 0], bool))
PROBE_K = [1, 2, None, 1, 3]
PROBE_V = pf.Col(np.array([15, 30, 5, 25, 1], np.int64))
LT = [pf.Term(pf.LT, pf.INT, (pf.BUILD, 0), (pf.PROBE, 0))]


def _kat(ids=None, nflags=5):
    ob, op = pm.inner_pairs(BUILD_K, PROBE_K)
    # S, probe rows ascending, each row's build rows descending
    assert ob.tolist() == [1, 0, 4, 2, 1, 0] and op.tolist() == [0, 0, 1, 1, 3, 3]
    if ids is not None:
        ob = np.asarray(ids, np.uint64)[ob.astype(np.int64)]
    return ref.expected(ob, op, 5, nflags, LT, [BUILD_V], [PROBE_V], 5)


def test_kat_pairs_that_pass():
    """(1,0): 20 < 15 no; (0,0): 10 < 15 yes; (4,1): null operand, not true; (2,1): 30 < 30 no;
    (1,3): 20 < 25 yes; (0,3): 10 < 25 yes. The null probe key (row 2) and the null build key
    (row 3) are in no pair."""
    e = _kat()
    assert e["counts"].tolist() == [1, 0, 0, 2, 0]
    assert e["bitmap"].tolist() == [0b01001, 0, 0, 0, 0, 0, 0, 0]
    assert e["flags"].tolist() == [1, 1, 0, 0, 0]
    assert (e["matched"], e["pairs"], e["candidates"]) == (2, 3, 6)


def test_kat_four_join_types():
    e = _kat()
    assert pm.select_rows(e["bitmap"], 5, 1).tolist() == [0, 3]            # RightSemi
    assert pm.select_rows(e["bitmap"], 5, 0).tolist() == [1, 2, 4]         # RightAnti keeps the null key
    assert np.flatnonzero(e["flags"] == 1).tolist() == [0, 1]              # LeftSemi
    assert np.flatnonzero(e["flags"] == 0).tolist() == [2, 3, 4]           # LeftAnti: null operand, null key


def test_kat_id_beyond_build_rows():
    """Explicit ids: the id is the build_idx and the row of the build columns. Row 0 carries id
    7 >= build_rows = 5: its pairs fail and nothing is read. Left: (1,3) alone."""
    e = _kat(ids=[7, 1, 2, 3, 4], nflags=8)
    assert e["counts"].tolist() == [0, 0, 0, 1, 0]
    assert e["bitmap"][0] == 0b01000
    assert e["flags"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    assert (e["matched"], e["pairs"], e["candidates"]) == (1, 1, 6)


def test_kat_flags_accumulate_and_cut_off():
    ob, op = pm.inner_pairs(BUILD_K, PROBE_K)
    e = ref.expected(ob, op, 5, 1, LT, [BUILD_V], [PROBE_V], 5, before=[0])
    assert e["flags"].tolist() == [1]                  # id 1 >= nflags is skipped
    e = ref.expected(ob, op, 5, 5, LT, [BUILD_V], [PROBE_V], 5, before=[0, 0, 1, 0, 9])
    assert e["flags"].tolist() == [1, 1, 1, 0, 9]      # OR into arbitrary prior contents


def test_stats_minus_one_rules():
    e = _kat()
    assert ref.stats(e, bitmap=True, counts=True) == [2, 3, 6]
    assert ref.stats(e, bitmap=True, counts=False) == [2, -1, 6]
    assert ref.stats(e, bitmap=False, counts=True) == [2, 3, 6]
    assert ref.stats(e, bitmap=False, counts=False) == [-1, -1, 6]


# ---- the C ABI without a table ------------------------------------------------------------------

class _Pred:
    """An hj_pair_predicate over device memory where there is a GPU, else over a host buffer
    (the check cannot tell host from device memory without a GPU)."""

    def __init__(self, lib, terms, probe_rows=8):
        import torch

        if torch.cuda.is_available():
            self.buf = torch.zeros(64, dtype=torch.int64, device="cuda")
            p = self.buf.data_ptr()
        else:
            self.buf = np.zeros(64, np.int64)
            p = self.buf.ctypes.data
        self.terms = (lib.HjPairTerm * len(terms))(*[lib.HjPairTerm(*t) for t in terms])
        self.b = (lib.HjKeyColumn * 1)(lib.HjKeyColumn(p, None, None, 0, 8, 0))
        self.p = (lib.HjKeyColumn * 1)(lib.HjKeyColumn(p, None, None, 0, 8, 0))
        self.s = lib.HjPairPredicate(len(terms), self.terms, 1, self.b, 8, 1, self.p, probe_rows)


def test_symbol_is_exported_and_bound(dfp):
    from datafusion_parallelism_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "hj_probe_match_filtered" in set(re.findall(r" T (hj_[a-z0-9_]+)", out))
    assert "hj_probe_match_filtered" in {n for n, _, _ in _lib.SIGNATURES}
    assert _lib.load().hj_probe_match_filtered is not None


def test_predicate_checks_come_first(dfp):
    """An invalid predicate is HJ_ERR_INVALID naming the term, before the table is looked at and
    with or without a GPU; a valid one leaves what hj_probe_match says of a null table."""
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    B, P = _lib.HJ_SIDE_BUILD, _lib.HJ_SIDE_PROBE
    x = np.zeros(16, np.int64)
    p = x.ctypes.data
    ok = (_lib.HJ_CMP_LT, _lib.HJ_VAL_INT, B, 0, P, 0, 0)
    bad = _Pred(_lib, [ok, (9, _lib.HJ_VAL_INT, B, 0, P, 0, 0)])
    assert L.hj_probe_match_filtered(None, p, None, 0, 8, bad.s, p, None, None, 0, p, None) == _lib.HJ_ERR_INVALID
    assert b"term 1" in L.hj_last_error() and b"bad op" in L.hj_last_error()
    bad = _Pred(_lib, [(_lib.HJ_CMP_EQ, _lib.HJ_VAL_INT, B, 3, P, 0, 0)])
    assert L.hj_probe_match_filtered(None, p, None, 0, 8, bad.s, p, None, None, 0, p, None) == _lib.HJ_ERR_INVALID
    assert b"term 0" in L.hj_last_error()
    assert L.hj_probe_match_filtered(None, p, None, 0, 8, None, p, None, None, 0, p, None) == _lib.HJ_ERR_INVALID
    assert b"null pair predicate" in L.hj_last_error()
    good = _Pred(_lib, [ok])
    want = L.hj_probe_match(None, p, None, 0, 8, p, None, None, 0, p, p, None)
    assert want == _lib.HJ_ERR_INVALID and b"null table" in L.hj_last_error()
    assert L.hj_probe_match_filtered(None, p, None, 0, 8, good.s, p, None, None, 0, p, None) == want
    assert b"null table" in L.hj_last_error()
