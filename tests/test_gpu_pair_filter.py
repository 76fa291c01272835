"""GPU: the pair filter (hj_pair_filter_test / hj_pair_filter_select, include/hj.h) against
its numpy restatement (tests/pair_filter_ref.py), bit for bit: bitmap, count, the selected
pairs and their order; untouched memory around every output; the operator's CompareFilter
against the host JoinFilter it describes."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_filter_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NB, NP = 1000, 700  # build rows, probe rows of the shared sides
# one below, at and one above the ballot word (64) and the tile (4096 pairs), every power of
# two up to 16384, and a size of several tiles that is a multiple of neither
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 50_000]
SENT_B, SENT_P = -0x0123456789ABCDEF, 0x5A5A5A5A


def _lib_():
    from datafusion_parallelism_amd import _lib

    return _lib, _lib.load()


# ---- columns: the same values as a numpy reference column and as a device column -----------

def make_col(values, valid=None, voff=0, typ=None):
    """(ref.Col, DeviceColumn): `voff` rows are put in front and sliced off again, so the
    device column's validity bitmap starts at bit voff."""
    from datafusion_parallelism_amd.columns import DeviceColumn

    n = len(values)
    if isinstance(values, np.ndarray):
        full = np.concatenate([np.zeros(voff, values.dtype), values])
    else:
        full = [b"pad"] * voff + list(values)
    mask = None if valid is None else np.concatenate([np.zeros(voff, bool), ~valid])
    if isinstance(full, list) and typ in (pa.string(), pa.large_string()):
        full = [x.decode() for x in full]
    arr = pa.array(full, type=typ, mask=mask)[voff:]
    col = DeviceColumn.from_arrow(arr, DEV)
    assert col.length == n and (valid is None or col.voff == voff)
    return ref.Col(values, valid), col


_SIDES = {}


def sides():
    """Both sides' columns, made once: ints and uints of every width, floats, strings; nulls
    on either side with validity offsets 3 (build) and 13 (probe); some columns without
    validity."""
    if _SIDES:
        return _SIDES
    rng = np.random.default_rng(11)
    words = [b"", b"a", b"ab", b"abc", b"az", "aé".encode(), b"b", b"\x7f", b"\x80", b"\x80\x00", b"\xff", b"abcdefghij"]
    utf = ["", "a", "ab", "abc", "az", "aé", "b", "\x7f", "\u0080", "zz", "aéb", "abcdefghijklmnopq"]
    for side, rows, voff in (("b", NB, 3), ("p", NP, 13)):
        cols = {}
        for w in (1, 2, 4, 8):
            # small range: many equal values, so EQ / LE / GE have both outcomes
            cols[f"i{w}"] = make_col(rng.integers(-5, 6, rows).astype(f"int{8 * w}"), rng.random(rows) < 0.85, voff)
            cols[f"u{w}"] = make_col(rng.integers(0, 7, rows).astype(f"uint{8 * w}"),
                                     (rng.random(rows) < 0.85) if side == "b" else None, voff)
        big = np.array([0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1], np.uint64)
        cols["u8big"] = make_col(big[rng.integers(0, 6, rows)], None if side == "b" else rng.random(rows) < 0.9, voff)
        cols["i8big"] = make_col(rng.integers(-2**62, 2**62, rows), None, voff)
        rc, dc = make_col(rng.random(rows) < 0.5, rng.random(rows) < 0.9, voff)
        cols["bool"] = (ref.Col(rc.values.astype(np.uint8), rc.valid), dc)  # one byte, 0 / 1, on the device
        spec64 = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, 0.1, 3.0], np.float64)
        nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001], np.uint64).view(np.float64)
        f8 = np.concatenate([spec64, nans])[rng.integers(0, 11, rows)]
        cols["f8"] = make_col(f8, rng.random(rows) < 0.9, voff)
        f4 = np.concatenate([spec64.astype(np.float32),
                             np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)])[rng.integers(0, 10, rows)]
        cols["f4"] = make_col(f4, None if side == "p" else rng.random(rows) < 0.9, voff)
        cols["bin"] = make_col([words[i] for i in rng.integers(0, len(words), rows)], rng.random(rows) < 0.9, voff,
                               pa.binary() if side == "b" else pa.large_binary())
        cols["str"] = make_col([utf[i].encode() for i in rng.integers(0, len(utf), rows)],
                               None if side == "b" else rng.random(rows) < 0.9, voff,
                               pa.string() if side == "b" else pa.large_string())
        _SIDES[side] = cols
    return _SIDES


_PAIRS = {}


def pairs(n):
    """n candidate pairs as a probe emits them - probe rows ascending, each row's build rows
    descending, duplicates on both sides - with out-of-range and all-ones indices mixed in."""
    if n not in _PAIRS:
        rng = np.random.default_rng(n + 5)
        p = np.sort(rng.integers(0, NP, n)).astype(np.uint32)
        b = rng.integers(0, NB // 4, n).astype(np.uint64) * np.uint64(4)
        order = np.lexsort((-b.astype(np.int64), p))
        b, p = b[order], p[order]
        bad = rng.random(n)
        b[bad < 0.02] = np.uint64(NB)
        b[(bad >= 0.02) & (bad < 0.04)] = np.uint64(2**64 - 1)
        b[(bad >= 0.04) & (bad < 0.05)] = np.uint64(2**32 + 3)
        p[(bad >= 0.05) & (bad < 0.07)] = np.uint32(NP)
        p[(bad >= 0.07) & (bad < 0.09)] = np.uint32(2**32 - 1)
        _PAIRS[n] = (b, p, torch.from_numpy(b.view(np.int64)).to(DEV), torch.from_numpy(p.view(np.int32)).to(DEV))
    return _PAIRS[n]


CLS = {"i": ref.INT, "u": ref.UINT, "f": ref.FLOAT, "b": ref.BYTES, "s": ref.BYTES}


def predicate(terms):
    """terms: (("b" | "p", column name), op, ("b" | "p", column name) | constant) ->
    (ref terms, ref build cols, ref probe cols, PairPredicate)."""
    from datafusion_parallelism_amd.columns import PairPredicate

    S = sides()
    names = {"b": [], "p": []}

    def idx(side, name):
        if name not in names[side]:
            names[side].append(name)
        return names[side].index(name)

    rterms, dterms = [], []
    for (ls, ln), op, rhs in terms:
        cls = ref.UINT if ln == "bool" else CLS[ln[0]]
        lref = (ref.BUILD if ls == "b" else ref.PROBE, idx(ls, ln))
        if isinstance(rhs, tuple):
            rs, rn = rhs
            rref = (ref.BUILD if rs == "b" else ref.PROBE, idx(rs, rn))
            dterms.append((("build" if ls == "b" else "probe", lref[1]), op, ("build" if rs == "b" else "probe", rref[1])))
        else:
            rref = (ref.CONST, ref.const_bits(cls, rhs))
            dterms.append((("build" if ls == "b" else "probe", lref[1]), op, rhs))
        rterms.append(ref.Term(ref.OPS[op], cls, lref, rref))
    rb, rp = [S["b"][n][0] for n in names["b"]], [S["p"][n][0] for n in names["p"]]
    pred = PairPredicate([S["b"][n][1] for n in names["b"]], [S["p"][n][1] for n in names["p"]], dterms, NB, NP)
    return rterms, rb, rp, pred


# ---- raw calls with guarded outputs ------------------------------------------------------------

def launch_test(pred, b, p):
    lib, L = _lib_()
    n = b.numel()
    nbytes = ((n + 63) // 64) * 8
    bm = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)  # never zeroed by the caller
    cnt = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    lib.check(L.hj_pair_filter_test(pred.struct, b.data_ptr() if n else None, p.data_ptr() if n else None, n,
                                    bm.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream().cuda_stream or None))
    return bm, cnt, nbytes


def run_test(pred, b, p):
    bm, cnt, nbytes = launch_test(pred, b, p)
    host = bm.cpu().numpy()
    assert np.all(host[nbytes:] == 0xFF), "bytes past the bitmap were written"
    return host[:nbytes], int(cnt.item())


def launch_select(pred, b, p, stream=None):
    lib, L = _lib_()
    n = b.numel()
    ob = torch.full((n + 16,), SENT_B, dtype=torch.int64, device=DEV)
    op = torch.full((n + 16,), SENT_P, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.hj_pair_filter_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream()
    lib.check(L.hj_pair_filter_select(pred.struct, b.data_ptr() if n else None, p.data_ptr() if n else None, n,
                                      ob.data_ptr(), op.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                      s.cuda_stream or None))
    return ob, op, cnt, ws


def finish_select(out):
    ob, op, cnt, _ = out
    m = int(cnt.item())
    ob, op = ob.cpu().numpy(), op.cpu().numpy()
    assert np.all(ob[m:] == SENT_B) and np.all(op[m:] == SENT_P), "outputs at or beyond *d_count were written"
    return ob[:m].view(np.uint64), op[:m].view(np.uint32)


def check_against_ref(terms, n):
    rterms, rb, rp, pred = predicate(terms)
    b, p, db, dp = pairs(n)
    want = ref.pair_pass(rterms, rb, rp, NB, NP, b, p)
    bm, cnt = run_test(pred, db, dp)
    assert cnt == int(want.sum()), (terms, n, cnt, int(want.sum()))
    assert np.array_equal(bm, ref.bitmap(want)), (terms, n)
    gb, gp = finish_select(launch_select(pred, db, dp))
    wb, wp = ref.select(want, b, p)
    assert np.array_equal(gb, wb) and np.array_equal(gp, wp), (terms, n)
    return want


# ---- 1. sizes ----------------------------------------------------------------------------------

MIXED = [(("b", "i1"), "<=", ("p", "i8")), (("p", "f4"), "!=", ("b", "f8")), (("b", "u2"), "<", 5),
         (("b", "bin"), ">=", ("p", "bin"))]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(dfp, n):
    """A predicate of all four classes (nulls on both sides, validity offsets 3 and 13) at
    every size around the ballot word and the tile, and over several tiles."""
    want = check_against_ref(MIXED, n)
    if n >= 4095:
        assert 0 < want.sum() < n
    # only fixed-width terms: the instantiation without the BYTES loop
    check_against_ref(MIXED[:3], n)


# ---- 2. every op x class, widths, constants ------------------------------------------------------

OPS = ["==", "!=", "<", "<=", ">", ">="]
N_OPS = 4097 + 64


@pytest.mark.parametrize("kind", ["i", "u"])
def test_int_ops_and_widths(dfp, kind):
    for op in OPS:
        for lw, rw in [(1, 8), (2, 4), (4, 2), (8, 1), (8, 8), (1, 1)]:
            want = check_against_ref([(("b", f"{kind}{lw}"), op, ("p", f"{kind}{rw}"))], N_OPS)
            assert 0 < want.sum() < N_OPS
        for w in (1, 2, 4, 8):
            check_against_ref([(("p", f"{kind}{w}"), op, 3)], N_OPS)
        check_against_ref([(("p", f"{kind}4"), op, ("p", f"{kind}2"))], N_OPS)  # both operands of one side
    if kind == "i":
        for op in OPS:
            check_against_ref([(("b", "i2"), op, -2)], N_OPS)
            check_against_ref([(("b", "i8big"), op, ("p", "i8big"))], N_OPS)
            check_against_ref([(("b", "i8big"), op, -2**61)], N_OPS)
            check_against_ref([(("b", "i1"), op, 2**40)], N_OPS)  # a constant wider than the column
    else:
        for op in OPS:
            for c in (2**63, 2**63 + 1, 2**64 - 1, 2**63 - 1, 0):
                check_against_ref([(("b", "u8big"), op, c)], N_OPS)
            check_against_ref([(("b", "u8big"), op, ("p", "u8big"))], N_OPS)
            check_against_ref([(("b", "u1"), op, ("p", "u8big"))], N_OPS)
            check_against_ref([(("b", "bool"), op, ("p", "bool"))], N_OPS)
            check_against_ref([(("b", "bool"), op, True)], N_OPS)


def test_float_ops(dfp):
    """+-0, +-inf and NaNs of both signs in IEEE totalOrder; float32 against float64 and
    against a double constant."""
    for op in OPS:
        for l, r in [("f8", "f8"), ("f4", "f8"), ("f8", "f4"), ("f4", "f4")]:
            want = check_against_ref([(("b", l), op, ("p", r))], N_OPS)
            assert 0 < want.sum() < N_OPS
        for c in (0.0, -0.0, 0.1, float(np.float32(0.1)), float("inf"), float("-inf"), float("nan"), 1.5):
            check_against_ref([(("b", "f4"), op, c)], N_OPS)
            check_against_ref([(("p", "f8"), op, c)], N_OPS)
    nan_neg = float(np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0])
    want = check_against_ref([(("p", "f8"), "==", nan_neg)], N_OPS)
    assert want.sum() > 0  # the NaN of the same bits is equal


def test_bytes_ops(dfp):
    """Binary against LargeBinary and Utf8 against LargeUtf8: empty strings, prefixes, bytes
    >= 0x80, unsigned order."""
    for op in OPS:
        for name in ("bin", "str"):
            want = check_against_ref([(("b", name), op, ("p", name))], N_OPS)
            assert 0 < want.sum() < N_OPS
            check_against_ref([(("p", name), op, ("b", name))], N_OPS)
        check_against_ref([(("b", "bin"), op, ("b", "str"))], N_OPS)  # 4-byte offsets on both operands


def test_temporal_columns(dfp):
    """date32 (4 bytes) and timestamp (8 bytes) compare as INT of their width, against a
    column of the same Arrow type and against an int constant in the type's unit."""
    from datafusion_parallelism_amd.columns import DeviceColumn, PairPredicate

    rng = np.random.default_rng(8)
    d_b, d_p = rng.integers(-50, 50, NB).astype(np.int32), rng.integers(-50, 50, NP).astype(np.int32)
    t_b, t_p = rng.integers(-10**12, 10**12, NB), rng.integers(-10**12, 10**12, NP)
    vb, vp = rng.random(NB) < 0.9, rng.random(NP) < 0.9
    dev = lambda v, t, valid: DeviceColumn.from_arrow(pa.array(v, mask=~valid).cast(t), DEV)
    pred = PairPredicate([dev(d_b, pa.date32(), vb), dev(t_b, pa.timestamp("us"), vb)],
                         [dev(d_p, pa.date32(), vp), dev(t_p, pa.timestamp("us"), vp)],
                         [(("build", 0), "<=", ("probe", 0)), (("probe", 1), ">", ("build", 1)), (("probe", 0), ">=", -40)])
    rterms = [ref.Term(ref.LE, ref.INT, (ref.BUILD, 0), (ref.PROBE, 0)),
              ref.Term(ref.GT, ref.INT, (ref.PROBE, 1), (ref.BUILD, 1)),
              ref.Term(ref.GE, ref.INT, (ref.PROBE, 0), (ref.CONST, -40))]
    b, p, db, dp = pairs(4097)
    want = ref.pair_pass(rterms, [ref.Col(d_b, vb), ref.Col(t_b, vb)], [ref.Col(d_p, vp), ref.Col(t_p, vp)], NB, NP, b, p)
    assert 0 < want.sum() < len(want)
    bm, cnt = run_test(pred, db, dp)
    assert cnt == want.sum() and np.array_equal(bm, ref.bitmap(want))
    gb, gp = finish_select(launch_select(pred, db, dp))
    assert np.array_equal(gb, b[want]) and np.array_equal(gp, p[want])


def test_true_everywhere_and_false_everywhere(dfp):
    from datafusion_parallelism_amd.columns import PairPredicate, pair_filter_select, pair_filter_test

    for n in (4096, 5000):
        b = torch.arange(n, dtype=torch.int64, device=DEV) % NB
        p = (torch.arange(n, dtype=torch.int64, device=DEV) % NP).to(torch.int32)
        col = sides()["b"]["i8big"][1]
        for op, all_pass in (("==", True), ("<", False)):
            pred = PairPredicate([col], [], [(("build", 0), op, ("build", 0))], NB, NP)
            bm, cnt = run_test(pred, b, p)
            assert cnt == (n if all_pass else 0)
            assert np.array_equal(bm, ref.bitmap(np.full(n, all_pass)))
            gb, gp = finish_select(launch_select(pred, b, p))
            assert len(gb) == cnt and (not all_pass or (np.array_equal(gb.view(np.int64), b.cpu().numpy())
                                                        and np.array_equal(gp.view(np.int32), p.cpu().numpy())))
            # the wrappers of columns.py
            wb, wcnt = pair_filter_test(pred, b, p)
            sb, sp = pair_filter_select(pred, b, p)
            assert wcnt == cnt and sb.numel() == cnt and sp.numel() == cnt
            assert np.array_equal(wb.cpu().numpy()[: len(bm)], bm)


def test_sixteen_terms_over_sixteen_and_sixteen_columns(dfp):
    from datafusion_parallelism_amd.columns import PairPredicate

    rng = np.random.default_rng(3)
    bcols = [make_col(rng.integers(0, 40, NB).astype(np.int32), rng.random(NB) < 0.97, 3) for _ in range(16)]
    pcols = [make_col(rng.integers(0, 4, NP).astype(np.int64), rng.random(NP) < 0.97, 13) for _ in range(16)]
    pred = PairPredicate([c[1] for c in bcols], [c[1] for c in pcols],
                         [(("build", j), ">=", ("probe", 15 - j)) for j in range(16)])
    rterms = [ref.Term(ref.GE, ref.INT, (ref.BUILD, j), (ref.PROBE, 15 - j)) for j in range(16)]
    b, p, db, dp = pairs(16385)
    want = ref.pair_pass(rterms, [c[0] for c in bcols], [c[0] for c in pcols], NB, NP, b, p)
    assert 0 < want.sum() < len(want)
    bm, cnt = run_test(pred, db, dp)
    assert cnt == want.sum() and np.array_equal(bm, ref.bitmap(want))
    gb, gp = finish_select(launch_select(pred, db, dp))
    assert np.array_equal(gb, b[want]) and np.array_equal(gp, p[want])


# ---- 3. select against test, concurrency, arguments ----------------------------------------------

def test_select_equals_the_pairs_compressed_by_tests_bitmap(dfp):
    _, _, _, pred = predicate(MIXED)
    b, p, db, dp = pairs(50_000)
    bm, cnt = run_test(pred, db, dp)
    keep = np.unpackbits(bm, bitorder="little")[: len(b)].astype(bool)
    gb, gp = finish_select(launch_select(pred, db, dp))
    assert len(gb) == cnt and np.array_equal(gb, b[keep]) and np.array_equal(gp, p[keep])


def test_two_selects_on_two_streams(dfp):
    cases = [predicate(MIXED), predicate([(("b", "str"), "<", ("p", "str")), (("p", "i4"), ">", -3)])]
    b, p, db, dp = pairs(50_000)
    wants = [ref.pair_pass(rt, rb, rp, NB, NP, b, p) for rt, rb, rp, _ in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for _ in range(3):
        for (_, _, _, pred), s in zip(cases, streams):
            with torch.cuda.stream(s):
                outs.append(launch_select(pred, db, dp, s))  # each call its own workspace
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        gb, gp = finish_select(out)
        assert np.array_equal(gb, b[wants[k % 2]]) and np.array_equal(gp, p[wants[k % 2]])


def test_argument_checks(dfp):
    lib, L = _lib_()
    INV = lib.HJ_ERR_INVALID
    _, _, _, pred = predicate(MIXED[:2])
    n = 1000
    _, _, db, dp = pairs(4095)
    b, p = db[:n].contiguous(), dp[:n].contiguous()
    ob = torch.zeros(n + 8, dtype=torch.int64, device=DEV)
    op = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    bm = torch.zeros(((n + 63) // 64) * 8 + 8, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.hj_pair_filter_workspace_bytes(n) + 8, dtype=torch.uint8, device=DEV)
    B, P, OB, OP, C, BM, WS = (t.data_ptr() for t in (b, p, ob, op, cnt, bm, ws))
    sel = lambda *a: L.hj_pair_filter_select(pred.struct, *a, None)
    tst = lambda *a: L.hj_pair_filter_test(pred.struct, *a, None)
    assert sel(B, P, n, OB, OP, C, WS) == lib.HJ_OK and tst(B, P, n, BM, C) == lib.HJ_OK
    torch.cuda.synchronize()
    # aliasing: the same buffers, and a partial overlap
    assert sel(B, P, n, B, OP, C, WS) == INV and sel(B, P, n, OB, P, C, WS) == INV
    assert sel(B, P, n - 8, B + 64, OP, C, WS) == INV and sel(B + 64, P, n - 8, B, OP, C, WS) == INV
    # misalignment
    assert sel(B, P, n, OB + 4, OP, C, WS) == INV and sel(B, P, n, OB, OP + 2, C, WS) == INV
    assert sel(B, P, n, OB, OP, C + 4, WS) == INV and sel(B, P, n, OB, OP, C, WS + 1) == INV
    assert tst(B, P, n, BM + 1, C) == INV and tst(B, P, n, BM, C + 4) == INV
    # null arguments
    assert sel(B, P, n, None, OP, C, WS) == INV and sel(B, P, n, OB, None, C, WS) == INV
    assert sel(B, P, n, OB, OP, None, WS) == INV and sel(B, P, n, OB, OP, C, None) == INV
    assert sel(None, P, n, OB, OP, C, WS) == INV and sel(B, None, n, OB, OP, C, WS) == INV
    assert tst(B, P, n, None, C) == INV and tst(B, P, n, BM, None) == INV and tst(None, P, n, BM, C) == INV
    # sizes
    assert sel(B, P, -1, OB, OP, C, WS) == INV and sel(B, P, 1 << 40, OB, OP, C, WS) == INV
    assert tst(B, P, -1, BM, C) == INV and tst(B, P, 1 << 40, BM, C) == INV
    # host memory: outputs, and a predicate whose column lies in host memory
    host = np.zeros(2 * n, np.int64)
    assert sel(B, P, n, host.ctypes.data, OP, C, WS) == INV and tst(B, P, n, BM, host.ctypes.data) == INV
    col = lib.HjKeyColumn(host.ctypes.data, None, None, 0, 8, 0)
    term = lib.HjPairTerm(0, 0, 0, 0, 2, 0, 0)
    hp = lib.HjPairPredicate(1, (lib.HjPairTerm * 1)(term), 1, (lib.HjKeyColumn * 1)(col), n, 0, None, n)
    assert L.hj_pair_predicate_check(hp) == INV and b"device" in L.hj_last_error()
    assert L.hj_pair_filter_test(hp, B, P, n, BM, C, None) == INV
    # n == 0 still writes the count
    cnt.fill_(-1)
    assert sel(None, None, 0, None, None, C, WS) == lib.HJ_OK and int(cnt[0].item()) == 0
    cnt.fill_(-1)
    assert tst(None, None, 0, None, C) == lib.HJ_OK and int(cnt[0].item()) == 0


# ---- 4. a scan of the tile totals beyond its first level ---------------------------------------

def test_large_scan(dfp):
    """launch_scan_u64 scans segments of 4096 values (256 threads x 16) and then the segment
    sums: more than 4096 tiles of 4096 pairs, i.e. more than 2^24 pairs, leave its first
    level. Indices and the expected result are made on the device."""
    from datafusion_parallelism_amd.columns import DeviceColumn, PairPredicate, pair_filter_select, pair_filter_test

    n = (1 << 24) + 3 * 4096 + 77
    g = torch.Generator(device=DEV).manual_seed(5)
    bv = torch.randint(-1000, 1000, (NB,), dtype=torch.int64, device=DEV, generator=g)
    pv = torch.randint(-1000, 1000, (NP,), dtype=torch.int64, device=DEV, generator=g)
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    b = (i * 7) % NB
    p = (i % NP).to(torch.int32)
    pred = PairPredicate([DeviceColumn(pa.int64(), NB, data=bv.view(torch.uint8))],
                         [DeviceColumn(pa.int64(), NP, data=pv.view(torch.uint8))], [(("build", 0), "<", ("probe", 0))])
    keep = bv[b] < pv[p.to(torch.int64)]
    want = int(keep.sum().item())
    assert n // 4 < want < 3 * n // 4
    gb, gp = pair_filter_select(pred, b, p)
    assert gb.numel() == want and torch.equal(gb, b[keep]) and torch.equal(gp, p[keep])
    _, cnt = pair_filter_test(pred, b, p)
    assert cnt == want


# ---- 5. operator ---------------------------------------------------------------------------------

def _rows(tbl):
    return [tuple(tbl.column(i)[r].as_py() for i in range(tbl.num_columns)) for r in range(tbl.num_rows)]


def test_kat_full_join_with_compare_filter(dfp):
    """src/lib.rs:651-726: ON left.id = right.id AND left.value != right.value, the filter on
    the string columns evaluated on the device."""
    from datafusion_parallelism_amd.operator import CompareFilter, L, ParallelHashJoin, R

    ids = lambda v: pa.array(v, pa.int32())
    left = pa.RecordBatch.from_pydict({"id": ids([1, 2, 3, None]), "value": ["left", "left", "same", "left"]})
    right = pa.RecordBatch.from_pydict({"id": ids([2, 3, 4, None]), "value": ["right", "same", "right", "right"]})
    flt = CompareFilter([(L("value"), "!=", R("value"))])
    got = pa.Table.from_batches(ParallelHashJoin([[left]], [[right]], on=[("id", "id")], join_type="full", filter=flt,
                                                 right_schema=right.schema).collect())
    want = [(1, "left", None, None), (2, "left", 2, "right"), (3, "same", None, None), (None, None, 3, "same"),
            (None, None, 4, "right"), (None, None, None, "right"), (None, "left", None, None)]
    assert sorted(_rows(got), key=repr) == sorted(want, key=repr)


JOIN_TYPES = ["inner", "left", "right", "full", "leftsemi", "leftanti", "rightsemi", "rightanti"]


def _band_sides():
    """A key of 55 duplicates per value on the build side; int and float payloads with nulls,
    no NaN and no -0.0 (there pyarrow's IEEE comparison and totalOrder agree)."""
    rng = np.random.default_rng(23)
    nb, npr = 110, 16
    left = pa.Table.from_pydict({
        "id": pa.array(np.repeat([0, 1], 55), mask=rng.random(nb) < 0.03), "bid": np.arange(nb),
        "lo": pa.array(rng.integers(0, 60, nb), mask=rng.random(nb) < 0.1),
        "hi": pa.array(rng.uniform(20, 120, nb), mask=rng.random(nb) < 0.1)})
    right = pa.Table.from_pydict({
        "id": pa.array(rng.integers(0, 3, npr), mask=rng.random(npr) < 0.05), "pid": np.arange(npr),
        "ts": pa.array(rng.integers(0, 100, npr), mask=rng.random(npr) < 0.1),
        "x": pa.array(rng.uniform(0, 100, npr).astype(np.float32), mask=rng.random(npr) < 0.1)})
    return left, right


@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_operator_compare_filter_equals_its_callable(dfp, jt, monkeypatch):
    """R.ts >= L.lo AND R.x < L.hi on the device against the same filter as a host callable:
    the same rows in the same order, unbounded and under max_output_rows=7, with and
    without the key filter; the device path never evaluates on the host."""
    from datafusion_parallelism_amd import operator as opm
    from datafusion_parallelism_amd.operator import CompareFilter, L, ParallelHashJoin, R

    left, right = _band_sides()
    flt = CompareFilter([(R("ts"), ">=", L("lo")), (R("x"), "<", L("hi"))])
    host = flt.as_callable()
    host_calls = []
    real = host.expression
    host.expression = lambda l, r: (host_calls.append(1), real(l, r))[1]
    spied = []
    monkeypatch.setattr(CompareFilter, "as_callable", lambda self: spied.append("as_callable"))
    monkeypatch.setattr(opm.JoinFilter, "__init__", lambda self, *a, **k: spied.append("JoinFilter"))

    def join(f, **kw):
        out = ParallelHashJoin([left.to_batches()], [right.to_batches()], on=[("id", "id")], join_type=jt, filter=f,
                               right_schema=right.schema, **kw).collect()
        return out

    for prefilter in (False, True):
        for limit in (None, 7):
            kw = dict(prefilter=prefilter, **({"max_output_rows": limit} if limit else {}))
            before = len(host_calls)
            want = join(host, **kw)
            assert len(host_calls) > before  # the spy sees the host path
            assert not spied
            got = join(flt, **kw)
            assert not spied, spied
            assert len(got) == len(want)
            if limit:
                assert all(x.num_rows <= limit for x in got)
            tg, tw = pa.Table.from_batches(got), pa.Table.from_batches(want)
            assert tg.num_rows > 0 and tg.equals(tw), (jt, prefilter, limit)


def test_operator_unsupported_type_raises(dfp):
    """No silent host fallback: a type the device does not compare is a TypeError."""
    from datafusion_parallelism_amd.operator import CompareFilter, L, ParallelHashJoin, R

    left = pa.RecordBatch.from_pydict({"id": pa.array([1, 2], pa.int32()), "v": pa.array([1, 2], pa.int32())})
    right = pa.RecordBatch.from_pydict({"id": pa.array([1, 2], pa.int32()), "v": pa.array([1.0, 2.0], pa.float64())})
    with pytest.raises(TypeError):
        ParallelHashJoin([[left]], [[right]], on=[("id", "id")], filter=CompareFilter([(L("v"), "<", R("v"))]),
                         right_schema=right.schema).collect()
