"""GPU: the filtered pair plan (hj_pair_plan_filtered / hj_pair_window_filtered). Every
expectation is match_filter_ref.filtered_pairs / expected over the oracle's inner pairs: F,
its statistics, bitmap and flags; a window is the slice [lo, lo + cap) of that F. Nothing is
expected from the library's own pair path."""
import numpy as np
import pytest
import torch

import match_filter_ref as ref
import pair_filter_ref as pf
import pair_window_ref as pw
import probe_match_ref as pm
import test_gpu_match_filter as mmf  # its builds of every multiplicity and layout, int_col, cuda
import test_gpu_pair_filter as pft   # its columns of every class and width
from key_filter_ref import pack_validity

pytestmark = pytest.mark.gpu

cuda, int_col, lt_predicate, LT = mmf.cuda, mmf.int_col, mmf.lt_predicate, mmf.LT
SENT_B, SENT_P = -0x0123456789ABCDEF, 0x5A5A5A5A


def plan_raw(t, keys, n, pred, valid=None, voff=0, bitmap=True, flags=None, nflags=0, stats=True):
    """hj_pair_plan_filtered on raw pointers: the plan is followed by 8 guard bytes, the bitmap
    is pre-filled with 0xFF and guarded, the statistics hold garbage and a guard."""
    size = t.pair_plan_filtered_bytes(n)
    plan = torch.full((size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    nb = pm.bitmap_bytes(n)
    bm = torch.full((nb + 8,), 0xFF, dtype=torch.uint8, device="cuda") if bitmap else None
    st = torch.full((4,), -7, dtype=torch.int64, device="cuda") if stats else None
    t.pair_plan_filtered_async(keys.data_ptr(), n, pred, plan.data_ptr(), torch.cuda.current_stream().cuda_stream,
                               None if valid is None else valid.data_ptr(), voff,
                               None if bm is None else bm.data_ptr(), None if flags is None else flags.data_ptr(),
                               nflags, None if st is None else st.data_ptr())
    torch.cuda.synchronize()
    assert (plan[size:] == 0xA5).all(), "plan guard bytes overwritten"
    out = {}
    if bitmap:
        b = bm.cpu().numpy()
        assert (b[nb:] == 0xFF).all(), "bitmap guard bytes overwritten"
        out["bitmap"] = b[:nb]
    if stats:
        s = st.cpu().tolist()
        assert s[3] == -7, "statistics written past int64[3]"
        out["stats"] = s[:3]
    return plan, out


def window_launch(t, plan, n, pred, lo, cap, probe_ids=None, probe_base=0, stream=None):
    """hj_pair_window_filtered into poisoned outputs of cap + 2 elements (no sync)."""
    ob = torch.full((cap + 2,), SENT_B, dtype=torch.int64, device="cuda")
    op = torch.full((cap + 2,), SENT_P, dtype=torch.int32, device="cuda")
    dw = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t.pair_window_filtered_async(plan.data_ptr(), n, pred, lo, cap, ob.data_ptr(), op.data_ptr(),
                                 stream if stream is not None else torch.cuda.current_stream().cuda_stream,
                                 dw.data_ptr(), None if probe_ids is None else probe_ids.data_ptr(), probe_base)
    return ob, op, dw


def window_finish(out):
    ob, op, dw = out
    torch.cuda.synchronize()
    w, guard = dw.cpu().tolist()
    assert guard == -7, "d_written written past one int64"
    ob, op = ob.cpu().numpy(), op.cpu().numpy()
    assert (ob[w:] == SENT_B).all() and (op[w:] == SENT_P).all(), "written at or beyond index w"
    return ob[:w].view(np.uint64), op[:w].view(np.uint32), w


def window_ok(t, plan, n, pred, fb, fp, lo, cap, **kw):
    ids = kw.get("probe_ids")
    eb, ep, ew = pw.window(fb, fp, lo, cap, None if ids is None else ids.cpu().numpy(), kw.get("probe_base", 0))
    gb, gp, w = window_finish(window_launch(t, plan, n, pred, lo, cap, **kw))
    assert w == ew, (lo, cap, w, ew)
    assert np.array_equal(gb, eb) and np.array_equal(gp, ep), (lo, cap)


def plan_ok(t, keys, n, pred, e, fb, fp, nflags, valid=None, voff=0, before=None):
    """One plan call with every output against `e`, and its whole F against (fb, fp); flags
    start from `before` (default zeros) plus 64 guard bytes that must stay 0."""
    f = torch.zeros(nflags + 64, dtype=torch.uint8, device="cuda")
    if before is not None:
        f[:nflags] = cuda(before)
    plan, got = plan_raw(t, keys, n, pred, valid, voff, flags=f, nflags=nflags)
    assert got["stats"] == [e["matched"], e["pairs"], e["candidates"]], (got["stats"], e["matched"], e["pairs"])
    assert np.array_equal(got["bitmap"], e["bitmap"]), "bitmap differs"
    fh = f.cpu().numpy()
    assert np.array_equal(fh[:nflags], e["flags"]), "flags differ"
    assert not fh[nflags:].any(), "flags written past nflags"
    assert len(fb) == e["pairs"]
    window_ok(t, plan, n, pred, fb, fp, 0, len(fb))
    return plan


# ---- 1. sizes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("key_type", ["int64", "int32"])
def test_sizes(dfp, oracle_mod, key_type):
    """test_gpu_match_filter.test_sizes' set-up: every edge size with keys unaligned to 16
    bytes, the key validity at bit offset 3, nulls in both predicate columns (offsets 3, 13)."""
    dt = np.int64 if key_type == "int64" else np.int32
    rng = np.random.default_rng(17 + (key_type == "int32"))
    NB = 600
    bk = rng.integers(0, 250, NB).astype(dt)
    bv = rng.random(NB) > 0.05
    rb, db = int_col(rng.integers(0, 100, NB), rng.random(NB) < 0.9, 3)
    with dfp.HashTable(1, key_type, 0) as t:
        t.build(cuda(bk), bv)
        for n in mmf.SIZES:
            pk = rng.integers(-10, 270, n).astype(dt)
            pv = rng.random(n) > 0.15
            buf = torch.zeros(n + 3, dtype=torch.int64 if dt is np.int64 else torch.int32, device="cuda")
            keys = buf[1:n + 1]
            keys.copy_(torch.from_numpy(pk))
            assert n == 0 or keys.data_ptr() % 16 == (8 if dt is np.int64 else 4)
            rp, dp = int_col(rng.integers(0, 100, n), rng.random(n) < 0.9, 13)
            ob, op = oracle_mod.inner_join(bk, pk, bv, pv)
            e = ref.expected(ob, op, n, NB, LT, [rb], [rp], NB)
            fb, fp = ref.filtered_pairs(ob, op, LT, [rb], [rp], NB, n)
            if n >= 255:
                assert 0 < e["pairs"] < e["candidates"]
            pred = lt_predicate(db, dp, NB, n)
            plan_ok(t, keys, n, pred, e, fb, fp, NB, cuda(pack_validity(pv, 3)), 3)
            # the wrapper: the same F from all(), the statistics read once
            p = t.pair_plan(keys, cuda(pack_validity(pv, 3)), valid_offset=3, predicate=pred, bitmap=True)
            assert (p.matched, p.total, p.candidates) == (e["matched"], e["pairs"], e["candidates"])
            gb, gp = p.all()
            assert np.array_equal(gb.cpu().numpy().view(np.uint64), fb)
            assert np.array_equal(gp.cpu().numpy().view(np.uint32), fp)
            assert np.array_equal(p.bitmap.cpu().numpy(), e["bitmap"])


# ---- 2. layouts x multiplicities x predicates -----------------------------------------------------

PREDICATES = {
    "lt": [(("b", "i4"), "<", ("p", "i4"))],
    "ne": [(("b", "u2"), "!=", ("p", "u2"))],
    "band": [(("b", "i8"), ">=", ("p", "i2")), (("b", "i1"), "<=", ("p", "i4"))],
    "always": [(("b", "i8big"), "!=", 7)],
    "never": [(("b", "i8big"), "==", 7)],
    "bytes": [(("b", "str"), "<", ("p", "str"))],
    "float": [(("b", "f8"), "<=", ("p", "f4"))],
}
LAYOUTS = ["plain", "packed", "runs", "hashed", "ids", "ids_u31", "wrap_dense"]


def _wrap_built(dfp, t):
    """A table wrapped from a built direct-addressed table's arrays (hj_table_wrap_dense)."""
    piece = t.dense_piece()
    used = torch.zeros(1, dtype=torch.int64, device="cuda")
    t.dense_export(dup_used=used)
    torch.cuda.synchronize()
    refs = torch.empty(piece["nvalues"], dtype=torch.int32, device="cuda")
    dup = torch.empty(max(int(used.item()), 1), dtype=torch.int32, device="cuda")
    t.dense_export(refs=refs, dup=dup)
    torch.cuda.synchronize()
    return dfp.HashTable.wrap_dense(0, "int64", piece["key_min"], refs, dup, piece["packed"])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_and_multiplicities(dfp, oracle_mod, layout):
    """Keys of 1, 2, 9, 10, 15, 16, 64, 65 and 200 build rows in every table layout, under
    predicates of every class; with explicit ids, the id names the row of the build columns
    and ids at or beyond build_rows / nflags fail unread / are not marked."""
    rng = np.random.default_rng(50 + LAYOUTS.index(layout))
    base = {"ids": "packed", "ids_u31": "packed", "wrap_dense": "packed"}.get(layout, layout)
    vals, bk = mmf._mult_build(base, rng)
    NBK, n = len(bk), pft.NP
    assert NBK <= pft.NB
    pk = np.concatenate([vals[rng.integers(0, len(vals), n - 60)], rng.integers(20, 40, 60)]).astype(np.int64)
    rng.shuffle(pk)
    pv = rng.random(n) > 0.05
    ids, build_rows, nflags = None, pft.NB, NBK
    if layout.startswith("ids"):
        ids = np.cumsum(rng.integers(1, 3, NBK)).astype(np.int64)  # ascending, < 2 * NBK < pft.NB
        ids[NBK * 9 // 10:] += pft.NB                              # the last tenth: beyond the build columns
        nflags = int(ids[NBK * 6 // 10])
    ob, op = oracle_mod.inner_join(bk, pk, None, pv)
    idb = ob.astype(np.uint64) if ids is None else ids[ob.astype(np.int64)].astype(np.uint64)
    if ids is not None:
        assert (idb >= build_rows).any() and ((idb >= nflags) & (idb < build_rows)).any() and (idb < nflags).any()
    L = dfp.load()
    old = L.hj_set_build_mode(1 if layout == "hashed" else 0)
    try:
        if layout == "plain":
            t = mmf._wrap_plain(dfp, bk)
        else:
            t = dfp.HashTable(1, "int64", 0)
            t.append(0, cuda(bk), ids=None if ids is None else cuda(ids), ids_u31=layout == "ids_u31")
            t.finish_all()
            assert (t.stats()["buckets"] > 0) == (layout == "hashed")
        tables = [t]
        if layout == "wrap_dense":
            tables.append(_wrap_built(dfp, t))
        try:
            keys, valid = cuda(pk), cuda(pack_validity(pv, 0))
            for name, terms in PREDICATES.items():
                rterms, rb, rp, pred = pft.predicate(terms)
                e = ref.expected(idb, op, n, nflags, rterms, rb, rp, build_rows, pft.NP)
                fb, fp = ref.filtered_pairs(idb, op, rterms, rb, rp, build_rows, pft.NP)
                if name == "never":
                    assert e["pairs"] == 0
                elif name == "always" and ids is None:
                    assert e["pairs"] == e["candidates"] and e["counts"].max() == 200
                elif name != "always":
                    assert 0 < e["pairs"] < e["candidates"], name
                plan_ok(tables[-1], keys, n, pred, e, fb, fp, nflags, valid, 0)
        finally:
            for x in reversed(tables):
                x.close()
    finally:
        L.hj_set_build_mode(old)


# ---- 3. windows -----------------------------------------------------------------------------------

CAPS = [0, 1, 63, 64, 65, 1000, 2048, 2049]
_WIN = {}


def _win_case(dfp, oracle_mod):
    """A key of 200 build rows hit by 300 probe rows among ordinary rows (keys of 1..4 build
    rows), under L.v < R.v: |F| of a few tens of thousands. Made once, left unchanged."""
    if not _WIN:
        rng = np.random.default_rng(71)
        bk = np.concatenate([np.full(200, 7), rng.integers(100, 250, 300)]).astype(np.int64)
        rng.shuffle(bk)
        NB, n = len(bk), 2500
        pk = np.concatenate([np.full(300, 7), rng.integers(100, 300, n - 300)]).astype(np.int64)
        rng.shuffle(pk)
        rb, db = int_col(rng.integers(0, 100, NB), rng.random(NB) < 0.95, 3)
        rp, dp = int_col(rng.integers(0, 100, n), rng.random(n) < 0.95, 13)
        ob, op = oracle_mod.inner_join(bk, pk)
        fb, fp = ref.filtered_pairs(ob, op, LT, [rb], [rp], NB, n)
        e = ref.expected(ob, op, n, NB, LT, [rb], [rp], NB)
        t = dfp.HashTable(1, "int64", 0)
        t.build(cuda(bk))
        pred = lt_predicate(db, dp, NB, n)
        keys = cuda(pk)
        plan, got = plan_raw(t, keys, n, pred)
        assert got["stats"] == [e["matched"], e["pairs"], e["candidates"]]
        _WIN.update(t=t, n=n, pk=pk, pred=pred, plan=plan, fb=fb, fp=fp, e=e, keys=keys)
    return _WIN


def _los(c):
    """Window starts: 0, inside a lane-walked row's passing pairs, inside a later wave round
    of the 200-row key, the first rank of the second 1024-row block, |F| - 1, |F|, |F| + 5."""
    fp, pk, counts, T = c["fp"], c["pk"], c["e"]["counts"].astype(np.int64), len(c["fp"])
    start = np.concatenate([[0], np.cumsum(counts)])
    small = int(np.flatnonzero((pk != 7) & (counts >= 2))[0])
    hot = int(np.flatnonzero((pk == 7) & (counts >= 80))[3])
    edge = int(np.searchsorted(fp, 1024))
    assert 20_000 < T < 100_000 and edge == start[1024] and 0 < edge < T
    return [0, int(start[small]) + 1, int(start[hot]) + 70, edge, T - 1, T, T + 5]


def test_windows(dfp, oracle_mod):
    c = _win_case(dfp, oracle_mod)
    for lo in _los(c):
        for cap in CAPS:
            window_ok(c["t"], c["plan"], c["n"], c["pred"], c["fb"], c["fp"], lo, cap)


@pytest.mark.parametrize("step", [1, 97, 4096])
def test_windows_cover_f(dfp, oracle_mod, step):
    """windows(N) concatenated is F, on the plan of tens of thousands of passing pairs."""
    c = _win_case(dfp, oracle_mod)
    fb, fp = c["fb"], c["fp"]
    p = c["t"].pair_plan(c["keys"], predicate=c["pred"])
    assert p.total == len(fb)
    parts = list(p.windows(step))
    assert len(parts) == -(-len(fb) // step) and all(0 < b.numel() <= step for b, _ in parts)
    gb = torch.cat([b for b, _ in parts]).cpu().numpy().view(np.uint64)
    gp = torch.cat([q for _, q in parts]).cpu().numpy().view(np.uint32)
    assert np.array_equal(gb, fb) and np.array_equal(gp, fp)


def test_two_windows_on_two_streams_and_twice_the_same(dfp, oracle_mod):
    c = _win_case(dfp, oracle_mod)
    T = len(c["fb"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = window_launch(c["t"], c["plan"], c["n"], c["pred"], 0, T // 2 + 11, stream=s1.cuda_stream)
    b = window_launch(c["t"], c["plan"], c["n"], c["pred"], T // 2 - 7, T, stream=s2.cuda_stream)
    ga, gb = window_finish(a), window_finish(b)
    for (lo, cap), got in (((0, T // 2 + 11), ga), ((T // 2 - 7, T), gb)):
        eb, ep, ew = pw.window(c["fb"], c["fp"], lo, cap)
        assert got[2] == ew and np.array_equal(got[0], eb) and np.array_equal(got[1], ep)
    # the plan is read-only: the same window again gives identical bytes
    again = window_finish(window_launch(c["t"], c["plan"], c["n"], c["pred"], 0, T // 2 + 11))
    assert again[2] == ga[2] and again[0].tobytes() == ga[0].tobytes() and again[1].tobytes() == ga[1].tobytes()


def test_probe_ids_and_probe_base(dfp, oracle_mod):
    from datafusion_parallelism_amd import HjError, _lib

    c = _win_case(dfp, oracle_mod)
    T, n = len(c["fb"]), c["n"]
    rng = np.random.default_rng(5)
    ids = cuda(rng.integers(-2**31, 2**31, n).astype(np.int32))
    for lo, cap in ((0, T), (_los(c)[2], 2049), (T - 1, 5)):
        window_ok(c["t"], c["plan"], n, c["pred"], c["fb"], c["fp"], lo, cap, probe_ids=ids)
        window_ok(c["t"], c["plan"], n, c["pred"], c["fb"], c["fp"], lo, cap, probe_base=2**32 - n)
    L = dfp.load()
    x = torch.zeros(8, dtype=torch.int64, device="cuda")
    st = L.hj_pair_window_filtered(c["t"]._h, c["plan"].data_ptr(), n, c["pred"].struct, ids.data_ptr(), 5, 0, 4,
                                   x.data_ptr(), x.data_ptr(), None, None)
    assert st == _lib.HJ_ERR_INVALID and b"exclusive" in L.hj_last_error()
    with pytest.raises(ValueError):
        c["t"].pair_window_filtered_async(c["plan"].data_ptr(), n, c["pred"], 0, 4, x.data_ptr(), x.data_ptr(),
                                          probe_ids_ptr=ids.data_ptr(), probe_base=5)
    with pytest.raises(HjError, match="aligned"):
        c["t"].pair_window_filtered_async(c["plan"].data_ptr(), n, c["pred"], 0, 4, x.data_ptr(), x.data_ptr() + 2)
    # the wrapper's plan carries ids / a base to its windows
    p = c["t"].pair_plan(c["keys"], probe_ids=ids, predicate=c["pred"])
    gb, gp = p.window(100, 3000)
    eb, ep, _ = pw.window(c["fb"], c["fp"], 100, 3000, ids.cpu().numpy())
    assert np.array_equal(gb.cpu().numpy().view(np.uint64), eb) and np.array_equal(gp.cpu().numpy().view(np.uint32), ep)


# ---- 4. accumulation ------------------------------------------------------------------------------

def test_flags_accumulate_over_two_batches(dfp, oracle_mod):
    rng = np.random.default_rng(33)
    reps = rng.integers(1, 120, 60)
    bk = np.repeat(np.arange(60, dtype=np.int64), reps)
    rng.shuffle(bk)
    NB = len(bk)
    rb, db = int_col(rng.integers(0, 100, NB), None)
    want = (rng.random(NB) < 0.2).astype(np.uint8)
    with dfp.HashTable(1, "int64", 0) as t:
        t.build(cuda(bk))
        flags = cuda(want)
        for lo, hi in ((0, 40), (25, 60)):
            n = 700
            pk = rng.integers(lo, hi, n).astype(np.int64)
            rp, dp = int_col(rng.integers(0, 60, n), None)
            ob, op = oracle_mod.inner_join(bk, pk)
            e = ref.expected(ob, op, n, NB, LT, [rb], [rp], NB, before=want)
            fb, fp = ref.filtered_pairs(ob, op, LT, [rb], [rp], NB, n)
            p = t.pair_plan(cuda(pk), predicate=lt_predicate(db, dp, NB, n), build_flags=flags)
            want = e["flags"]
            assert p.bitmap is None and (p.matched, p.total, p.candidates) == (e["matched"], len(fb), e["candidates"])
            assert np.array_equal(flags.cpu().numpy(), want)
            gb, gp = p.all()
            assert np.array_equal(gb.cpu().numpy().view(np.uint64), fb)
            assert np.array_equal(gp.cpu().numpy().view(np.uint32), fp)
        assert not want.all()


# ---- 5. errors ------------------------------------------------------------------------------------

def test_errors_and_n_zero(dfp):
    from datafusion_parallelism_amd import HjError, _lib

    _, db = int_col(np.zeros(1000, np.int64), None)
    _, dp = int_col(np.zeros(100, np.int64), None)
    keys = torch.arange(100, dtype=torch.int64, device="cuda")
    with dfp.HashTable(1, "int64", devices=[0, 0]) as t:
        t.append(0, torch.arange(1000, dtype=torch.int64, device="cuda"))
        t.finish_all()
        with pytest.raises(HjError, match="multi-GPU") as e:
            t.pair_plan(keys, predicate=lt_predicate(db, dp, 1000, 100))
        assert e.value.status == _lib.HJ_ERR_INVALID
        assert t._L.hj_pair_plan_filtered_bytes(t._h, 100) == -1
    with dfp.HashTable(1, "int64", 0) as t:
        t.build(torch.arange(1000, dtype=torch.int64, device="cuda"))
        short = lt_predicate(db, dp, 1000, 50)
        with pytest.raises(HjError, match="probe_rows") as e:
            plan_raw(t, keys, 100, short)
        assert e.value.status == _lib.HJ_ERR_INVALID
        pred = lt_predicate(db, dp, 1000, 100)
        plan, got = plan_raw(t, keys, 100, pred)
        with pytest.raises(HjError, match="probe_rows"):
            window_launch(t, plan, 100, short, 0, 4)
        # n == 0 still writes d_stats and d_written
        plan, got = plan_raw(t, keys, 0, pred)
        assert got["stats"] == [0, 0, 0] and len(got["bitmap"]) == 0
        assert window_finish(window_launch(t, plan, 0, pred, 0, 16))[2] == 0
        p = t.pair_plan(keys[:0], predicate=pred, bitmap=True)
        assert (p.matched, p.total, p.candidates) == (0, 0, 0) and p.all()[0].numel() == 0 and list(p.windows(5)) == []


def test_argument_checks_on_a_built_table(dfp):
    """With a real table the pointer and range checks answer themselves, each with its message."""
    from datafusion_parallelism_amd import _lib

    L = dfp.load()
    INV = _lib.HJ_ERR_INVALID
    _, db = int_col(np.arange(1000, dtype=np.int64), None)
    _, dp = int_col(np.where(np.arange(100) % 2 == 1, np.arange(100) + 1, 0), None)  # L.v < R.v: the odd rows pass
    keys = torch.arange(100, dtype=torch.int64, device="cuda")
    x = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = x.data_ptr()
    with dfp.HashTable(1, "int64", 0) as t:
        t.build(torch.arange(1000, dtype=torch.int64, device="cuda"))
        pred = lt_predicate(db, dp, 1000, 100).struct
        assert t.pair_plan_filtered_bytes(100) <= x.numel() * 8

        def plan(plan=p, bm=None, flags=None, nflags=0, st=None, n=100, k=keys.data_ptr()):
            return L.hj_pair_plan_filtered(t._h, k, None, 0, n, pred, plan, bm, flags, nflags, st, None)

        def window(plan=p, n=100, ids=None, base=0, lo=0, cap=4, ob=p + 8192, op=p + 16384, dw=None):
            return L.hj_pair_window_filtered(t._h, plan, n, pred, ids, base, lo, cap, ob, op, dw, None)

        def refused(st, word):
            assert st == INV and word in L.hj_last_error(), (st, word, L.hj_last_error())

        refused(plan(plan=None), b"null plan")
        refused(plan(plan=p + 4), b"aligned")
        refused(plan(bm=p + 24580), b"aligned")
        refused(plan(st=p + 24580), b"aligned")
        refused(plan(nflags=5), b"nflags")
        refused(plan(nflags=-1, flags=p), b"nflags")
        refused(plan(k=None), b"null keys")
        refused(plan(n=2**32), b"2^32")
        assert plan(st=p + 24576) == _lib.HJ_OK
        torch.cuda.synchronize()
        assert x[3072:3075].tolist() == [50, 50, 100]  # unique keys: one candidate per row, the odd rows' pass
        refused(window(plan=None), b"null plan")
        refused(window(plan=p + 4), b"aligned")
        refused(window(dw=p + 24580), b"aligned")
        refused(window(ob=p + 8196), b"aligned")
        refused(window(op=p + 16386), b"aligned")
        refused(window(ob=None), b"null output")
        refused(window(op=None), b"null output")
        refused(window(lo=-1), b"pair_lo")
        refused(window(cap=-1), b"capacity")
        refused(window(cap=2**42 + 1), b"2^42")
        refused(window(n=2**32), b"2^32")
        refused(window(base=2**32 - 4), b"2^32")
        refused(window(ids=p, base=5), b"exclusive")
        assert window(cap=0, ob=None, op=None, dw=p + 24600) == _lib.HJ_OK  # every output optional at capacity 0
        assert window(dw=p + 24600) == _lib.HJ_OK
        torch.cuda.synchronize()
        assert int(x[3075]) == 4 and x[1024:1028].tolist() == [1, 3, 5, 7]
        assert x.view(torch.int32)[4096:4100].tolist() == [1, 3, 5, 7]
