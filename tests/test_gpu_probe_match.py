"""GPU: the match probe (hj_probe_match), the bitmap select (hj_select_bitmap) and the
operator's match path (match_probe=True). Expected values come from the oracle's inner
pairs through probe_match_ref.py; where pairs exist, hj_mark_rows over the GPU's own pairs
must give the same build flags."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import probe_match_ref as ref
from key_filter_ref import pack_validity

pytestmark = pytest.mark.gpu

EDGE_N = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
I64_MIN, I64_MAX = -(2**63), 2**63 - 1


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def match_raw(t, keys: torch.Tensor, n: int, valid: torch.Tensor | None = None, voff: int = 0,
              flags: torch.Tensor | None = None, nflags: int = 0, counts: bool = True):
    """hj_probe_match on raw pointers into poisoned outputs: the bitmap is pre-filled with
    0xFF and followed by 8 guard bytes, the counts and statistics hold garbage."""
    nb = ref.bitmap_bytes(n)
    bm = torch.full((nb + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda") if counts else None
    st = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(t.match_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    t.probe_match_async(keys.data_ptr(), n, bm.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream,
                        None if valid is None else valid.data_ptr(), voff, None if cnt is None else cnt.data_ptr(),
                        None if flags is None else flags.data_ptr(), nflags, st.data_ptr())
    torch.cuda.synchronize()
    bm = bm.cpu().numpy()
    assert (bm[nb:] == 0xFF).all(), "bitmap guard bytes overwritten"
    out = {"bitmap": bm[:nb], "matched": int(st[0].item()), "pairs": int(st[1].item())}
    if counts:
        c = cnt.cpu().numpy()
        assert (c[n:] == -1).all(), "counts written past n"
        out["counts"] = c[:n].view(np.uint32)
    return out


def check_outputs(got, e):
    assert np.array_equal(got["bitmap"], e["bitmap"]), "bitmap differs"
    if "counts" in got:
        assert np.array_equal(got["counts"], e["counts"]), "counts differ"
    assert (got["matched"], got["pairs"]) == (e["matched"], e["pairs"])


def flags_of_gpu_pairs(t, keys, valid, voff, nflags, before=None):
    """hj_mark_rows over the pair probe's own build indices."""
    from datafusion_parallelism_amd.columns import mark_rows

    b, _ = t.probe(keys, valid, device_output=True, valid_offset=voff)
    f = torch.zeros(max(nflags, 1), dtype=torch.uint8, device="cuda") if before is None else cuda(before)
    return mark_rows(b, nflags, f).cpu().numpy()[:nflags]


# ---- 1. word and tile edges ---------------------------------------------------------

@pytest.mark.parametrize("key_type", ["int64", "int32"])
@pytest.mark.parametrize("voff", [0, 3, 67])
def test_word_and_tile_edges(dfp, oracle_mod, key_type, voff):
    dt = np.int64 if key_type == "int64" else np.int32
    rng = np.random.default_rng(voff + (key_type == "int32"))
    bk = rng.integers(0, 700, 1000).astype(dt)
    bv = rng.random(len(bk)) > 0.05
    with dfp.HashTable(1, key_type, 0) as t:
        t.build(cuda(bk), bv)
        for n in EDGE_N:
            pk = rng.integers(-20, 760, n).astype(dt)
            pv = rng.random(n) > 0.2
            # element 1 of a fresh tensor: 8- but not 16-byte aligned (int64), 4- but not 16- (int32)
            buf = torch.zeros(n + 3, dtype=torch.int64 if dt is np.int64 else torch.int32, device="cuda")
            keys = buf[1:n + 1]
            keys.copy_(torch.from_numpy(pk))
            assert n == 0 or keys.data_ptr() % 16 == (8 if dt is np.int64 else 4)
            valid = cuda(pack_validity(pv, voff))
            flags = torch.zeros(len(bk) + 64, dtype=torch.uint8, device="cuda")
            got = match_raw(t, keys, n, valid, voff, flags, len(bk))
            ob, op = oracle_mod.inner_join(bk, pk, bv, pv)
            e = ref.expected(ob, op, n, len(bk))
            check_outputs(got, e)
            f = flags.cpu().numpy()
            assert np.array_equal(f[:len(bk)], e["flags"]) and not f[len(bk):].any()
            if n:
                assert np.array_equal(flags_of_gpu_pairs(t, keys, valid, voff, len(bk)), e["flags"])
                # the bitmap is a validity bitmap for any probe: the same pairs come out
                b2, p2 = t.probe(keys, cuda(got["bitmap"]), device_output=True)
                assert np.array_equal(b2.cpu().numpy().astype(np.uint64), ob)
                assert np.array_equal(p2.cpu().numpy().astype(np.uint32), op)


def test_optional_outputs_and_errors(dfp, oracle_mod):
    """Every output is optional; d_stats is written whichever others are null; a misaligned
    workspace or bitmap is HJ_ERR_INVALID."""
    from datafusion_parallelism_amd import HjError, _lib

    rng = np.random.default_rng(5)
    bk = rng.integers(0, 500, 800).astype(np.int64)
    pk = rng.integers(0, 700, 1000).astype(np.int64)
    ob, op = oracle_mod.inner_join(bk, pk)
    e = ref.expected(ob, op, len(pk), len(bk))
    with dfp.HashTable(1, "int64", 0) as t:
        t.build(cuda(bk))
        keys = cuda(pk)
        ws = torch.empty(t.match_workspace_bytes(len(pk)) + 8, dtype=torch.uint8, device="cuda")
        st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        t.probe_match_async(keys.data_ptr(), len(pk), None, ws.data_ptr(), s, d_stats_ptr=st.data_ptr())
        assert st.tolist() == [e["matched"], e["pairs"]]
        flags = torch.zeros(len(bk), dtype=torch.uint8, device="cuda")
        t.probe_match_async(keys.data_ptr(), len(pk), None, ws.data_ptr(), s, build_flags_ptr=flags.data_ptr(),
                            nflags=len(bk))  # no statistics, no bitmap
        assert np.array_equal(flags.cpu().numpy(), e["flags"])
        bm = torch.empty(ref.bitmap_bytes(len(pk)) + 8, dtype=torch.uint8, device="cuda")
        for bad in [dict(bitmap_ptr=bm.data_ptr() + 4, workspace_ptr=ws.data_ptr()),
                    dict(bitmap_ptr=bm.data_ptr(), workspace_ptr=ws.data_ptr() + 4),
                    dict(bitmap_ptr=bm.data_ptr(), workspace_ptr=0)]:
            with pytest.raises(HjError) as err:
                t.probe_match_async(keys.data_ptr(), len(pk), stream=s, **bad)
            assert err.value.status == _lib.HJ_ERR_INVALID
        r = t.probe_match(keys, counts=True)
        assert r.matched == e["matched"] and r.pairs == e["pairs"]
        assert np.array_equal(r.bitmap.cpu().numpy(), e["bitmap"])
        assert np.array_equal(r.counts.cpu().numpy().view(np.uint32), e["counts"])
        assert t.probe_match(keys).counts is None


# ---- 2. direct-addressed refs of every kind (+ 8. wrapped tables) -----------------------

def _run_keys(rng, nkeys=3000, maxrun=12):
    """The keys of test_gpu_parity.py's _run_keys: sorted build keys in runs of 1..maxrun
    consecutive rows (run refs for 2..9 rows, packed counts and header counts beyond), a few
    split keys, and probe keys over and beyond the build range."""
    lens = rng.integers(1, maxrun + 1, nkeys)
    bk = np.repeat(np.arange(nkeys, dtype=np.int64) * 3, lens)
    bk = np.concatenate([bk, bk[:: max(1, len(bk) // 50)]])
    pk = rng.integers(-5, nkeys * 3 + 5, 40000).astype(np.int64)
    return bk, pk


@pytest.mark.parametrize("parts", [1, 2])
def test_direct_addressed_refs(dfp, oracle_mod, parts):
    rng = np.random.default_rng(61 + parts)
    bk, pk = _run_keys(rng)
    n = len(bk)
    bv = None if parts == 1 else rng.random(n) > 0.05
    cut = [0, n] if parts == 1 else [0, n // 3, n]
    with dfp.HashTable(parts, "int64", 0) as t:
        for p in range(parts):
            t.append(p, cuda(bk[cut[p]:cut[p + 1]]), None if bv is None else bv[cut[p]:cut[p + 1]])
        t.finish_all()
        st = t.stats()
        assert st["buckets"] == 0 and st["max_key_rows"] >= 12
        keys = cuda(pk)
        flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
        got = match_raw(t, keys, len(pk), flags=flags, nflags=n)
        ob, op = oracle_mod.inner_join(bk, pk, bv, None)
        e = ref.expected(ob, op, len(pk), n)
        check_outputs(got, e)
        assert np.array_equal(flags.cpu().numpy(), e["flags"])
        assert np.array_equal(flags_of_gpu_pairs(t, keys, None, 0, n), e["flags"])
        if parts == 1:
            # 8. a table wrapped from this one's arrays (hj_table_wrap_dense) answers the same
            piece = t.dense_piece()
            used = torch.zeros(1, dtype=torch.int64, device="cuda")
            t.dense_export(dup_used=used)
            torch.cuda.synchronize()
            refs = torch.empty(piece["nvalues"], dtype=torch.int32, device="cuda")
            dup = torch.empty(max(int(used.item()), 1), dtype=torch.int32, device="cuda")
            t.dense_export(refs=refs, dup=dup)
            torch.cuda.synchronize()
            with dfp.HashTable.wrap_dense(0, "int64", piece["key_min"], refs, dup, piece["packed"]) as w:
                wflags = torch.zeros(n, dtype=torch.uint8, device="cuda")
                wgot = match_raw(w, keys, len(pk), flags=wflags, nflags=n)
                check_outputs(wgot, e)
                assert np.array_equal(wflags.cpu().numpy(), e["flags"])


# ---- 3. hashed table at a high load factor ------------------------------------------------

def test_hashed_high_load(dfp, oracle_mod, monkeypatch):
    """60,000 random 64-bit keys, a quarter duplicated 2..40 times, one key of 90 rows (its
    count in the segment header), keys 0, -1, INT64_MIN, INT64_MAX, load factor 0.8 (displaced
    keys: a 5-slot bucket at mean 4 keys overflows with probability ~ 0.21)."""
    monkeypatch.setenv("DFP_HJ_LOAD_FACTOR", "0.8")
    L = dfp.load()
    old = L.hj_set_build_mode(1)
    try:
        rng = np.random.default_rng(80)
        distinct = rng.integers(I64_MIN, I64_MAX, 60_000, dtype=np.int64)
        distinct[:4] = [0, -1, I64_MIN, I64_MAX]
        reps = np.ones(len(distinct), dtype=np.int64)
        q = len(distinct) // 4
        reps[4:4 + q] = rng.integers(2, 41, q)
        reps[0] = 3       # key 0 (the side bucket) duplicated
        reps[5] = 90      # count in the segment header
        bk = np.repeat(distinct, reps)
        rng.shuffle(bk)
        pk = np.concatenate([distinct[rng.integers(0, len(distinct), 50_000)],
                             rng.integers(I64_MIN, I64_MAX, 50_000, dtype=np.int64)])
        rng.shuffle(pk)
        pk[:6] = [0, -1, I64_MIN, I64_MAX, distinct[5], 0]
        n = len(bk)
        with dfp.HashTable(1, "int64", 0) as t:
            t.build(cuda(bk))
            assert t.stats()["buckets"] > 0
            keys = cuda(pk)
            flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
            got = match_raw(t, keys, len(pk), flags=flags, nflags=n)
            ob, op = oracle_mod.inner_join(bk, pk)
            e = ref.expected(ob, op, len(pk), n)
            assert e["counts"].max() == 90
            check_outputs(got, e)
            assert np.array_equal(flags.cpu().numpy(), e["flags"])
            assert np.array_equal(flags_of_gpu_pairs(t, keys, None, 0, n), e["flags"])
    finally:
        L.hj_set_build_mode(old)


# ---- 4. explicit build ids ---------------------------------------------------------------

@pytest.mark.parametrize("ids_u31", [False, True])
@pytest.mark.parametrize("dups", [1, 300, 5000])
def test_explicit_build_ids(dfp, oracle_mod, ids_u31, dups):
    """The inputs of test_gpu_parity.py::test_explicit_build_ids: flags are indexed by id; nflags
    cuts off the top tenth of the ids and nothing is written past it."""
    rng = np.random.default_rng(dups + ids_u31)
    bk = np.concatenate([rng.integers(0, 3000, 20000), np.full(dups, 77)]).astype(np.int64)
    rng.shuffle(bk)
    bv = rng.random(len(bk)) > 0.05
    ids = np.cumsum(rng.integers(1, 50, len(bk))).astype(np.int64) + 10**6
    pk = np.concatenate([rng.integers(0, 4000, 30000), [77, 77]]).astype(np.int64)
    nflags = int(ids[len(ids) * 9 // 10])
    with dfp.HashTable(2, "int64", 0) as t:
        h = len(bk) // 2
        t.append(0, cuda(bk[:h]), bv[:h], ids=cuda(ids[:h]), ids_u31=ids_u31)
        t.append(1, cuda(bk[h:]), bv[h:], ids=cuda(ids[h:]), ids_u31=ids_u31)
        t.finish_all()
        keys = cuda(pk)
        flags = torch.zeros(nflags + 64, dtype=torch.uint8, device="cuda")
        got = match_raw(t, keys, len(pk), flags=flags, nflags=nflags)
        ob, op = oracle_mod.inner_join(bk, pk, bv, None)
        idb = ids[ob.astype(np.int64)].astype(np.uint64)
        assert (idb >= nflags).any() and (idb < nflags).any()
        e = ref.expected(idb, op, len(pk), nflags)
        check_outputs(got, e)
        f = flags.cpu().numpy()
        assert np.array_equal(f[:nflags], e["flags"])
        assert not f[nflags:].any(), "flags written past nflags"
        assert np.array_equal(flags_of_gpu_pairs(t, keys, None, 0, nflags), e["flags"])


# ---- 5. accumulation over batches into pre-seeded flags ------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_flags_accumulate(dfp, oracle_mod, layout):
    """Two probe batches into one build_flags that already marks some rows of duplicated
    keys: the result is seed | marks(batch 1) | marks(batch 2) - the flags cannot serve as
    the per-key claim."""
    L = dfp.load()
    old = L.hj_set_build_mode(layout)
    try:
        rng = np.random.default_rng(50 + layout)
        # keys 0..399 with 1..150 rows each: singles, short keys, claimed keys, wave-walked keys
        reps = rng.integers(1, 151, 400)
        bk = np.repeat(np.arange(400, dtype=np.int64) * (1 if layout == 0 else 0x9E3779B97F4A7), reps)
        rng.shuffle(bk)
        n = len(bk)
        seed = (rng.random(n) < 0.3).astype(np.uint8)
        vals = np.unique(bk)
        # (the last 50 keys are never probed: their rows keep the seed)
        batches = [np.concatenate([rng.choice(vals[:200], 3000), rng.integers(-50, 0, 100)]).astype(np.int64),
                   np.concatenate([rng.choice(vals[150:350], 3000), rng.integers(-50, 0, 100)]).astype(np.int64)]
        with dfp.HashTable(1, "int64", 0) as t:
            t.build(cuda(bk))
            assert (t.stats()["buckets"] > 0) == (layout == 1)
            flags = cuda(seed)
            want = seed
            for pk in batches:
                r = t.probe_match(cuda(pk), build_flags=flags)
                ob, op = oracle_mod.inner_join(bk, pk)
                want = ref.expected_flags(ob, n, want)
                assert (r.matched, r.pairs) == ref.expected_stats(op)
                assert np.array_equal(flags.cpu().numpy(), want)
            assert want.sum() > seed.sum() and not want.all()
    finally:
        L.hj_set_build_mode(old)


# ---- 6. hot key --------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_hot_key(dfp, layout):
    """200,000 build rows of one key probed by 200,000 rows of it: 4 * 10^10 pairs that no
    buffer holds, decided by 401,000 flags. Expected values in closed form (the oracle and
    the pair probe cannot run this). Marking a hot key once per probe row would be
    4 * 10^10 byte stores."""
    L = dfp.load()
    old = L.hj_set_build_mode(layout)
    try:
        rng = np.random.default_rng(6)
        H, c, m = 7, 200_000, 200_000
        bk = np.concatenate([np.full(c, H), np.arange(1000, 2000)]).astype(np.int64)
        rng.shuffle(bk)
        pk = np.concatenate([np.full(m, H), np.arange(1000, 1500), np.arange(5000, 5500), np.full(300, H)])
        pv = np.concatenate([np.ones(m + 1000, dtype=bool), np.zeros(300, dtype=bool)])
        order = rng.permutation(len(pk))
        pk, pv = pk[order].astype(np.int64), pv[order]
        with dfp.HashTable(1, "int64", 0) as t:
            t.build(cuda(bk))
            assert (t.stats()["buckets"] > 0) == (layout == 1)
            flags = torch.zeros(len(bk), dtype=torch.uint8, device="cuda")
            r = t.probe_match(cuda(pk), pv, counts=True, build_flags=flags)
            assert r.pairs == c * m + 500 == 40_000_000_500
            assert r.matched == m + 500
            want_counts = np.where(pv & (pk == H), c, np.where(pv & (pk >= 1000) & (pk < 1500), 1, 0))
            assert np.array_equal(r.counts.cpu().numpy().view(np.uint32), want_counts.astype(np.uint32))
            assert np.array_equal(r.bitmap.cpu().numpy(), ref.expected_bitmap(np.flatnonzero(want_counts), len(pk)))
            want_flags = ((bk == H) | ((bk >= 1000) & (bk < 1500))).astype(np.uint8)
            assert np.array_equal(flags.cpu().numpy(), want_flags) and want_flags.sum() == c + 500
    finally:
        L.hj_set_build_mode(old)


# ---- 7. select_bitmap -----------------------------------------------------------------------

@pytest.mark.parametrize("bit_offset", [0, 5, 64, 69])
def test_select_bitmap(dfp, bit_offset):
    from datafusion_parallelism_amd.columns import select_bitmap

    rng = np.random.default_rng(bit_offset)
    for n in EDGE_N + [40_000]:
        for fill in ("random", "zeros", "ones"):
            nbits = bit_offset + n
            bits = {"random": rng.random(nbits) < 0.4, "zeros": np.zeros(nbits, bool), "ones": np.ones(nbits, bool)}[fill]
            packed = np.packbits(bits, bitorder="little")
            # one byte into a fresh tensor: the bitmap need not be aligned either
            buf = torch.zeros(len(packed) + 9, dtype=torch.uint8, device="cuda")
            bm = buf[1:1 + len(packed)]
            bm.copy_(torch.from_numpy(packed))
            buf[1 + len(packed):] = 0xFF if fill == "zeros" else 0  # bytes past the bitmap are not rows
            for want in (0, 1):
                got = select_bitmap(bm, n, want, base=1000, bit_offset=bit_offset).cpu().numpy().view(np.uint32)
                exp = np.flatnonzero(bits[bit_offset:] == bool(want)) + 1000
                assert np.array_equal(got, exp), (n, fill, want)
                assert np.array_equal(got, ref.select_rows(packed, n, want, 1000, bit_offset))
    big = select_bitmap(cuda(np.full(8, 0xFF, np.uint8)), 64, 1, base=2**32 - 64).cpu().numpy().view(np.uint32)
    assert big[0] == 2**32 - 64 and big[-1] == 2**32 - 1


# ---- 9. multi-GPU tables are refused ---------------------------------------------------------

def test_multi_table_refused(dfp):
    from datafusion_parallelism_amd import HjError, _lib

    with dfp.HashTable(1, "int64", devices=[0, 0]) as t:
        t.append(0, torch.arange(1000, dtype=torch.int64, device="cuda"))
        t.finish_all()
        with pytest.raises(HjError, match="multi-GPU") as e:
            t.probe_match(torch.arange(100, dtype=torch.int64, device="cuda"))
        assert e.value.status == _lib.HJ_ERR_INVALID


# ---- 10. operator -----------------------------------------------------------------------------

SEMI_ANTI = ["leftsemi", "leftanti", "rightsemi", "rightanti"]


def rb(**cols):
    return pa.RecordBatch.from_pydict(cols)


def join(left_parts, right_parts, jt, on=(("id", "id"),), match_probe=False, flt=None, schema=None, **kw):
    from datafusion_parallelism_amd.operator import ParallelHashJoin

    out = ParallelHashJoin(left_parts, right_parts, on=list(on), join_type=jt, filter=flt, right_schema=schema,
                           match_probe=match_probe, **kw).collect()
    return pa.Table.from_batches(out) if out else None


def rows_of(tbl):
    return [] if tbl is None else [tuple(c[r].as_py() for c in tbl.columns) for r in range(tbl.num_rows)]


KATS = {  # the reference's KAT inputs (tests/test_gpu_join_types.py): left ids, right ids
    "leftsemi": ([1, 2, None], [1, 1, None]),       # src/lib.rs:324-371
    "leftanti": ([1, 2, None], [1, 1, None]),       # src/lib.rs:389-436
    "rightsemi": ([1, 2, None], [1, 2, 3, None, 2]),
    "rightanti": ([1, 2, None], [1, 2, 3, None]),   # src/lib.rs:512-575
}
KAT_ROWS = {"leftsemi": [(1, "left")], "leftanti": [(2, "left"), (None, "left")],
            "rightsemi": [(1, "right"), (2, "right"), (2, "right")], "rightanti": [(3, "right"), (None, "right")]}


@pytest.mark.parametrize("jt", SEMI_ANTI)
def test_operator_kats(dfp, jt):
    lid, rid = KATS[jt]
    left = rb(id=pa.array(lid, pa.int32()), value=["left"] * len(lid))
    right = rb(id=pa.array(rid, pa.int32()), value=["right"] * len(rid))
    got = join([[left]], [[right]], jt, match_probe=True, schema=right.schema)
    base = join([[left]], [[right]], jt, match_probe=False, schema=right.schema)
    assert got.equals(base)
    assert rows_of(got) == KAT_ROWS[jt]


def _random_sides(rng, nb=3000, np_=5000):
    bk, pk = rng.integers(0, 2500, nb), rng.integers(0, 4000, np_)
    bnull, pnull = rng.random(nb) < 0.05, rng.random(np_) < 0.05
    left = pa.Table.from_pydict({"id": pa.array(bk, mask=bnull), "bid": np.arange(nb), "g": rng.integers(0, 3, nb)})
    right = pa.Table.from_pydict({"id": pa.array(pk, mask=pnull), "pid": np.arange(np_), "g": rng.integers(0, 3, np_)})
    return left, right


@pytest.mark.parametrize("jt", SEMI_ANTI)
def test_operator_random(dfp, jt):
    """Nulls and duplicates; one partition (exact batch equality) and two partitions of two
    probe batches each (sorted rows); a `valid` bitmap at a non-zero offset (sliced batches)."""
    left, right = _random_sides(np.random.default_rng(7))
    one_l, one_r = [left.to_batches()], [right.slice(3).to_batches(max_chunksize=2600)]
    got = join(one_l, one_r, jt, match_probe=True, schema=right.schema)
    base = join(one_l, one_r, jt, match_probe=False, schema=right.schema)
    assert got.num_rows > 0 and got.equals(base)
    lb, rbs = left.to_batches(max_chunksize=800), right.to_batches(max_chunksize=1250)
    two_l, two_r = [lb[0::2], lb[1::2]], [rbs[0::2], rbs[1::2]]
    assert all(len(p) == 2 for p in two_r)
    got = join(two_l, two_r, jt, match_probe=True, schema=right.schema)
    base = join(two_l, two_r, jt, match_probe=False, schema=right.schema)
    assert sorted(rows_of(got), key=repr) == sorted(rows_of(base), key=repr) and got.num_rows > 0


@pytest.mark.parametrize("jt", SEMI_ANTI)
def test_operator_fallbacks(dfp, jt):
    """A JoinFilter, a two-column key or a multi-GPU table: match_probe=True silently takes the
    pair path and gives the same answer. With prefilter=True too, the match path ignores the
    filter."""
    from datafusion_parallelism_amd.operator import JoinFilter

    left, right = _random_sides(np.random.default_rng(9), 1500, 2500)
    l, r = [left.to_batches()], [right.to_batches()]
    flt = JoinFilter(lambda a, b: pc.less(a.column("bid"), b.column("pid")), ["bid"], ["pid"])
    variants = [dict(flt=flt), dict(on=(("id", "id"), ("g", "g"))), dict(devices=[0, 0]), dict(prefilter=True)]
    for kw in variants:
        got = join(l, r, jt, match_probe=True, schema=right.schema, **kw)
        base = join(l, r, jt, match_probe=False, schema=right.schema, **kw)
        assert got.equals(base) and got.num_rows > 0, kw
