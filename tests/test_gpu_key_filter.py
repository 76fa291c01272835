"""GPU: the device key filter (include/hj.h "key filter", csrc/hj_filter.hip).

* The filter's words after add, the test bitmap and count and the select keys and ids,
  bit for bit against the numpy restatement of the two layouts (key_filter_ref.py).
* HashTable.probe(prefilter=...), ParallelHashJoin(prefilter=True) and tpch.q3 with
  DFP_TPCH_PREFILTER=1 return what they return without the filter, in the same order.
"""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

from key_filter_ref import RefFilter, pack_validity, plan

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1
# wave (64) and select-tile (4096) boundaries, and more than two tiles
PROBE_SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 10001]
NP_DTYPES = {"int32": np.int32, "int64": np.int64}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build_keys(which: str, dtype) -> np.ndarray:
    """Build sides of 0, 1 and 5,000 rows; the large one has duplicates, negative keys and
    key 0, and rows exactly at its minimum and maximum."""
    if which == "empty":
        return np.zeros(0, dtype)
    if which == "one":
        return np.array([0], dtype)
    rng = np.random.default_rng(21)
    k = rng.integers(-3000, 3000, 5000)
    k[:4] = [-3000, 2999, 0, -1]
    return k.astype(dtype)


def probe_keys(n: int, lo: int, hi: int, dtype, seed: int) -> np.ndarray:
    """Random keys around [lo, hi] with, where they fit, the keys just outside the range on
    both sides and the extremes of the type (the range test's unsigned subtraction)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(lo - 500, hi + 501, n).astype(dtype)
    info = np.iinfo(dtype)
    special = [lo - 1, hi + 1, lo, hi, info.min, info.max, 0, info.min + 1, info.max - 1]
    for i, v in enumerate(special):
        if 2 * i + 1 < n:
            k[2 * i + 1] = v
    return k


def new_filter(dfp, kind, lo, hi, expected):
    from datafusion_parallelism_amd import KeyFilter

    return KeyFilter(0, kind, lo, hi, expected)


def words_of(f) -> np.ndarray:
    return f.words().cpu().numpy().view(np.uint64)


def check_probe_side(f, ref: RefFilter, pk: np.ndarray, valid, voff: int, base: int):
    """test and select of one probe batch against the restatement."""
    n = len(pk)
    vmask = None if valid is None else cuda(pack_validity(valid, voff))
    bitmap, count = f.test(cuda(pk), vmask, voff)
    want_bits, want_count = ref.test(pk, valid)
    assert count == want_count
    assert bitmap.dtype == torch.uint8 and bitmap.numel() == (n + 63) // 64 * 8
    assert np.array_equal(bitmap.cpu().numpy(), want_bits)
    keys, ids = f.select(cuda(pk), vmask, voff, probe_base=base)
    want_keys, want_ids = ref.select(pk, valid, base)
    assert keys.dtype == cuda(pk).dtype and ids.dtype == torch.int32
    assert np.array_equal(keys.cpu().numpy(), want_keys)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), want_ids)


@pytest.mark.parametrize("which", ["empty", "one", "dups"])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("kind", ["range", "bloom"])
def test_words_bitmap_and_select_match_the_restatement(dfp, kind, dtype, which):
    dt = NP_DTYPES[dtype]
    bk = build_keys(which, dt)
    rng = np.random.default_rng(3)
    bvalid = rng.random(len(bk)) > 0.1
    bvalid[:4] = True  # the rows at key_lo and key_hi stay
    lo, hi = (int(bk.min()), int(bk.max())) if len(bk) else (-10, 10)
    with new_filter(dfp, kind, lo, hi, len(bk)) as f:
        ref = RefFilter(kind, lo, hi, len(bk))
        info = f.info()
        assert (info["kind"], info["nwords"]) == (kind, ref.nwords) and info["exact"] == (kind == "range")
        assert (info["key_lo"], info["key_hi"], info["expected_keys"]) == (lo, hi, len(bk))
        assert not words_of(f).any()  # zeroed at creation
        # the build validity as a bitmap from bit 3
        f.add(cuda(bk), cuda(pack_validity(bvalid, 3)), 3)
        ref.add(bk, bvalid)
        assert np.array_equal(words_of(f), ref.words)
        assert f.info()["dropped_adds"] == 0
        for i, n in enumerate(PROBE_SIZES):
            pk = probe_keys(n, lo, hi, dt, seed=100 + i)
            pvalid = np.random.default_rng(200 + i).random(n) > 0.1
            check_probe_side(f, ref, pk, None, 0, 0)
            check_probe_side(f, ref, pk, pvalid, 0, 1000)
            check_probe_side(f, ref, pk, pvalid, 3, 0)
        if len(bk):  # every valid build key passes
            got, count = f.test(cuda(bk), bvalid)
            assert count == int(bvalid.sum())


def test_bloom_takes_the_extreme_keys(dfp):
    bk = np.array([INT64_MIN, INT64_MAX, 0, -1, 5, 5, INT64_MIN], np.int64)
    with new_filter(dfp, "bloom", 0, -1, len(bk)) as f:
        ref = RefFilter("bloom", 0, -1, len(bk))
        f.add(cuda(bk))
        ref.add(bk)
        assert np.array_equal(words_of(f), ref.words)
        pk = probe_keys(4097, -100, 100, np.int64, seed=9)
        pk[:7] = bk
        check_probe_side(f, ref, pk, None, 0, 0)
        keys, ids = f.select(cuda(pk))
        assert ids.cpu().numpy()[:7].tolist() == list(range(7))


@pytest.mark.parametrize("lo", [0, -7, INT64_MIN, INT64_MAX])
def test_range_of_width_one(dfp, lo):
    with new_filter(dfp, "range", lo, lo, 1) as f:
        ref = RefFilter("range", lo, lo, 1)
        assert f.info()["nwords"] == 1
        pk = np.array([lo, lo - 1 if lo > INT64_MIN else INT64_MAX, lo + 1 if lo < INT64_MAX else INT64_MIN,
                       INT64_MIN, INT64_MAX, 0], np.int64)
        check_probe_side(f, ref, pk, None, 0, 0)  # an empty filter passes nothing
        f.add(cuda(np.array([lo, lo], np.int64)))
        ref.add(np.array([lo, lo], np.int64))
        assert words_of(f).tolist() == [1]
        check_probe_side(f, ref, pk, None, 0, 0)


@pytest.mark.parametrize("kind", ["range", "bloom"])
def test_add_in_batches_in_any_order(dfp, kind):
    bk = build_keys("dups", np.int64)
    lo, hi = int(bk.min()), int(bk.max())
    a, b = bk[:1777], bk[1777:]
    got = []
    for batches in ([bk], [a, b], [b, a]):
        with new_filter(dfp, kind, lo, hi, len(bk)) as f:
            for x in batches:
                f.add(cuda(x))
            got.append(words_of(f))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    ref = RefFilter(kind, lo, hi, len(bk))
    ref.add(bk)
    assert np.array_equal(got[0], ref.words)


def test_range_counts_the_adds_it_drops(dfp):
    bk = build_keys("dups", np.int64)
    lo, hi = int(bk.min()), int(bk.max())
    outside = np.array([lo - 1, hi + 1, INT64_MIN, INT64_MAX, hi + 64, lo - 64, hi + 10**12], np.int64)
    mixed = np.concatenate([bk[:100], outside, bk[100:]])
    valid = np.ones(len(mixed), bool)
    with new_filter(dfp, "range", lo, hi, len(bk)) as f, new_filter(dfp, "range", lo, hi, len(bk)) as g:
        f.add(cuda(mixed), valid)
        g.add(cuda(bk))
        assert f.info()["dropped_adds"] == 7 and g.info()["dropped_adds"] == 0
        assert np.array_equal(words_of(f), words_of(g))
        # a null row outside the range is not an add at all
        valid[100:107] = False
        with new_filter(dfp, "range", lo, hi, len(bk)) as h:
            h.add(cuda(mixed), valid)
            assert h.info()["dropped_adds"] == 0


@pytest.mark.parametrize("kind", ["range", "bloom"])
def test_int32_probe_of_a_filter_filled_from_int64(dfp, kind):
    bk = build_keys("dups", np.int64)
    lo, hi = int(bk.min()), int(bk.max())
    pk = probe_keys(4097, lo, hi, np.int32, seed=4)
    with new_filter(dfp, kind, lo, hi, len(bk)) as f, new_filter(dfp, kind, lo, hi, len(bk)) as g:
        f.add(cuda(bk))
        g.add(cuda(bk.astype(np.int32)))
        assert np.array_equal(words_of(f), words_of(g))
        b32, c32 = f.test(cuda(pk))
        b64, c64 = f.test(cuda(pk.astype(np.int64)))
        assert c32 == c64 and torch.equal(b32, b64)
        k32, i32 = f.select(cuda(pk))
        k64, i64 = f.select(cuda(pk.astype(np.int64)))
        assert k32.dtype == torch.int32 and torch.equal(i32, i64) and torch.equal(k32.to(torch.int64), k64)


def test_from_keys_follows_the_auto_rule(dfp):
    from datafusion_parallelism_amd import KeyFilter

    dense = np.arange(0, 64 * 100, 64, dtype=np.int64)       # 100 keys over 6337 values: <= 64 per key
    sparse = np.arange(0, 66 * 100, 66, dtype=np.int64)      # 100 keys over 6535 values: more
    for bk, kind in ((dense, "range"), (sparse, "bloom"), (np.zeros(0, np.int64), "bloom")):
        with KeyFilter.from_keys(cuda(bk)) as f:
            info = f.info()
            lo, hi = (int(bk.min()), int(bk.max())) if len(bk) else (INT64_MAX, INT64_MIN)
            assert (info["kind"], info["nwords"]) == plan("auto", lo, hi, len(bk))
            assert info["kind"] == kind and (info["key_lo"], info["key_hi"]) == (lo, hi)
            ref = RefFilter("auto", lo, hi, len(bk))
            ref.add(bk)
            assert np.array_equal(words_of(f), ref.words)
    # nulls take no part in the range
    valid = np.ones(len(dense), bool)
    valid[[0, -1]] = False
    with KeyFilter.from_keys(cuda(dense), valid) as f:
        assert (f.info()["key_lo"], f.info()["key_hi"]) == (64, int(dense[-2]))


# ---- probe parity ---------------------------------------------------------------

def _join_case(layout: str):
    rng = np.random.default_rng(17)
    if layout == "dense":  # key range <= 8 x rows: direct-addressed
        bk = rng.integers(0, 8000, 5000).astype(np.int64)
        pk = rng.integers(0, 400_000, 20000).astype(np.int64)
    else:                  # 5,000 rows over a 10^9 range: hashed
        bk = rng.integers(0, 10**9, 3500).astype(np.int64)
        bk = np.concatenate([bk, bk[:1500]])  # duplicated keys
        pk = rng.integers(0, 10**9, 20000).astype(np.int64)
        hit = rng.random(len(pk)) < 0.02
        pk[hit] = rng.choice(bk, int(hit.sum()))
    bvalid = rng.random(len(bk)) > 0.05
    pvalid = rng.random(len(pk)) > 0.1
    return bk, bvalid, pk, pvalid


def _table(dfp, layout, bk, bvalid):
    if layout == "multi":
        t = dfp.HashTable(1, "int64", devices=[0, 0])
        t.append(0, cuda(bk), bvalid)
        t.finish(0)
        return t
    t = dfp.HashTable(1, "int64", 0).build(cuda(bk), bvalid)
    assert (t.stats()["buckets"] == 0) == (layout == "dense")
    return t


@pytest.mark.parametrize("kind", ["range", "bloom", "auto"])
@pytest.mark.parametrize("layout", ["hashed", "dense", "multi"])
def test_probe_with_prefilter_returns_the_same_pairs(dfp, layout, kind):
    from datafusion_parallelism_amd import KeyFilter

    bk, bvalid, pk, pvalid = _join_case("dense" if layout == "dense" else "hashed")
    with _table(dfp, layout, bk, bvalid) as t, KeyFilter.from_keys(cuda(bk), bvalid, kind=kind) as f:
        for valid, voff in ((None, 0), (pvalid, 0), (cuda(pack_validity(pvalid, 3)), 3)):
            b0, p0 = t.probe(cuda(pk), valid, device_output=True, valid_offset=voff)
            b1, p1 = t.probe(cuda(pk), valid, device_output=True, valid_offset=voff, prefilter=f)
            assert b0.numel() > 0
            assert b1.dtype == torch.int64 and p1.dtype == torch.int32
            assert torch.equal(b0, b1) and torch.equal(p0, p1)
        kept = f.test(cuda(pk), pvalid)[1]
        matched = len(np.unique(p0.cpu().numpy()))
        assert matched <= kept < len(pk) // 4  # the filter did drop most rows
        if f.info()["exact"]:
            assert kept == matched


@pytest.mark.parametrize("kind", ["range", "bloom", "auto"])
def test_all_miss_probe_returns_empty_tensors(dfp, kind):
    from datafusion_parallelism_amd import KeyFilter

    bk = np.arange(0, 10_000, 2, dtype=np.int64)
    pk = np.arange(1, 10_001, 2, dtype=np.int64)
    with dfp.HashTable(1, "int64", 0).build(cuda(bk)) as t, KeyFilter.from_keys(cuda(bk), kind="range") as exact:
        b, p = t.probe(cuda(pk), device_output=True, prefilter=exact)
        assert b.numel() == 0 and p.numel() == 0 and b.dtype == torch.int64 and p.dtype == torch.int32
        with KeyFilter.from_keys(cuda(bk), kind=kind) as f:
            b, p = t.probe(cuda(pk), device_output=True, prefilter=f)  # Bloom false positives miss in the table
            assert b.numel() == 0 and p.numel() == 0


@pytest.mark.parametrize("kind", ["bloom", "auto"])
def test_empty_build_returns_empty_tensors(dfp, kind):
    from datafusion_parallelism_amd import KeyFilter

    bk = np.zeros(0, np.int64)
    pk = np.arange(5000, dtype=np.int64)
    with dfp.HashTable(1, "int64", 0).build(cuda(bk)) as t, KeyFilter.from_keys(cuda(bk), kind=kind) as f:
        assert f.info()["nwords"] == 1 and f.test(cuda(pk))[1] == 0
        b, p = t.probe(cuda(pk), device_output=True, prefilter=f)
        assert b.numel() == 0 and p.numel() == 0
    # every build key null: the same
    bk = np.arange(100, dtype=np.int64)
    with dfp.HashTable(1, "int64", 0).build(cuda(bk), np.zeros(100, bool)) as t, \
            KeyFilter.from_keys(cuda(bk), np.zeros(100, bool), kind=kind) as f:
        b, p = t.probe(cuda(pk), device_output=True, prefilter=f)
        assert b.numel() == 0 and p.numel() == 0


def test_prefilter_needs_device_output(dfp):
    from datafusion_parallelism_amd import KeyFilter

    bk = np.arange(100, dtype=np.int64)
    with dfp.HashTable(1, "int64", 0).build(cuda(bk)) as t, KeyFilter.from_keys(cuda(bk)) as f:
        with pytest.raises(TypeError):
            t.probe(bk, prefilter=f)


# ---- operator parity --------------------------------------------------------------

JOIN_TYPES = ["inner", "left", "right", "full", "leftsemi", "leftanti", "rightsemi", "rightanti"]


def _sides(two_keys: bool = False):
    """Build and probe batches with nulls and duplicates in the keys of both sides."""
    rng = np.random.default_rng(29)

    def side(n, hi, prefix):
        k = rng.integers(0, hi, n)
        cols = {f"{prefix}k": pa.array(k, pa.int64(), mask=rng.random(n) < 0.08),
                f"{prefix}v": pa.array(rng.integers(0, 1000, n), pa.int32())}
        if two_keys:
            cols[f"{prefix}k2"] = pa.array(rng.integers(0, 3, n), pa.int32(), mask=rng.random(n) < 0.05)
        return pa.RecordBatch.from_pydict(cols)

    return side(3000, 40_000, "l"), side(6000, 60_000, "r")


def _collect(left_parts, right_parts, jt, prefilter, on, flt=None, right_schema=None):
    from datafusion_parallelism_amd.operator import ParallelHashJoin

    j = ParallelHashJoin(left_parts, right_parts, on=on, join_type=jt, filter=flt, right_schema=right_schema,
                         prefilter=prefilter)
    out = j.collect()
    assert (j._build._shared._filter is not None) == prefilter
    return pa.Table.from_batches(out) if out else None


def _rows(tbl):
    if tbl is None:
        return []
    return list(zip(*[c.to_pylist() for c in tbl.columns]))


def _sorted(rows):
    return sorted(rows, key=lambda t: tuple((x is None, x) for x in t))


@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_operator_prefilter_one_partition_row_for_row(dfp, jt):
    left, right = _sides()
    on = [("lk", "rk")]
    a = _collect([[left]], [[right]], jt, False, on, right_schema=right.schema)
    b = _collect([[left]], [[right]], jt, True, on, right_schema=right.schema)
    assert (a is None) == (b is None)
    if a is not None:
        assert a.num_rows > 0 and a.equals(b)


@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_operator_prefilter_two_partitions_sorted_rows(dfp, jt):
    left, right = _sides()
    on = [("lk", "rk")]
    lp = [[left.slice(0, 1000), left.slice(1000, 500)], [left.slice(1500)]]
    rp = [[right.slice(0, 2500)], [right.slice(2500, 3000), right.slice(5500)]]
    a = _collect(lp, rp, jt, False, on, right_schema=right.schema)
    b = _collect(lp, rp, jt, True, on, right_schema=right.schema)
    assert len(_rows(a)) > 0 and _sorted(_rows(a)) == _sorted(_rows(b))


@pytest.mark.parametrize("jt", ["inner", "full", "rightanti"])
def test_operator_prefilter_two_column_key(dfp, jt):
    left, right = _sides(two_keys=True)
    on = [("lk", "rk"), ("lk2", "rk2")]
    a = _collect([[left]], [[right]], jt, False, on, right_schema=right.schema)
    b = _collect([[left]], [[right]], jt, True, on, right_schema=right.schema)
    assert a.num_rows > 0 and a.equals(b)


@pytest.mark.parametrize("jt", ["inner", "left", "rightsemi"])
def test_operator_prefilter_with_join_filter(dfp, jt):
    from datafusion_parallelism_amd.operator import JoinFilter

    left, right = _sides()
    flt = JoinFilter(lambda l, r: pc.less(l.column("lv"), r.column("rv")), ["lv"], ["rv"])
    on = [("lk", "rk")]
    a = _collect([[left]], [[right]], jt, False, on, flt, right.schema)
    b = _collect([[left]], [[right]], jt, True, on, flt, right.schema)
    assert a.num_rows > 0 and a.equals(b)


# ---- TPC-H parity -------------------------------------------------------------------

def test_q3_with_the_prefilter_knob(dfp, monkeypatch):
    from datafusion_parallelism_amd import tpch

    calls = []
    real = tpch.KeyFilter.from_keys
    monkeypatch.setattr(tpch.KeyFilter, "from_keys", classmethod(lambda cls, *a, **k: calls.append(1) or real(*a, **k)))
    t = tpch.generate(0.01, "cuda:0", seed=3)
    monkeypatch.delenv("DFP_TPCH_PREFILTER", raising=False)
    want = tpch.q3(t, "BUILDING", "1995-03-15")
    assert not calls
    monkeypatch.setenv("DFP_TPCH_PREFILTER", "1")
    got = tpch.q3(t, "BUILDING", "1995-03-15")
    assert calls  # the joins did go through a filter
    assert got.groups == want.groups > 0
    assert (got.l_orderkey, got.revenue, got.o_orderdate, got.o_shippriority) == \
        (want.l_orderkey, want.revenue, want.o_orderdate, want.o_shippriority)
