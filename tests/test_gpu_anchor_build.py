"""The anchor build: the speculative dense frag build without a key-range pass. Its
partition bins every build key by 8192-value block relative to the first build key (the
anchor), leaves each tile's exact key range, and a fold publishes the range; keys beyond
2047 blocks from the anchor (far keys) make the build take another layout.

Every case is built once and probed through the fused and the sliced probe; pairs are
bit-exact against the oracle (canonical order), and ``stats()["buckets"]`` says which
layout was built. Builds whose first batch carries a validity bitmap keep the key-range
reduction (the anchor must be a valid key the kernels can read at once); they are here all
the same, as are builds whose later batches carry one (those take the anchor build).

Run on an MI355X: ``pytest -m gpu``.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I64_MIN = int(np.iinfo(np.int64).min)
I64_MAX = int(np.iinfo(np.int64).max)
BLK = 8192
N = 50_000        # 4 tiles of 16384 rows (the last one partial)
BIG = 2_100_000   # 8 x rows just covers 2048 blocks: the block-limit cases stay dense
GOLD = 0x9E3779B97F4A7C15


def _perm(rng, lo, span, n):
    """n distinct keys of [lo, lo + span) in a permuted order, both ends among them."""
    k = rng.permutation(span)[:n].astype(np.int64)
    k[1], k[2] = 0, span - 1
    return k + np.int64(lo)  # lo + span - 1 <= INT64_MAX in every case below


def _anchor_at(bk, where):
    """Move the minimum / maximum / a middle key to row 0 (the anchor)."""
    bk = bk.copy()
    order = np.argsort(bk, kind="stable")
    i = {"min": order[0], "max": order[-1], "mid": order[len(bk) // 2]}[where]
    bk[0], bk[i] = bk[i], bk[0]
    return bk


def _bitmap(mask, off):
    """An LSB validity bitmap whose bit `off` is row 0 (the bits before it are set: a
    reader that ignored the offset would see valid rows)."""
    return np.packbits(np.concatenate([np.ones(off, bool), mask]), bitorder="little")


def _case(name):
    """-> dict(batches=[(partition, keys, mask | None, bitmap bit offset)], key_type)."""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))
    kt = "int64"
    one = lambda bk, mask=None, off=0: [(0, np.asarray(bk), mask, off)]  # noqa: E731
    if name in ("anchor_min", "anchor_max", "anchor_mid"):
        batches = one(_anchor_at(_perm(rng, 123_457, 6 * N, N), name[7:]))
    elif name == "min_below_block":  # min = k * 8192 - 1: one key in the table's first block
        batches = one(_anchor_at(_perm(rng, 37 * BLK - 1, 5 * N, N), "mid"))
    elif name == "straddle_zero":
        batches = one(_perm(rng, -3 * N - 11, 6 * N, N))
    elif name == "all_negative":
        batches = one(_anchor_at(_perm(rng, -9 * N, 7 * N, N), "max"))
    elif name == "near_i64_min":
        batches = one(_anchor_at(_perm(rng, I64_MIN, 6 * N, N), "mid"))
    elif name == "near_i64_max":
        batches = one(_anchor_at(_perm(rng, I64_MAX - 6 * N + 1, 6 * N, N), "mid"))
    elif name == "i64_min_anchor":
        batches = one(_anchor_at(_perm(rng, I64_MIN, 6 * N, N), "min"))
    elif name == "i64_max_anchor":
        batches = one(_anchor_at(_perm(rng, I64_MAX - 6 * N + 1, 6 * N, N), "max"))
    elif name in ("blocks_2047", "blocks_2048"):  # an aligned exact range of that many blocks
        nb = int(name[7:])
        batches = one(_anchor_at(_perm(rng, -5 * BLK, nb * BLK, BIG), "max" if nb == 2048 else "min"))
    elif name == "aligned_cap_plus_1":  # 2048 blocks exactly (ceil), 2049 aligned ones
        batches = one(_anchor_at(_perm(rng, 3 * BLK + 100, 2048 * BLK - 50, BIG), "mid"))
    elif name == "anchor_mid_pm2047":  # every bin 0..4094 in use, none far: too sparse, hashed
        bk = _perm(rng, -2047 * BLK, 4095 * BLK, BIG)
        bk[0] = 5  # the anchor, in block 0
        batches = one(bk)
    elif name in ("one_key_p2048", "one_key_m2048"):  # one far key, exactly 2048 bins away
        bk = _perm(rng, 40 * BLK, 2000 * BLK, BIG)
        if name == "one_key_p2048":
            bk = _anchor_at(bk, "min")
            bk[BIG // 2] = (int(bk[0]) // BLK + 2048) * BLK
        else:
            bk = _anchor_at(bk, "max")
            bk[BIG // 2] = (int(bk[0]) // BLK - 2048) * BLK + BLK - 1
        batches = one(bk)
    elif name == "far_first_tile":
        bk = _perm(rng, 1000, 6 * N, N)
        bk[777] = 10**15
        batches = one(bk)
    elif name == "far_last_tile":  # the earlier tiles have sorted when the far key shows
        bk = _perm(rng, 1000, 6 * N, N)
        bk[N - 3] = -(10**15)
        batches = one(bk)
    elif name == "all_far":
        with np.errstate(over="ignore"):
            batches = one((np.arange(1, N + 1, dtype=np.uint64) * np.uint64(GOLD)).view(np.int64))
    elif name == "every_key_twice":
        k = _perm(rng, -7000, 3 * N, N // 2)
        bk = np.concatenate([k, k])
        rng.shuffle(bk)
        batches = one(bk)
    elif name == "one_key_10000":
        bk = np.concatenate([_perm(rng, 500, 5 * N, N - 10_000), np.full(10_000, 4242, np.int64)])
        rng.shuffle(bk)
        batches = one(bk)
    elif name == "exponential":
        batches = one(None)  # filled by the test (the oracle's generator)
    elif name in ("bitmap_offset", "first_row_null", "first_tile_null"):  # first batch with a bitmap
        bk = _perm(rng, -20_000, 6 * N, N)
        mask = rng.random(N) > 0.1
        if name == "first_row_null":
            mask[0] = False
        if name == "first_tile_null":
            mask[:16384 + 5] = False
        batches = one(bk, mask, 0 if name == "first_row_null" else 5)
    elif name in ("later_batch_nulls", "later_batch_tile_null"):  # anchor build, tiles with a bitmap
        bk = _perm(rng, 9 * BLK - 3, 6 * N, N)
        mask = rng.random(N - 20_000) > 0.2
        if name == "later_batch_tile_null":
            mask[:16384] = False
        batches = [(0, bk[:20_000], None, 0), (0, bk[20_000:], mask, 3)]
    elif name == "int32":
        kt = "int32"
        batches = one(_anchor_at(_perm(rng, -2**31, 6 * N, N), "mid").astype(np.int32))
    elif name == "int32_top":
        kt = "int32"
        batches = one(_anchor_at(_perm(rng, 2**31 - 6 * N, 6 * N, N), "min").astype(np.int32))
    elif name == "three_batches_two_parts":  # canonical rows: partition 0's batches, then 1's
        bk = _perm(rng, -BLK - 1, 6 * N, N)
        batches = [(0, bk[:17_000], None, 0), (1, bk[17_000:40_001], None, 0), (0, bk[40_001:], None, 0)]
    elif name == "empty":
        batches = one(np.zeros(0, np.int64))
    elif name == "one_row":
        batches = one(np.array([-8193], np.int64))
    elif name == "all_null":
        batches = one(_perm(rng, 0, 6 * N, N), np.zeros(N, bool), 0)
    else:
        raise KeyError(name)
    return {"batches": batches, "key_type": kt}


CASES = ["anchor_min", "anchor_max", "anchor_mid", "min_below_block", "straddle_zero", "all_negative",
         "near_i64_min", "near_i64_max", "i64_min_anchor", "i64_max_anchor",
         "blocks_2047", "blocks_2048", "aligned_cap_plus_1", "anchor_mid_pm2047", "one_key_p2048", "one_key_m2048",
         "far_first_tile", "far_last_tile", "all_far",
         "every_key_twice", "one_key_10000", "exponential",
         "bitmap_offset", "first_row_null", "first_tile_null", "later_batch_nulls", "later_batch_tile_null",
         "int32", "int32_top", "three_batches_two_parts", "empty", "one_row", "all_null"]


def _canonical(batches):
    """The build side in canonical row order (partition, then append order) + its mask."""
    ordered = sorted(range(len(batches)), key=lambda i: (batches[i][0], i))
    keys = np.concatenate([batches[i][1] for i in ordered])
    masks = [np.ones(len(batches[i][1]), bool) if batches[i][2] is None else batches[i][2] for i in ordered]
    return keys, np.concatenate(masks)


def _probe_keys(rng, bk, mask):
    """Build keys (valid and null ones), near misses around the key range and, for a
    dense range, its block-aligned surroundings; clipped to the key type."""
    info = np.iinfo(bk.dtype)
    if bk.size == 0:
        return rng.integers(-1000, 1000, 5000).astype(bk.dtype)
    vk = bk[mask] if mask.any() else bk
    lo, hi = int(vk.min()), int(vk.max())
    parts = [rng.choice(np.unique(bk), 60_000)]  # (by value: a hot key's rows pair once or twice)
    if hi - lo < 2**40:
        a, b = max(lo - 2 * BLK, info.min), min(hi + 2 * BLK, info.max)
        parts.append((rng.integers(0, b - a + 1, 60_000, dtype=np.uint64).astype(object) + a).astype(bk.dtype))
    else:
        parts.append(rng.integers(info.min, info.max, 60_000, dtype=bk.dtype))
    edge = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, lo // BLK * BLK, lo // BLK * BLK - 1, info.min, info.max, 0]
    parts.append(np.array([min(max(e, info.min), info.max) for e in edge], dtype=bk.dtype))
    return np.concatenate(parts)


def _build(dfp, case):
    nparts = max(p for p, *_ in case["batches"]) + 1
    t = dfp.HashTable(nparts, case["key_type"], 0)
    for p, keys, mask, off in case["batches"]:
        if mask is None:
            t.append(p, torch.from_numpy(keys.copy()).cuda())
        elif off == 0:
            t.append(p, torch.from_numpy(keys.copy()).cuda(), mask)
        else:
            t.append(p, torch.from_numpy(keys.copy()).cuda(), torch.from_numpy(_bitmap(mask, off)).cuda(),
                     valid_offset=off)
    t.finish_all()
    return t


def _probe_both(dfp, t, pk):
    """The pairs through the fused (3) and the sliced (4) probe."""
    L = dfp.load()
    out = []
    old = L.hj_set_probe_mode(3)
    try:
        for mode in (3, 4):
            L.hj_set_probe_mode(mode)
            out.append(t.probe(torch.from_numpy(pk.copy()).cuda()))
    finally:
        L.hj_set_probe_mode(old)
    return out


def _same(got, want, what):
    (b, p), (ob, op) = got, want
    assert len(b) == len(ob), f"{what}: count {len(b)} != oracle {len(ob)}"
    assert np.array_equal(np.asarray(p, np.uint32), op), f"{what}: probe indices differ"
    assert np.array_equal(np.asarray(b, np.uint64), ob), f"{what}: build indices differ"


@pytest.mark.parametrize("name", CASES)
def test_anchor_build(dfp, oracle_mod, name):
    """Pairs equal to the oracle's through both probes; the layout the exact key range
    gives (direct-addressed when it spans at most 8 x valid rows); for a direct-addressed
    table the exact key_min / nvalues, and the exported piece, wrapped, probes alike."""
    case = _case(name)
    if name == "exponential":
        case["batches"] = [(0, oracle_mod.make_exponential_int_array(0, N).astype(np.int64), None, 0)]
    rng = np.random.default_rng(len(name))
    bk, mask = _canonical(case["batches"])
    pk = _probe_keys(rng, bk, mask)
    want = oracle_mod.inner_join(bk, pk, None if mask.all() else mask)
    t = _build(dfp, case)
    try:
        for got, mode in zip(_probe_both(dfp, t, pk), ("fused", "sliced")):
            _same(got, want, mode)
        st = t.stats()
        nvalid = int(mask.sum())
        if nvalid == 0:
            return
        lo, hi = int(bk[mask].min()), int(bk[mask].max())
        dense = hi - lo + 1 <= 8 * len(bk)  # the layout rule: the range against 8 x build rows
        assert (st["buckets"] == 0) == dense, (st, lo, hi)
        if not dense:
            return
        piece = t.dense_piece()
        assert piece["key_min"] == lo and piece["nvalues"] == hi - lo + 1, (piece, lo, hi)
        if piece["nvalues"] > 3_000_000:  # the block-limit cases: the observables only
            return
        refs = torch.empty(piece["nvalues"], dtype=torch.int32, device="cuda")
        used = torch.zeros(1, dtype=torch.int64, device="cuda")
        t.dense_export(dup_used=used)
        dup = torch.empty(max(int(used.item()), 1), dtype=torch.int32, device="cuda")
        t.dense_export(refs=refs, dup=dup)
        torch.cuda.synchronize()
        w = dfp.HashTable.wrap_dense(0, case["key_type"], piece["key_min"], refs, dup, piece["packed"])
        try:
            for got, mode in zip(_probe_both(dfp, w, pk), ("wrapped fused", "wrapped sliced")):
                _same(got, want, mode)
        finally:
            w.close()
    finally:
        t.close()


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(0, sys.argv[1] + "/tests")
import oracle, datafusion_parallelism_amd as dfp, test_gpu_anchor_build as T
dfp.load()
for name in sys.argv[2:]:
    case = T._case(name)
    bk, mask = T._canonical(case["batches"])
    pk = T._probe_keys(np.random.default_rng(len(name)), bk, mask)
    t = T._build(dfp, case)
    for b, p in T._probe_both(dfp, t, pk):
        print(name, oracle.pairs_digest(b, p), t.stats()["buckets"])
    t.close()
"""


def test_anchor_build_knob_off(dfp, oracle_mod):
    """DFP_HJ_ANCHOR_BUILD=0 (read once per process: a fresh child) restores the key-range
    reduction before the partition; pairs and layouts are the same."""
    names = ["anchor_mid", "min_below_block", "near_i64_max", "far_last_tile", "later_batch_nulls"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DFP_HJ_ANCHOR_BUILD="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, *names], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in names]
    assert len(lines) == 2 * len(names), r.stdout
    for name in names:
        case = _case(name)
        bk, mask = _canonical(case["batches"])
        pk = _probe_keys(np.random.default_rng(len(name)), bk, mask)
        ob, op = oracle_mod.inner_join(bk, pk, None if mask.all() else mask)
        want = oracle_mod.pairs_digest(ob, op)
        t = _build(dfp, case)
        try:
            buckets = t.stats()["buckets"]
        finally:
            t.close()
        for ln in lines:
            if ln[0] == name:
                assert ln[1] == want, f"{name}: pairs differ with the knob off"
                assert int(ln[2]) == buckets, f"{name}: layout differs with the knob off"
