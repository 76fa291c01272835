"""Times the filtered match probe (hj_probe_match_filtered) with HIP events next to what the
operator does without it for the same answer, the pair path: the pair probe into
preallocated buffers of exactly the pair count, hj_pair_filter_select over the pairs, then
hj_mark_rows + hj_select_rows over the surviving probe indices (RightSemi) or hj_mark_rows
over the surviving build indices (LeftSemi). The pair path is given its pair count and its
filtered count in advance (no second probe, no host read between its kernels): its best case.

Shapes: bench.py's c2 (one pair per match), the low-cardinality join of
tools/match_probe_bench.py (2000 keys of 1000 build rows, 2 * 10^6 probe rows over twice the
key range: 10^9 candidate pairs) and its orders x lineitem join (TPC-H Q3 at SF100, 1 % of
the probe rows match). Predicates: one int64 `!=` term (L.v != R.v), and a two-term band
(R.ts >= L.lo AND R.ts < L.hi, about a tenth of the pairs pass). All variants of a shape and
predicate alternate within one process: every round runs each once; warm-up rounds, then the
median of --reps rounds and [min .. max]. The LeftSemi variants zero the build flags inside
the timed region: flags left set by an earlier round would let the filtered probe skip.

    python tools/match_filter_bench.py > profiles/match_filter.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import pyarrow as pa
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (CONFIGS and gen_inputs: the benchmark's own shapes)
from match_probe_bench import q3_inputs, rounds  # noqa: E402
from datafusion_parallelism_amd import HashTable, _lib  # noqa: E402
from datafusion_parallelism_amd.columns import DeviceColumn, PairPredicate  # noqa: E402


def line(name: str, ms, note: str = "") -> None:
    med, lo, hi = ms
    print(f"  {name:<58s} {med * 1e3:10.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {note}", flush=True)


def verdict(match, pairs) -> str:
    """The comparison the two paths' own spreads allow."""
    ratio = pairs[0] / match[0]
    if match[1] > pairs[2]:
        return f"pair path {ratio:.2f} x the match path's time: the match path is slower beyond both spreads"
    if match[2] < pairs[1]:
        return f"pair path {ratio:.2f} x the match path's time: the match path is faster beyond both spreads"
    return f"pair path {ratio:.2f} x the match path's time: inside the two paths' spreads"


def col(t: torch.Tensor) -> DeviceColumn:
    return DeviceColumn(pa.int64(), t.numel(), data=t.view(torch.uint8))


def predicates(dev, B: int, n: int):
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    bv = torch.randint(0, 1000, (B,), dtype=torch.int64, device=dev, generator=g)
    pv = torch.randint(0, 1000, (n,), dtype=torch.int64, device=dev, generator=g)
    lo = torch.randint(0, 1000, (B,), dtype=torch.int64, device=dev, generator=g)
    hi = lo + 100
    ne = PairPredicate([col(bv)], [col(pv)], [(("build", 0), "!=", ("probe", 0))], B, n)
    band = PairPredicate([col(lo), col(hi)], [col(pv)],
                         [(("probe", 0), ">=", ("build", 0)), (("probe", 0), "<", ("build", 1))], B, n)
    return {"L.v != R.v": ne, "R.ts >= L.lo AND R.ts < L.hi": band}


def run_shape(name: str, bk: torch.Tensor, pk: torch.Tensor, args) -> None:
    L = _lib.load()
    dev = pk.device
    s = torch.cuda.current_stream(dev).cuda_stream or None
    B, n = bk.numel(), pk.numel()
    with HashTable(1, "int64", dev.index or 0) as t:
        t.build(bk)
        st = t.stats()
        h = t._h
        bitmap = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev)
        bflags = torch.zeros(B, dtype=torch.uint8, device=dev)
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        sws = torch.empty(L.hj_select_bitmap_workspace_bytes(n), dtype=torch.uint8, device=dev)
        pws = torch.empty(L.hj_probe_workspace_bytes(n), dtype=torch.uint8, device=dev)
        pflags = torch.empty(n, dtype=torch.uint8, device=dev)
        rows64 = torch.empty(n, dtype=torch.int64, device=dev)
        rws = torch.empty(L.hj_select_workspace_bytes(n), dtype=torch.uint8, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        fcnt = torch.zeros(1, dtype=torch.int64, device=dev)
        print(f"{name}: build {B} rows ({'direct-addressed' if st['buckets'] == 0 else 'hashed'}, "
              f"{st['distinct_keys']} keys, max {st['max_key_rows']} rows per key), probe {n} rows", flush=True)
        for pname, pred in predicates(dev, B, n).items():
            def match(bm, flags):
                _lib.check(L.hj_probe_match_filtered(h, pk.data_ptr(), None, 0, n, pred.struct, bm, None, flags,
                                                     B if flags else 0, stats.data_ptr(), s))

            def select_bitmap():
                _lib.check(L.hj_select_bitmap(bitmap.data_ptr(), 0, n, 1, 0, rows.data_ptr(), cnt.data_ptr(),
                                              sws.data_ptr(), s))

            match(bitmap.data_ptr(), None)
            matched, _, pairs = stats.tolist()
            # the pair path, sized by the known pair count
            cap = max(pairs, 1)
            ob = torch.empty(cap, dtype=torch.int64, device=dev)
            op = torch.empty(cap, dtype=torch.int32, device=dev)
            fb = torch.empty(cap, dtype=torch.int64, device=dev)
            fp = torch.empty(cap, dtype=torch.int32, device=dev)
            fws = torch.empty(L.hj_pair_filter_workspace_bytes(pairs), dtype=torch.uint8, device=dev)

            def pairs_filtered():
                _lib.check(L.hj_probe_async(h, pk.data_ptr(), None, 0, n, ob.data_ptr(), op.data_ptr(), cap,
                                            d_total.data_ptr(), pws.data_ptr(), s))
                _lib.check(L.hj_pair_filter_select(pred.struct, ob.data_ptr(), op.data_ptr(), pairs, fb.data_ptr(),
                                                   fp.data_ptr(), fcnt.data_ptr(), fws.data_ptr(), s))

            pairs_filtered()
            assert int(d_total.item()) == pairs, (int(d_total.item()), pairs)
            passing = int(fcnt.item())

            def right_semi_pairs():
                pairs_filtered()
                pflags.zero_()
                _lib.check(L.hj_mark_rows(fp.data_ptr(), 4, passing, pflags.data_ptr(), n, s))
                _lib.check(L.hj_select_rows(pflags.data_ptr(), n, 1, rows64.data_ptr(), cnt.data_ptr(), rws.data_ptr(), s))

            def left_semi_pairs():
                bflags.zero_()
                pairs_filtered()
                _lib.check(L.hj_mark_rows(fb.data_ptr(), 8, passing, bflags.data_ptr(), B, s))

            def right_semi_match():
                match(bitmap.data_ptr(), None)
                select_bitmap()

            def left_semi_match():
                bflags.zero_()
                match(None, bflags.data_ptr())

            # the two paths agree before anything is timed
            right_semi_pairs()
            want_rows = rows64[: int(cnt.item())].clone()
            right_semi_match()
            assert int(cnt.item()) == matched == want_rows.numel() and torch.equal(rows[:matched].long(), want_rows)
            left_semi_pairs()
            want_flags = bflags.clone()
            left_semi_match()
            assert torch.equal(bflags, want_flags)
            res = rounds({"rsemi match": right_semi_match, "rsemi pairs": right_semi_pairs,
                          "lsemi match": left_semi_match, "lsemi pairs": left_semi_pairs}, args.warmup, args.reps)
            print(f" {pname}: candidates {pairs}, passing {passing} ({passing / max(pairs, 1):.1%}), probe rows kept "
                  f"{matched}, build rows marked {int(want_flags.sum())}", flush=True)
            line("RightSemi  hj_probe_match_filtered + hj_select_bitmap", res["rsemi match"])
            line("RightSemi  probe + pair_filter_select + mark + select", res["rsemi pairs"],
                 verdict(res["rsemi match"], res["rsemi pairs"]))
            line("LeftSemi   hj_probe_match_filtered (build_flags only)", res["lsemi match"])
            line("LeftSemi   probe + pair_filter_select + mark", res["lsemi pairs"],
                 verdict(res["lsemi match"], res["lsemi pairs"]))
            del ob, op, fb, fp, fws


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,skew,q3", help="comma-separated: c2, skew, q3")
    ap.add_argument("--skew-rows", type=int, default=2_000_000, help="build rows = probe rows of the skew shape")
    ap.add_argument("--skew-keys", type=int, default=2000)
    ap.add_argument("--q3-build-rows", type=int, default=14_600_000)
    ap.add_argument("--q3-probe-rows", type=int, default=323_000_000)
    ap.add_argument("--q3-orders", type=int, default=150_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"# HIP events; every round runs each variant once; median of {args.reps} rounds after {args.warmup} "
          "warm-up rounds, [min .. max]", flush=True)
    for shape in args.shapes.split(","):
        if shape == "skew":
            B, K = args.skew_rows, args.skew_keys
            bk = torch.arange(B, dtype=torch.int64, device=dev) % K
            g = torch.Generator(device=dev)
            g.manual_seed(2)
            pk = torch.randint(0, 2 * K, (B,), dtype=torch.int64, device=dev, generator=g)
            run_shape(f"skew: {K} keys of {B // K} build rows", bk, pk, args)
        elif shape == "q3":
            bk, probes = q3_inputs(dev, args.q3_build_rows, args.q3_probe_rows, args.q3_orders)
            pk = probes["shuffled"]
            del probes
            run_shape("q3 orders x lineitem, probe shuffled", bk, pk, args)
        else:
            bk, pk, _, _ = bench.gen_inputs(bench.CONFIGS[shape], 0, 1, dev)
            run_shape(shape, bk, pk, args)
        del bk, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
