"""Times the match probe (hj_probe_match: bitmap only, with counts, with build flags) and
hj_select_bitmap with HIP events, next to what the operator does today for the same answer:
the pair probe into preallocated buffers, then hj_mark_rows + hj_select_rows over the probe
indices (RightSemi / RightAnti), plus hj_mark_rows over the build indices (LeftSemi /
LeftAnti). Shapes: bench.py's c2, c2h and c3 (its generators and sizes, imported from it) and
the orders x lineitem join of tools/key_filter_bench.py (TPC-H Q3 at SF100), probe side
clustered and shuffled, and a low-cardinality join (2000 keys of 1000 build rows each: 10^9
pairs) as the skewed case the pair path can still hold. All variants of a shape alternate
within one process: every round runs each of them once; warm-up rounds, then the median of
--reps rounds and [min .. max].
Each match line carries its algorithmic bytes (key bytes + n/8 bitmap bytes + 4 table bytes
per in-range row of a direct-addressed table or 64 per valid row of a hashed one, + 4 n with
counts) and the rate they give.

    python tools/match_probe_bench.py > profiles/match_probe.txt

The pair path is given its pair count in advance (buffers of exactly that capacity, no
second probe, no host read of the total between its kernels): its best case.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS and gen_inputs: the benchmark's own shapes)
from datafusion_parallelism_amd import HashTable, _lib  # noqa: E402


def order_key(i: torch.Tensor) -> torch.Tensor:
    """TPC-H's sparse order keys: 8 consecutive values of every 32 (key_filter_bench.py)."""
    return (i // 8) * 32 + i % 8 + 1


def q3_inputs(dev, B: int, P: int, orders: int):
    """tools/key_filter_bench.py's build and probe sides: a random tenth of the orders in
    key order; 99 % of the probe rows belong to orders that are not in the build."""
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    half = orders // 2
    bidx = 2 * torch.randint(0, half, (B,), device=dev, generator=g).sort().values
    bk = order_key(bidx)
    pidx = 2 * torch.randint(0, half, (P,), device=dev, generator=g) + 1
    nhit = P // 100
    pidx[:nhit] = bidx[torch.randint(0, B, (nhit,), device=dev, generator=g)]
    clustered = order_key(pidx.sort().values)
    del pidx, bidx
    shuffled = clustered[torch.randperm(P, device=dev, generator=g)]
    return bk, {"clustered": clustered, "shuffled": shuffled}


def rounds(variants: dict, warmup: int, reps: int) -> dict:
    """Every round runs each variant once (alternating); -> name: (median, min, max) ms."""
    ts = {k: [] for k in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts[name].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def line(name: str, ms, alg_bytes: int | None = None, note: str = "") -> None:
    med, lo, hi = ms
    alg = f"alg {alg_bytes / 1e6:9.1f} MB {alg_bytes / med / 1e6:8.1f} GB/s" if alg_bytes else " " * 35
    print(f"  {name:<46s} {med * 1e3:10.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {alg}  {note}", flush=True)


def run_shape(name: str, bk: torch.Tensor, pk: torch.Tensor, args) -> None:
    L = _lib.load()
    dev = pk.device
    s = torch.cuda.current_stream(dev).cuda_stream or None
    B, n = bk.numel(), pk.numel()
    kb = pk.element_size()
    with HashTable(1, "int64", dev.index or 0) as t:
        t.build(bk)
        st = t.stats()
        dense = st["buckets"] == 0
        if dense:
            piece = t.dense_piece()
            d = pk - piece["key_min"]
            inrange = int(((d >= 0) & (d < piece["nvalues"])).sum())
            del d
            table_bytes = 4 * inrange
        else:
            table_bytes = 64 * n
        h = t._h
        bitmap = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        bflags = torch.zeros(B, dtype=torch.uint8, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        mws = torch.empty(t.match_workspace_bytes(n), dtype=torch.uint8, device=dev)
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        sws = torch.empty(L.hj_select_bitmap_workspace_bytes(n), dtype=torch.uint8, device=dev)

        def match(c=None, f=None):
            _lib.check(L.hj_probe_match(h, pk.data_ptr(), None, 0, n, bitmap.data_ptr(), c, f, B if f else 0,
                                        stats.data_ptr(), mws.data_ptr(), s))

        def select_bitmap():
            _lib.check(L.hj_select_bitmap(bitmap.data_ptr(), 0, n, 1, 0, rows.data_ptr(), cnt.data_ptr(),
                                          sws.data_ptr(), s))

        match()
        matched, pairs = stats.tolist()
        # the pair path, sized by the known pair count
        cap = max(pairs, 1)
        ob = torch.empty(cap, dtype=torch.int64, device=dev)
        op = torch.empty(cap, dtype=torch.int32, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        pws = torch.empty(L.hj_probe_workspace_bytes(n), dtype=torch.uint8, device=dev)
        pflags = torch.empty(n, dtype=torch.uint8, device=dev)
        rows64 = torch.empty(n, dtype=torch.int64, device=dev)
        rws = torch.empty(L.hj_select_workspace_bytes(n), dtype=torch.uint8, device=dev)

        def pair_probe():
            _lib.check(L.hj_probe_async(h, pk.data_ptr(), None, 0, n, ob.data_ptr(), op.data_ptr(), cap,
                                        d_total.data_ptr(), pws.data_ptr(), s))

        def right_semi_pairs():
            pair_probe()
            pflags.zero_()
            _lib.check(L.hj_mark_rows(op.data_ptr(), 4, pairs, pflags.data_ptr(), n, s))
            _lib.check(L.hj_select_rows(pflags.data_ptr(), n, 1, rows64.data_ptr(), cnt.data_ptr(), rws.data_ptr(), s))

        def left_semi_pairs():
            pair_probe()
            _lib.check(L.hj_mark_rows(ob.data_ptr(), 8, pairs, bflags.data_ptr(), B, s))

        def right_semi_match():
            match()
            select_bitmap()

        pair_probe()
        assert int(d_total.item()) == pairs, (int(d_total.item()), pairs)
        res = rounds({
            "match bitmap": match,
            "match counts": lambda: match(c=counts.data_ptr()),
            "match flags": lambda: match(f=bflags.data_ptr()),
            "select_bitmap": select_bitmap,
            "rsemi match": right_semi_match,
            "pair probe": pair_probe,
            "rsemi pairs": right_semi_pairs,
            "lsemi pairs": left_semi_pairs,
        }, args.warmup, args.reps)
        key_bytes = kb * n + n // 8
        print(f"{name}: build {B} rows ({'direct-addressed' if dense else 'hashed'}, {st['distinct_keys']} keys, "
              f"max {st['max_key_rows']} rows per key), probe {n} rows, matched {matched} ({matched / n:.2%}), "
              f"pairs {pairs}", flush=True)
        line("hj_probe_match  bitmap", res["match bitmap"], key_bytes + table_bytes)
        line("hj_probe_match  bitmap + counts", res["match counts"], key_bytes + table_bytes + 4 * n)
        line("hj_probe_match  bitmap + build_flags", res["match flags"], key_bytes + table_bytes,
             "= LeftSemi / LeftAnti, match path")
        line("hj_select_bitmap", res["select_bitmap"], n // 8 + 4 * matched)
        line("hj_probe_match + hj_select_bitmap", res["rsemi match"], None, "= RightSemi, match path")
        line("hj_probe_async (pairs)", res["pair probe"], None)
        line("hj_probe_async + mark_rows(p) + select_rows", res["rsemi pairs"], None,
             f"= RightSemi, the pair path takes {res['rsemi pairs'][0] / res['rsemi match'][0]:.2f} x the time of the match path")
        line("hj_probe_async + mark_rows(b)", res["lsemi pairs"], None,
             f"= LeftSemi, the pair path takes {res['lsemi pairs'][0] / res['match flags'][0]:.2f} x the time of the match path")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c2h,c3,q3,skew", help="comma-separated: c2, c2h, c3, q3, skew")
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
            # a low-cardinality key: 2000 keys of 1000 build rows each (rows of a key apart: no
            # run refs), probed by 2 * 10^6 rows over twice the key range: 10^9 pairs (12 GB)
            B, K = args.skew_rows, args.skew_keys
            bk = torch.arange(B, dtype=torch.int64, device=dev) % K
            g = torch.Generator(device=dev)
            g.manual_seed(2)
            pk = torch.randint(0, 2 * K, (B,), dtype=torch.int64, device=dev, generator=g)
            run_shape(f"skew: {K} keys of {B // K} build rows", bk, pk, args)
            del bk, pk
        elif shape == "q3":
            bk, probes = q3_inputs(dev, args.q3_build_rows, args.q3_probe_rows, args.q3_orders)
            for order, pk in probes.items():
                run_shape(f"q3 orders x lineitem, probe {order}", bk, pk, args)
            del bk, probes
        else:
            bk, pk, _, _ = bench.gen_inputs(bench.CONFIGS[shape], 0, 1, dev)
            run_shape(shape, bk, pk, args)
            del bk, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
