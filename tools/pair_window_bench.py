"""Times the pair plan (hj_pair_plan) and the pair windows (hj_pair_window) with HIP events,
next to the pair probe (hj_probe_async) into buffers of exactly the pair count: its best case,
and the memory the windows exist to avoid. Shapes: bench.py's c2 and c3 (its generators and
sizes, imported from it), a 1000-rows-per-key join (2000 keys of 1000 build rows each: 10^9
pairs) and a sparse probe (one row in 1000 has a partner). Per shape: the plan, every window
of 2^22 pairs and of 2^24 pairs one after another into one reused buffer of that size, one
window of the full output, and plan + windows together. All variants of a shape alternate
within one process: every round runs each of them once; warm-up rounds, then the median of
--reps rounds and [min .. max].

    python tools/pair_window_bench.py > profiles/pair_window.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (CONFIGS and gen_inputs: the benchmark's own shapes)
from datafusion_parallelism_amd import HashTable, _lib  # noqa: E402
from match_probe_bench import rounds  # noqa: E402

WINDOWS = (1 << 22, 1 << 24)


def line(name: str, ms, pairs: int | None = None, note: str = "") -> None:
    med, lo, hi = ms
    rate = f"{pairs / med / 1e6:8.2f} Gpairs/s" if pairs else " " * 17
    print(f"  {name:<44s} {med * 1e3:10.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {rate}  {note}", flush=True)


def run_shape(name: str, bk: torch.Tensor, pk: torch.Tensor, args) -> None:
    L = _lib.load()
    dev = pk.device
    s = torch.cuda.current_stream(dev).cuda_stream or None
    B, n = bk.numel(), pk.numel()
    with HashTable(1, "int64", dev.index or 0) as t:
        t.build(bk)
        st = t.stats()
        h = t._h
        plan = torch.empty(t.pair_plan_bytes(n), dtype=torch.uint8, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)

        def make_plan():
            _lib.check(L.hj_pair_plan(h, pk.data_ptr(), None, 0, n, plan.data_ptr(), d_total.data_ptr(), s))

        make_plan()
        pairs = int(d_total.item())
        cap = max(pairs, 1)
        ob = torch.empty(cap, dtype=torch.int64, device=dev)
        op = torch.empty(cap, dtype=torch.int32, device=dev)
        p_total = torch.zeros(1, dtype=torch.int64, device=dev)
        pws = torch.empty(L.hj_probe_workspace_bytes(n), dtype=torch.uint8, device=dev)

        def pair_probe():
            _lib.check(L.hj_probe_async(h, pk.data_ptr(), None, 0, n, ob.data_ptr(), op.data_ptr(), cap,
                                        p_total.data_ptr(), pws.data_ptr(), s))

        def windows(size: int):
            # every window into the first `size` elements: the caller's memory is one window's
            for lo in range(0, pairs, size):
                _lib.check(L.hj_pair_window(h, plan.data_ptr(), n, None, 0, lo, min(size, cap), ob.data_ptr(),
                                            op.data_ptr(), None, s))

        def plan_and_windows(size: int):
            make_plan()
            windows(size)

        pair_probe()
        assert int(p_total.item()) == pairs, (int(p_total.item()), pairs)
        # the full window must reproduce the pair probe before anything is timed
        wb, wp = torch.empty_like(ob), torch.empty_like(op)
        _lib.check(L.hj_pair_window(h, plan.data_ptr(), n, None, 0, 0, cap, wb.data_ptr(), wp.data_ptr(), None, s))
        assert torch.equal(wb[:pairs], ob[:pairs]) and torch.equal(wp[:pairs], op[:pairs]), "window != pair probe"
        del wb, wp
        variants = {"pair probe": pair_probe, "plan": make_plan, "window full": lambda: windows(cap)}
        for size in WINDOWS:
            variants[f"windows {size}"] = lambda size=size: windows(size)
            variants[f"plan + windows {size}"] = lambda size=size: plan_and_windows(size)
        res = rounds(variants, args.warmup, args.reps)
        print(f"{name}: build {B} rows ({'direct-addressed' if st['buckets'] == 0 else 'hashed'}, "
              f"{st['distinct_keys']} keys, max {st['max_key_rows']} rows per key), probe {n} rows, pairs {pairs}, "
              f"plan {plan.numel() / 1e6:.1f} MB, full pair buffers {12 * pairs / 1e6:.1f} MB", flush=True)
        probe_ms = res["pair probe"][0]
        line("hj_probe_async (all pairs at once)", res["pair probe"], pairs)
        line("hj_pair_plan", res["plan"], None, f"{n / res['plan'][0] / 1e6:.2f} Grows/s")
        line("hj_pair_window, one window of all pairs", res["window full"], pairs)
        for size in WINDOWS:
            k = -(-pairs // size)
            line(f"hj_pair_window x {k} (windows of 2^{size.bit_length() - 1})", res[f"windows {size}"], pairs,
                 f"buffers {12 * min(size, cap) / 1e6:.1f} MB")
            both = res[f"plan + windows {size}"]
            line(f"plan + windows of 2^{size.bit_length() - 1}", both, pairs,
                 f"= {both[0] / probe_ms:.2f} x the pair probe's time")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,perkey,sparse", help="comma-separated: c2, c3, perkey, sparse")
    ap.add_argument("--perkey-rows", type=int, default=2_000_000, help="build rows = probe rows of the perkey shape")
    ap.add_argument("--perkey-keys", type=int, default=2000)
    ap.add_argument("--sparse-build-rows", type=int, default=1_000_000)
    ap.add_argument("--sparse-probe-rows", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"# HIP events; every round runs each variant once; median of {args.reps} rounds after {args.warmup} "
          "warm-up rounds, [min .. max]", flush=True)
    for shape in args.shapes.split(","):
        if shape == "perkey":
            # 2000 keys of 1000 build rows each (rows of a key apart: no run refs), probed by
            # 2 * 10^6 rows over twice the key range: 10^9 pairs (12 GB of pair buffers)
            B, K = args.perkey_rows, args.perkey_keys
            bk = torch.arange(B, dtype=torch.int64, device=dev) % K
            g = torch.Generator(device=dev)
            g.manual_seed(2)
            pk = torch.randint(0, 2 * K, (B,), dtype=torch.int64, device=dev, generator=g)
            run_shape(f"perkey: {K} keys of {B // K} build rows", bk, pk, args)
        elif shape == "sparse":
            # distinct build keys; one probe row in 1000 has a partner
            B, P = args.sparse_build_rows, args.sparse_probe_rows
            g = torch.Generator(device=dev)
            g.manual_seed(3)
            bk = torch.randperm(B, device=dev, generator=g).to(torch.int64)
            pk = torch.randint(B, 2 * B, (P,), dtype=torch.int64, device=dev, generator=g)
            pk[::1000] = torch.randint(0, B, (len(pk[::1000]),), dtype=torch.int64, device=dev, generator=g)
            run_shape("sparse: 1 probe row in 1000 matches", bk, pk, args)
        else:
            bk, pk, _, _ = bench.gen_inputs(bench.CONFIGS[shape], 0, 1, dev)
            run_shape(shape, bk, pk, args)
        del bk, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
