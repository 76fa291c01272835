"""Times the key filter's kernels alone (hj_key_filter_add / _test / _select) with HIP
events on the shapes of C4's dominant join, orders ⋈ lineitem of TPC-H Q3 at SF100
(DESIGN.md §5a): 14.6 M build keys spread over a 600 M-value range, 323 M probe keys once
clustered by key and once shuffled, for the RANGE and the BLOOM layout. Warm-up, then the
median of --reps runs; each line carries its algorithmic bytes and the rate they give.

    python tools/key_filter_bench.py > profiles/key_filter_kernels.txt

add is timed on a freshly zeroed filter every run (a filled one skips every atomic).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datafusion_parallelism_amd import KeyFilter, _lib  # noqa: E402


def order_key(i: torch.Tensor) -> torch.Tensor:
    """TPC-H's sparse order keys: 8 consecutive values of every 32."""
    return (i // 8) * 32 + i % 8 + 1


def median_ms(fn, setup, warmup: int, reps: int) -> tuple[float, float, float]:
    ts = []
    for r in range(warmup + reps):
        state = setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
        del state
    return float(np.median(ts)), min(ts), max(ts)


def line(name: str, ms: tuple[float, float, float], alg_bytes: int, note: str = "") -> None:
    med, lo, hi = ms
    print(f"{name:<44s} {med * 1e3:10.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  alg {alg_bytes / 1e6:10.1f} MB"
          f"  {alg_bytes / med / 1e6:8.1f} GB/s  {note}", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-rows", type=int, default=14_600_000)
    ap.add_argument("--probe-rows", type=int, default=323_000_000)
    ap.add_argument("--orders", type=int, default=150_000_000, help="order keys of the domain (4 values per key)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream or None
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    B, P = args.build_rows, args.probe_rows
    # the build side: a random tenth of the orders (even order numbers), in key order, and
    # the same rows shuffled; the probe side: 99 % rows of orders that are not in the build
    # (odd order numbers), 1 % rows of build orders - C4's match rate
    half = args.orders // 2
    bidx = 2 * torch.randint(0, half, (B,), device=dev, generator=g).sort().values
    build = {"clustered": order_key(bidx)}
    build["shuffled"] = build["clustered"][torch.randperm(B, device=dev, generator=g)]
    lo, hi = int(build["clustered"].min()), int(build["clustered"].max())
    pidx = 2 * torch.randint(0, half, (P,), device=dev, generator=g) + 1
    nhit = P // 100
    pidx[:nhit] = bidx[torch.randint(0, B, (nhit,), device=dev, generator=g)]
    del bidx
    probe = {"clustered": order_key(pidx.sort().values)}
    del pidx
    probe["shuffled"] = probe["clustered"][torch.randperm(P, device=dev, generator=g)]
    print(f"# build {B} keys in [{lo}, {hi}] ({(hi - lo + 1) / B:.1f} values per key), probe {P} keys; "
          f"median of {args.reps} after {args.warmup} warm-up runs, [min .. max]", flush=True)

    out_keys = torch.empty(P, dtype=torch.int64, device=dev)
    out_ids = torch.empty(P, dtype=torch.int32, device=dev)
    bitmap = torch.empty((P + 63) // 64, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_key_filter_select_workspace_bytes(P) + 8, dtype=torch.uint8, device=dev)

    for kind in ("range", "bloom"):
        for order, bk in build.items():
            def add(f, bk=bk):
                _lib.check(L.hj_key_filter_add(f._h, _lib.HJ_INT64, bk.data_ptr(), None, 0, B, stream))

            ms = median_ms(add, lambda: KeyFilter(0, kind, lo, hi, B), args.warmup, args.reps)
            with KeyFilter(0, kind, lo, hi, B) as f:
                nwords = f.info()["nwords"]
            line(f"{kind:5s} add    build {order:9s}", ms, 8 * B + 8 * nwords, f"filter {nwords * 8 / 1e6:.1f} MB")
        with KeyFilter(0, kind, lo, hi, B) as f:
            f.add(build["clustered"])
            for order, pk in probe.items():
                def test(_, pk=pk):
                    _lib.check(L.hj_key_filter_test(f._h, _lib.HJ_INT64, pk.data_ptr(), None, 0, P, bitmap.data_ptr(),
                                                    cnt.data_ptr(), stream))

                ms = median_ms(test, lambda: None, args.warmup, args.reps)
                passing = int(cnt.item())
                line(f"{kind:5s} test   probe {order:9s}", ms, 8 * P + P // 8, f"passing {passing} ({passing / P:.2%})")

                def select(_, pk=pk):
                    _lib.check(L.hj_key_filter_select(f._h, _lib.HJ_INT64, pk.data_ptr(), None, 0, P, 0,
                                                      out_keys.data_ptr(), out_ids.data_ptr(), cnt.data_ptr(),
                                                      ws.data_ptr(), stream))

                ms = median_ms(select, lambda: None, args.warmup, args.reps)
                passing = int(cnt.item())
                line(f"{kind:5s} select probe {order:9s}", ms, 8 * P + 12 * passing,
                     f"passing {passing} ({passing / P:.2%})")


if __name__ == "__main__":
    main()
