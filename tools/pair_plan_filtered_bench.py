"""Times the filtered pair plan (hj_pair_plan_filtered + hj_pair_window_filtered) with HIP
events next to what the operator does without it for the same pairs: the pair probe into
buffers of exactly the candidate count, then hj_pair_filter_select over the candidates. The
baseline is given its candidate count and its filtered count in advance (no second probe, no
host read between its kernels): its best case. The composite-key baseline's extra
hj_filter_equal_pairs pass over all candidates is not included: it only widens the gap.

Shapes: the low-cardinality join of tools/match_filter_bench.py (2000 keys of 1000 build rows,
2 * 10^6 probe rows over twice the key range: 10^9 candidate pairs) under `!=` and under the
two-term band, bench.py's c2 (one pair per match) under `!=`, and the skew shape windowed at
2^20 rows per window: the filtered plan's windows hold passing pairs, the baseline's
(hj_pair_plan + per window hj_pair_window + hj_pair_filter_select) hold candidates. All
variants of a shape and predicate alternate within one process: every round runs each once;
warm-up rounds, then the median of --reps rounds and [min .. max]. Device bytes are the sum of
the buffers each path needs (outputs, plan, workspaces), the table and the inputs left out.

    python tools/pair_plan_filtered_bench.py > profiles/pair_plan_filtered.txt
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
from match_filter_bench import line, predicates  # noqa: E402
from match_probe_bench import rounds  # noqa: E402
from datafusion_parallelism_amd import HashTable, _lib  # noqa: E402


def verdict(new, base) -> str:
    """The comparison the two paths' own spreads allow."""
    ratio = base[0] / new[0]
    if new[1] > base[2]:
        return f"baseline {ratio:.2f} x the filtered plan's time: the filtered plan is slower beyond both spreads"
    if new[2] < base[1]:
        return f"baseline {ratio:.2f} x the filtered plan's time: the filtered plan is faster beyond both spreads"
    return f"baseline {ratio:.2f} x the filtered plan's time: inside the two paths' spreads"


def run_shape(name: str, bk: torch.Tensor, pk: torch.Tensor, args, only: set | None, window: int | None) -> None:
    L = _lib.load()
    dev = pk.device
    s = torch.cuda.current_stream(dev).cuda_stream or None
    B, n = bk.numel(), pk.numel()
    with HashTable(1, "int64", dev.index or 0) as t:
        t.build(bk)
        st = t.stats()
        h = t._h
        plan = torch.empty(t.pair_plan_filtered_bytes(n), dtype=torch.uint8, device=dev)
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        pws = torch.empty(L.hj_probe_workspace_bytes(n), dtype=torch.uint8, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        fcnt = torch.zeros(1, dtype=torch.int64, device=dev)
        print(f"{name}: build {B} rows ({'direct-addressed' if st['buckets'] == 0 else 'hashed'}, "
              f"{st['distinct_keys']} keys, max {st['max_key_rows']} rows per key), probe {n} rows", flush=True)
        for pname, pred in predicates(dev, B, n).items():
            if only is not None and pname not in only:
                continue

            def make_plan():
                _lib.check(L.hj_pair_plan_filtered(h, pk.data_ptr(), None, 0, n, pred.struct, plan.data_ptr(), None,
                                                   None, 0, stats.data_ptr(), s))

            make_plan()
            _, F, S = stats.tolist()
            print(f" {pname}: candidates {S}, passing {F} ({F / max(S, 1):.1%})", flush=True)
            if window is None:
                ob = torch.empty(max(S, 1), dtype=torch.int64, device=dev)
                op = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
                fb = torch.empty(max(S, 1), dtype=torch.int64, device=dev)
                fp = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
                fws = torch.empty(L.hj_pair_filter_workspace_bytes(S), dtype=torch.uint8, device=dev)
                nb = torch.empty(max(F, 1), dtype=torch.int64, device=dev)
                np_ = torch.empty(max(F, 1), dtype=torch.int32, device=dev)

                def new_path():
                    make_plan()
                    _lib.check(L.hj_pair_window_filtered(h, plan.data_ptr(), n, pred.struct, None, 0, 0, F,
                                                         nb.data_ptr(), np_.data_ptr(), written.data_ptr(), s))

                def base_path():
                    _lib.check(L.hj_probe_async(h, pk.data_ptr(), None, 0, n, ob.data_ptr(), op.data_ptr(), max(S, 1),
                                                d_total.data_ptr(), pws.data_ptr(), s))
                    _lib.check(L.hj_pair_filter_select(pred.struct, ob.data_ptr(), op.data_ptr(), S, fb.data_ptr(),
                                                       fp.data_ptr(), fcnt.data_ptr(), fws.data_ptr(), s))

                new_path()
                base_path()
                assert int(d_total.item()) == S and int(fcnt.item()) == F == int(written.item())
                assert torch.equal(nb[:F], fb[:F]) and torch.equal(np_[:F], fp[:F]), "the two paths disagree"
                new_bytes = plan.numel() + 12 * F
                base_bytes = 24 * S + fws.numel() + pws.numel()
                res = rounds({"plan": make_plan, "new": new_path, "base": base_path}, args.warmup, args.reps)
                line("hj_pair_plan_filtered alone", res["plan"])
                line("hj_pair_plan_filtered + one full hj_pair_window_filtered", res["new"],
                     f"{new_bytes / 1e6:.1f} MB ({plan.numel() / max(n, 1):.1f} B / probe row + 12 |F|)")
                line("probe + hj_pair_filter_select", res["base"],
                     f"{base_bytes / 1e6:.1f} MB (24 |S| + workspaces); " + verdict(res["new"], res["base"]))
                del ob, op, fb, fp, fws, nb, np_
            else:
                W = window
                wb = torch.empty(W, dtype=torch.int64, device=dev)
                wp = torch.empty(W, dtype=torch.int32, device=dev)
                fb = torch.empty(W, dtype=torch.int64, device=dev)
                fp = torch.empty(W, dtype=torch.int32, device=dev)
                fws = torch.empty(L.hj_pair_filter_workspace_bytes(W), dtype=torch.uint8, device=dev)
                pplan = torch.empty(t.pair_plan_bytes(n), dtype=torch.uint8, device=dev)

                def new_path():
                    make_plan()
                    for lo in range(0, F, W):
                        _lib.check(L.hj_pair_window_filtered(h, plan.data_ptr(), n, pred.struct, None, 0, lo, W,
                                                             wb.data_ptr(), wp.data_ptr(), written.data_ptr(), s))

                def base_path():
                    _lib.check(L.hj_pair_plan(h, pk.data_ptr(), None, 0, n, pplan.data_ptr(), d_total.data_ptr(), s))
                    for lo in range(0, S, W):
                        _lib.check(L.hj_pair_window(h, pplan.data_ptr(), n, None, 0, lo, W, wb.data_ptr(), wp.data_ptr(),
                                                    written.data_ptr(), s))
                        _lib.check(L.hj_pair_filter_select(pred.struct, wb.data_ptr(), wp.data_ptr(), min(W, S - lo),
                                                           fb.data_ptr(), fp.data_ptr(), fcnt.data_ptr(), fws.data_ptr(),
                                                           s))

                # the two paths agree before anything is timed: both sequences of windows, laid end
                # to end (untimed: the baseline's filtered count is read per window)
                nb, np_ = (torch.empty(max(F, 1), dtype=dt, device=dev) for dt in (torch.int64, torch.int32))
                bb, bp = (torch.empty(max(F, 1), dtype=dt, device=dev) for dt in (torch.int64, torch.int32))
                make_plan()
                for lo in range(0, F, W):
                    _lib.check(L.hj_pair_window_filtered(h, plan.data_ptr(), n, pred.struct, None, 0, lo, W,
                                                         nb.data_ptr() + 8 * lo, np_.data_ptr() + 4 * lo, None, s))
                _lib.check(L.hj_pair_plan(h, pk.data_ptr(), None, 0, n, pplan.data_ptr(), d_total.data_ptr(), s))
                at = 0
                for lo in range(0, S, W):
                    _lib.check(L.hj_pair_window(h, pplan.data_ptr(), n, None, 0, lo, W, wb.data_ptr(), wp.data_ptr(),
                                                written.data_ptr(), s))
                    _lib.check(L.hj_pair_filter_select(pred.struct, wb.data_ptr(), wp.data_ptr(), min(W, S - lo),
                                                       fb.data_ptr(), fp.data_ptr(), fcnt.data_ptr(), fws.data_ptr(), s))
                    k = int(fcnt.item())
                    assert at + k <= F
                    bb[at:at + k] = fb[:k]
                    bp[at:at + k] = fp[:k]
                    at += k
                assert at == F and int(d_total.item()) == S
                assert torch.equal(nb[:F], bb[:F]) and torch.equal(np_[:F], bp[:F]), "the two windowed paths disagree"
                del nb, np_, bb, bp
                new_bytes = plan.numel() + 12 * W
                base_bytes = pplan.numel() + 24 * W + fws.numel()
                res = rounds({"new": new_path, "base": base_path}, args.warmup, args.reps)
                line(f"filtered plan + {-(-F // W)} windows of {W} passing pairs", res["new"], f"{new_bytes / 1e6:.1f} MB")
                line(f"pair plan + {-(-S // W)} x (window of {W} candidates + select)", res["base"],
                     f"{base_bytes / 1e6:.1f} MB; " + verdict(res["new"], res["base"]))
                del wb, wp, fb, fp, fws, pplan


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="skew,c2,skew-windowed", help="comma-separated: skew, c2, skew-windowed")
    ap.add_argument("--skew-rows", type=int, default=2_000_000, help="build rows = probe rows of the skew shape")
    ap.add_argument("--skew-keys", type=int, default=2000)
    ap.add_argument("--window", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"# HIP events; every round runs each variant once; median of {args.reps} rounds after {args.warmup} "
          "warm-up rounds, [min .. max]", flush=True)
    for shape in args.shapes.split(","):
        if shape.startswith("skew"):
            B, K = args.skew_rows, args.skew_keys
            bk = torch.arange(B, dtype=torch.int64, device=dev) % K
            g = torch.Generator(device=dev)
            g.manual_seed(2)
            pk = torch.randint(0, 2 * K, (B,), dtype=torch.int64, device=dev, generator=g)
            windowed = shape == "skew-windowed"
            run_shape(f"skew{' windowed' if windowed else ''}: {K} keys of {B // K} build rows", bk, pk, args,
                      {"R.ts >= L.lo AND R.ts < L.hi"} if windowed else None, args.window if windowed else None)
        else:
            bk, pk, _, _ = bench.gen_inputs(bench.CONFIGS[shape], 0, 1, dev)
            run_shape(shape, bk, pk, args, {"L.v != R.v"}, None)
        del bk, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
