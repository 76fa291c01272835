"""Times the device pair filter (hj_pair_filter_test / hj_pair_filter_select) with HIP
events on the candidate pairs of a duplicated-key join (10^6 build rows of 10^5 keys, 10^6
probe rows: about 10^7 pairs), int64 payload columns:

  (a) one EQ term on 8-byte columns, next to hj_filter_equal_pairs on the same pairs and the
      same two columns (its nearest device relative: the same gathers) and to the host
      callable path (operator._apply_filter with a JoinFilter; the events span its copies
      and its pyarrow work, so that figure is wall time);
  (b) a two-term band R.ts >= L.lo AND R.ts < L.hi at selectivities near 0, 0.5 and 1;
  (c) a string != on Utf8 columns.

All variants alternate within one process: every round runs each of them once; warm-up
rounds, then the median of --reps rounds and [min .. max].

    python tools/pair_filter_bench.py > profiles/pair_filter.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from datafusion_parallelism_amd import HashTable, _lib  # noqa: E402
from datafusion_parallelism_amd import operator as opm  # noqa: E402
from datafusion_parallelism_amd.columns import (DeviceColumn, PairPredicate, _key_columns)  # noqa: E402
from match_probe_bench import rounds  # noqa: E402


def line(name: str, ms, pairs: int, note: str = "") -> None:
    med, lo, hi = ms
    print(f"  {name:<52s} {med * 1e3:10.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  spread {(hi - lo) / med * 100:5.1f} %  "
          f"{pairs / med / 1e6:7.2f} Gpairs/s  {note}", flush=True)


def i64col(t: torch.Tensor) -> DeviceColumn:
    return DeviceColumn(pa.int64(), t.numel(), data=t.view(torch.uint8))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-rows", type=int, default=1_000_000)
    ap.add_argument("--probe-rows", type=int, default=1_000_000)
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.load()
    s = torch.cuda.current_stream(dev).cuda_stream or None
    B, P, K = args.build_rows, args.probe_rows, args.keys
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    bk = torch.arange(B, dtype=torch.int64, device=dev) % K
    pk = torch.randint(0, K, (P,), dtype=torch.int64, device=dev, generator=g)
    with HashTable(1, "int64", 0) as t:
        t.build(bk)
        b, p = t.probe(pk, None, device_output=True)
    b, p = b.contiguous(), p.contiguous()
    n = b.numel()
    rnd = lambda lo, hi, m: torch.randint(lo, hi, (m,), dtype=torch.int64, device=dev, generator=g)
    bv, pv = rnd(0, 4, B), rnd(0, 4, P)                      # (a): equal for about 1 pair in 4
    ts = rnd(0, 1000, P)
    lo = {"0": torch.full((B,), 2000, dtype=torch.int64, device=dev), "0.5": rnd(0, 1000, B),
          "1": torch.full((B,), -1, dtype=torch.int64, device=dev)}
    hi = torch.full((B,), 2000, dtype=torch.int64, device=dev)
    vocab = np.array([f"value-{i:04d}" for i in range(64)])
    rs = np.random.default_rng(4)
    bs = DeviceColumn.from_arrow(pa.array(vocab[rs.integers(0, 64, B)]), dev)
    ps = DeviceColumn.from_arrow(pa.array(vocab[rs.integers(0, 64, P)]), dev)

    ob = torch.empty(n, dtype=torch.int64, device=dev)
    op = torch.empty(n, dtype=torch.int32, device=dev)
    bm = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_pair_filter_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ews = torch.empty(L.hj_equal_pairs_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def select(pred):
        return lambda: _lib.check(L.hj_pair_filter_select(pred.struct, b.data_ptr(), p.data_ptr(), n, ob.data_ptr(),
                                                          op.data_ptr(), cnt.data_ptr(), ws.data_ptr(), s))

    def test(pred):
        return lambda: _lib.check(L.hj_pair_filter_test(pred.struct, b.data_ptr(), p.data_ptr(), n, bm.data_ptr(),
                                                        cnt.data_ptr(), s))

    eq = PairPredicate([i64col(bv)], [i64col(pv)], [(("build", 0), "==", ("probe", 0))])
    ebc, epc = _key_columns([i64col(bv)]), _key_columns([i64col(pv)])

    def equal_pairs():
        _lib.check(L.hj_filter_equal_pairs(1, ebc, epc, b.data_ptr(), p.data_ptr(), n, ob.data_ptr(), op.data_ptr(),
                                           cnt.data_ptr(), ews.data_ptr(), s))

    bcols, pcols = [i64col(bv)], [i64col(pv)]
    host_flt = opm.JoinFilter(lambda l, r: pc.equal(l.column("v"), r.column("v")), ["v"], ["v"])

    def host_path():
        opm._apply_filter(host_flt, bcols, ["v"], pcols, ["v"], b, p)

    # the three must agree before anything is timed
    select(eq)()
    m = int(cnt.item())
    sb, sp = ob[:m].clone(), op[:m].clone()
    equal_pairs()
    assert int(cnt.item()) == m and torch.equal(ob[:m], sb) and torch.equal(op[:m], sp), "select != hj_filter_equal_pairs"
    hb, hp = opm._apply_filter(host_flt, bcols, ["v"], pcols, ["v"], b, p)
    assert torch.equal(hb, sb) and torch.equal(hp, sp), "select != host path"
    del sb, sp, hb, hp

    variants = {"a select": select(eq), "a test": test(eq), "equal_pairs": equal_pairs, "host": host_path}
    sel = {"a": m / n}
    for k, lo_t in lo.items():
        band = PairPredicate([i64col(lo_t), i64col(hi)], [i64col(ts)],
                             [(("probe", 0), ">=", ("build", 0)), (("probe", 0), "<", ("build", 1))])
        variants[f"b {k}"] = select(band)
        variants[f"b {k}"]()
        sel[f"b {k}"] = int(cnt.item()) / n
    ne = PairPredicate([bs], [ps], [(("build", 0), "!=", ("probe", 0))])
    variants["c select"] = select(ne)
    variants["c select"]()
    sel["c"] = int(cnt.item()) / n

    res = rounds(variants, args.warmup, args.reps)
    print(f"# HIP events; every round runs each variant once; median of {args.reps} rounds after {args.warmup} "
          "warm-up rounds, [min .. max], spread = (max - min) / median", flush=True)
    print(f"{n} candidate pairs ({B} build rows of {K} keys, {P} probe rows); workspace: pair filter "
          f"{ws.numel() / 1e6:.1f} MB, hj_filter_equal_pairs {ews.numel() / 1e6:.1f} MB", flush=True)
    line(f"(a) select, 1 term EQ int64 (passes {sel['a']:.3f})", res["a select"], n)
    line("(a) test (bitmap + count only)", res["a test"], n)
    line("    hj_filter_equal_pairs, same pairs and columns", res["equal_pairs"], n,
         f"select / equal_pairs = {res['a select'][0] / res['equal_pairs'][0]:.2f}")
    line("    host callable path (wall, copies included)", res["host"], n,
         f"= {res['host'][0] / res['a select'][0]:.0f} x the device select")
    for k in lo:
        line(f"(b) select, band of 2 terms (passes {sel[f'b {k}']:.3f})", res[f"b {k}"], n)
    line(f"(c) select, Utf8 != (passes {sel['c']:.3f})", res["c select"], n)
    a, e = res["a select"], res["equal_pairs"]
    ok = a[0] <= e[0] + (e[2] - e[1])
    print(f"expectation (a) no slower than hj_filter_equal_pairs beyond the latter's spread "
          f"({(e[2] - e[1]) * 1e3:.1f} us; select's own {(a[2] - a[1]) * 1e3:.1f} us): {'holds' if ok else 'FAILS'}", flush=True)


if __name__ == "__main__":
    main()
