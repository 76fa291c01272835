"""numpy restatement of the pair plan / pair window contract, written from the text of
include/hj.h ("Pair plan and pair window"): everything is derived from the inner pairs
(build_idx, probe_idx) of the same probe in canonical order. Shared by the CPU and GPU tests;
no GPU and no library call in here."""
import numpy as np

TILE = 2048  # output pairs of one workgroup of the window kernel: the sizes the tests straddle


def written(total: int, lo: int, cap: int) -> int:
    """w = clamp(|S| - pair_lo, 0, capacity)."""
    return max(min(total - lo, cap), 0)


def window(ob, op, lo: int, cap: int, probe_ids=None, probe_base: int = 0):
    """(out_build u64[w], out_probe u32[w], w) of hj_pair_window over the pairs S = (ob, op):
    S[lo + i] for i < w; the probe index goes through probe_ids or has probe_base added
    (mod 2^32 never applies: base + row < 2^32)."""
    ob, op = np.asarray(ob, dtype=np.uint64), np.asarray(op, dtype=np.uint32)
    w = written(len(ob), lo, cap)
    b, p = ob[lo:lo + w], op[lo:lo + w]
    if probe_ids is not None:
        p = np.asarray(probe_ids).view(np.uint32)[p.astype(np.int64)]
    else:
        p = (p.astype(np.uint64) + np.uint64(probe_base)).astype(np.uint32)
    return b, p, w


def cover(total: int, step: int) -> list[tuple[int, int]]:
    """Consecutive windows of `step` pairs that cover [0, total) once."""
    return [(lo, step) for lo in range(0, total, step)]
