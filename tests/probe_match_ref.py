"""numpy restatement of the match probe's contract, written from the text of include/hj.h
("Match probe", hj_select_bitmap): everything is derived from the inner pairs (build_idx,
probe_idx) of the same probe. Shared by the CPU and GPU tests; no GPU and no library call
in here."""
import numpy as np


def bitmap_bytes(n: int) -> int:
    return (n + 63) // 64 * 8


def expected_bitmap(op, n: int) -> np.ndarray:
    """Arrow LSB bitmap of ceil(n / 64) * 8 bytes: bit i set iff some pair has probe_idx i."""
    bits = np.zeros(bitmap_bytes(n) * 8, dtype=bool)
    bits[np.asarray(op, dtype=np.int64)] = True
    return np.packbits(bits, bitorder="little")


def expected_counts(op, n: int) -> np.ndarray:
    return np.bincount(np.asarray(op, dtype=np.int64), minlength=n).astype(np.uint32)


def expected_flags(ob, nflags: int, before=None) -> np.ndarray:
    """The flags before the call (default zeros) OR'ed with hj_mark_rows over the pairs'
    build indices (ids >= nflags skipped)."""
    flags = np.zeros(nflags, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8)
    b = np.asarray(ob).astype(np.uint64)
    flags[b[b < np.uint64(nflags)].astype(np.int64)] = 1
    return flags


def expected_stats(op) -> tuple[int, int]:
    """(set bits of the bitmap, pairs)."""
    op = np.asarray(op)
    return int(len(np.unique(op))), int(len(op))


def expected(ob, op, n: int, nflags: int, before=None) -> dict:
    m, p = expected_stats(op)
    return {"bitmap": expected_bitmap(op, n), "counts": expected_counts(op, n),
            "flags": expected_flags(ob, nflags, before), "matched": m, "pairs": p}


def select_rows(bitmap, n: int, want: int, base: int = 0, bit_offset: int = 0) -> np.ndarray:
    """hj_select_bitmap: ascending base + i, i < n, with bit bit_offset + i == want (uint32)."""
    bits = np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little")[bit_offset:bit_offset + n]
    return (np.flatnonzero(bits == want) + base).astype(np.uint32)


def inner_pairs(build, probe) -> tuple[np.ndarray, np.ndarray]:
    """Inner pairs of two small key lists (None = null, never equal to anything), probe rows
    ascending and each row's build rows descending: the canonical order. By hand, for KATs."""
    ob, op = [], []
    for i, k in enumerate(probe):
        for j in range(len(build) - 1, -1, -1):
            if k is not None and build[j] is not None and build[j] == k:
                ob.append(j)
                op.append(i)
    return np.array(ob, dtype=np.uint64), np.array(op, dtype=np.uint32)
