"""numpy restatement of the pair filter's contract, written from the text of include/hj.h
("pair filter") only: the range rule, nulls, the widening, the float key, unsigned-byte
order, the bitmap layout. Test helper; not part of the product.

A fixed-width column is a numpy array whose dtype gives class and width (int8..int64,
uint8..uint64, float32 / float64); a BYTES column is a list of bytes objects. `valid` is a
bool array (True = valid) or None.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EQ, NE, LT, LE, GT, GE = range(6)
INT, UINT, FLOAT, BYTES = range(4)
BUILD, PROBE, CONST = range(3)
OPS = {"==": EQ, "!=": NE, "<": LT, "<=": LE, ">": GT, ">=": GE}
INT64_MAX = np.int64(2**63 - 1)


@dataclass
class Col:
    values: object                  # np.ndarray (fixed width) or list[bytes]
    valid: np.ndarray | None = None


@dataclass
class Term:
    op: int
    cls: int
    lhs: tuple                      # (BUILD | PROBE, column index)
    rhs: tuple                      # (BUILD | PROBE, column index) or (CONST, int64 bits)


def float_key(x: np.ndarray) -> np.ndarray:
    """b ^ ((b >> 63) & INT64_MAX) of the doubles' bits, compared as signed."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return b ^ ((b >> np.int64(63)) & INT64_MAX)


def const_bits(cls: int, v) -> int:
    """rhs_const (as a signed int64) of a Python constant."""
    if cls == FLOAT:
        return int(np.float64(v).view(np.int64))
    if cls == UINT:
        return int(np.uint64(v).view(np.int64))
    return int(v)


def _fixed_key(cls: int, values: np.ndarray):
    """Keys whose order is the class's: int64 (INT, FLOAT) or uint64 (UINT)."""
    if cls == INT:
        assert values.dtype.kind == "i"
        return values.astype(np.int64)       # sign extension
    if cls == UINT:
        assert values.dtype.kind == "u"
        return values.astype(np.uint64)      # zero extension
    assert values.dtype in (np.float32, np.float64)
    return float_key(values.astype(np.float64))  # a float32 is widened to double


def _const_key(cls: int, bits: int):
    b = np.array([bits], dtype=np.int64)
    if cls == INT:
        return b
    if cls == UINT:
        return b.view(np.uint64)
    return float_key(b.view(np.float64))


def _compare(op: int, x, y):
    return [x == y, x != y, x < y, x <= y, x > y, x >= y][op]


def pair_pass(terms, build_cols, probe_cols, build_rows: int, probe_rows: int, bidx, pidx) -> np.ndarray:
    """bool[n]: pair i passes iff both indices are in range and every term is true; an
    out-of-range index is never dereferenced; a term with a null operand is not true."""
    bidx = np.asarray(bidx).astype(np.uint64)
    pidx = np.asarray(pidx).astype(np.uint32)
    ok = (bidx < np.uint64(build_rows)) & (pidx.astype(np.int64) < probe_rows)
    rows = {BUILD: np.where(ok, bidx, 0).astype(np.int64), PROBE: np.where(ok, pidx, 0).astype(np.int64)}
    cols = {BUILD: build_cols, PROBE: probe_cols}
    for t in terms:
        lc, lr = cols[t.lhs[0]][t.lhs[1]], rows[t.lhs[0]]
        live = ok.copy()
        if lc.valid is not None:
            live &= np.where(ok, lc.valid[lr * ok], False)
        rc = rr = None
        if t.rhs[0] != CONST:
            rc, rr = cols[t.rhs[0]][t.rhs[1]], rows[t.rhs[0]]
            if rc.valid is not None:
                live &= np.where(ok, rc.valid[rr * ok], False)
        res = np.zeros(len(bidx), dtype=bool)
        idx = np.nonzero(live)[0]
        if t.cls == BYTES:
            assert rc is not None, "BYTES takes no constant"
            for i in idx:
                x, y = bytes(lc.values[lr[i]]), bytes(rc.values[rr[i]])  # Python orders bytes as unsigned, prefix first
                res[i] = _compare(t.op, x, y)
        else:
            x = _fixed_key(t.cls, np.asarray(lc.values)[lr[idx]])
            y = _const_key(t.cls, t.rhs[1]) if rc is None else _fixed_key(t.cls, np.asarray(rc.values)[rr[idx]])
            res[idx] = _compare(t.op, x, y)
        ok = ok & res
    return ok


def bitmap(passes: np.ndarray) -> np.ndarray:
    """Arrow LSB bitmap of ceil(n / 64) * 8 bytes, bits at and beyond n zero."""
    n = len(passes)
    bits = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    bits[:n] = passes
    return np.packbits(bits, bitorder="little")


def select(passes: np.ndarray, bidx, pidx):
    return np.asarray(bidx)[passes], np.asarray(pidx)[passes]
