"""Device-resident Arrow columns and the index primitives of the join types
(SURVEY.md §8f rows f1 and f2), over the C ABI's hj_gather_* / hj_mark_rows /
hj_select_rows kernels.

  reference                                                   here
  ---------------------------------------------------------   ------------------------------
  take_multiple_record_batch (src/shared/shared.rs:83-92)     DeviceColumn.take
  ConcurrentBitSet::set_ones (src/utils/concurrent_bit_set.rs:28-60)
                                                              mark_rows
  get_set_indices_array / get_unset_indices_array,
  get_semi_indices / get_anti_indices
    (src/shared/datafusion_private.rs:85-135)                 select_rows

Index tensors: int64 (build side, the reference's UInt64) or int32 (probe side, UInt32);
-1 is a null index (the outer joins' missing side). Buffers move between host and HBM
only in `from_arrow` / `to_arrow`; the gathers run on the GPU (no CPU fallback).
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import pyarrow as pa
import torch

from . import _lib
from ._lib import check

_VAR = {pa.string(): 4, pa.binary(): 4, pa.large_string(): 8, pa.large_binary(): 8}


def _is_var(t: pa.DataType) -> bool:
    return t in _VAR


def _fixed_width(t: pa.DataType) -> int:
    if pa.types.is_boolean(t):
        return 1  # held as one byte per value on the device
    try:
        w = t.bit_width
    except ValueError as e:
        raise TypeError(f"column type {t} is not supported on the device") from e
    if w % 8 or w // 8 not in (1, 2, 4, 8, 16):
        raise TypeError(f"column type {t} is not supported on the device")
    return w // 8


def _to_device(buf: np.ndarray, device) -> torch.Tensor:
    # Arrow buffers are read-only; the host tensor is only read by the copy to HBM
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        host = torch.from_numpy(np.ascontiguousarray(buf))
    return host.to(device)


def _bitmap_bytes(n: int) -> int:
    return ((n + 63) // 64) * 8


def _stream(device) -> int | None:
    return torch.cuda.current_stream(device).cuda_stream or None


@dataclass
class DeviceColumn:
    """One Arrow column in HBM: `data` (fixed width) or `offsets` + `values` (Utf8 /
    Binary, 4- or 8-byte offsets), optional LSB validity bitmap starting at bit `voff`."""
    type: pa.DataType
    length: int
    data: torch.Tensor | None = None
    offsets: torch.Tensor | None = None
    values: torch.Tensor | None = None
    valid: torch.Tensor | None = None
    voff: int = 0

    @property
    def device(self):
        t = self.data if self.data is not None else self.offsets
        return t.device

    @classmethod
    def from_arrow(cls, arr: pa.Array | pa.ChunkedArray, device) -> "DeviceColumn":
        if isinstance(arr, pa.ChunkedArray):
            arr = arr.combine_chunks()
        t, n, off = arr.type, len(arr), arr.offset
        bufs = arr.buffers()
        valid = None
        voff = 0
        if arr.null_count > 0 and bufs[0] is not None:
            vb = np.frombuffer(bufs[0], dtype=np.uint8)
            valid, voff = _to_device(vb, device), off
        if _is_var(t):
            ob = _VAR[t]
            odt = np.int32 if ob == 4 else np.int64
            offs = np.frombuffer(bufs[1], dtype=odt)[off:off + n + 1]
            vals = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
            return cls(t, n, offsets=_to_device(offs, device), values=_to_device(vals if vals.size else
                                                                                np.zeros(1, np.uint8), device),
                       valid=valid, voff=voff)
        if pa.types.is_boolean(t):
            data = np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), dtype=np.uint8)
            return cls(t, n, data=_to_device(data if n else np.zeros(1, np.uint8), device), valid=valid, voff=voff)
        w = _fixed_width(t)
        raw = np.frombuffer(bufs[1], dtype=np.uint8)[off * w:(off + n) * w]
        return cls(t, n, data=_to_device(raw if raw.size else np.zeros(w, np.uint8), device), valid=valid,
                   voff=voff)

    def take(self, idx: torch.Tensor) -> "DeviceColumn":
        """Arrow take by device indices (int32 / int64, -1 = null) on the GPU."""
        L = _lib.load()
        if idx.dtype not in (torch.int32, torch.int64):
            raise TypeError("indices must be int32 or int64")
        idx = idx.contiguous()
        n = idx.numel()
        dev = self.device
        ib = 8 if idx.dtype == torch.int64 else 4
        dvalid = torch.empty(max(_bitmap_bytes(n), 8), dtype=torch.uint8, device=dev)
        vptr = self.valid.data_ptr() if self.valid is not None else None
        s = _stream(dev)
        if _is_var(self.type):
            ob = _VAR[self.type]
            out_off = torch.empty(n + 1, dtype=torch.int32 if ob == 4 else torch.int64, device=dev)
            ws = torch.empty(L.hj_gather_var_workspace_bytes(n), dtype=torch.uint8, device=dev)
            d_len = torch.zeros(1, dtype=torch.int64, device=dev)
            cap = max(int(self.values.numel()), 1) if n else 1
            for _ in range(2):
                out_val = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                check(L.hj_gather_var(self.offsets.data_ptr(), ob, self.values.data_ptr(), vptr, self.voff,
                                      idx.data_ptr() if n else None, ib, n, out_off.data_ptr(), out_val.data_ptr(),
                                      cap, dvalid.data_ptr(), d_len.data_ptr(), ws.data_ptr(), s))
                need = int(d_len.item())
                if need <= cap:
                    break
                cap = need
            if ob == 4 and need >= 2**31:
                raise _lib.HjError(_lib.HJ_ERR_CAPACITY, "gathered Utf8 column exceeds 2^31 bytes: use LargeUtf8")
            return DeviceColumn(self.type, n, offsets=out_off, values=out_val, valid=dvalid, voff=0)
        w = _fixed_width(self.type)
        dst = torch.empty(max(n * w, w), dtype=torch.uint8, device=dev)
        check(L.hj_gather_fixed(self.data.data_ptr(), vptr, self.voff, w, idx.data_ptr() if n else None, ib, n,
                                dst.data_ptr(), dvalid.data_ptr(), s))
        return DeviceColumn(self.type, n, data=dst, valid=dvalid, voff=0)

    def key_tensor(self) -> torch.Tensor:
        """An Int32 / Int64 column's values as a device tensor (no copy)."""
        if pa.types.is_int64(self.type):
            return self.data.view(torch.int64)[: self.length]
        if pa.types.is_int32(self.type):
            return self.data.view(torch.int32)[: self.length]
        raise TypeError(f"{self.type} is not an Int32/Int64 key column")

    def valid_bools(self) -> torch.Tensor | None:
        """The validity bitmap as one bool per row (device), or None without nulls."""
        if self.valid is None:
            return None
        i = torch.arange(self.length, dtype=torch.int64, device=self.device) + self.voff
        return ((self.valid[i >> 3] >> (i & 7).to(torch.uint8)) & 1).bool()

    @classmethod
    def concat(cls, cols: list["DeviceColumn"]) -> "DeviceColumn":
        """Arrow concat of columns of one type, on the device (the build side's
        cooperative concatenation in canonical order,
        src/operator/version10/parallel_join_execution_state.rs:256-298,317-347): fixed
        width values and Utf8/Binary values are copied device to device, offsets re-based,
        validity bitmaps re-packed from bit 0. One host read: the value ranges of the
        variable-width pieces."""
        if not cols:
            raise ValueError("concat of no columns")
        t = cols[0].type
        if any(c.type != t for c in cols):
            raise TypeError("concat of columns of different types")
        if len(cols) == 1 and cols[0].voff == 0:
            return cols[0]
        n = sum(c.length for c in cols)
        dev = cols[0].device
        valid = None
        if any(c.valid is not None for c in cols):
            bits = torch.cat([c.valid_bools() if c.valid is not None
                              else torch.ones(c.length, dtype=torch.bool, device=dev) for c in cols])
            pad = torch.zeros(_bitmap_bytes(n) * 8, dtype=torch.uint8, device=dev)
            pad[:n] = bits.to(torch.uint8)
            w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
            valid = (pad.view(-1, 8) * w).sum(1, dtype=torch.int32).to(torch.uint8)
            if valid.numel() < 8:
                valid = torch.cat([valid, torch.zeros(8 - valid.numel(), dtype=torch.uint8, device=dev)])
        if _is_var(t):
            bounds = torch.stack([torch.stack([c.offsets[0], c.offsets[c.length]]) for c in cols]).to(torch.int64)
            b = bounds.tolist()  # the one host read
            offs, vals, base = [], [], 0
            for c, (a, e) in zip(cols, b):
                offs.append(c.offsets[: c.length].to(torch.int64) - a + base)
                vals.append(c.values[a:e])
                base += e - a
            odt = cols[0].offsets.dtype
            offs.append(torch.tensor([base], dtype=torch.int64, device=dev))
            values = torch.cat(vals) if base else torch.zeros(1, dtype=torch.uint8, device=dev)
            return cls(t, n, offsets=torch.cat(offs).to(odt), values=values, valid=valid, voff=0)
        w = _fixed_width(t)
        data = torch.cat([c.data[: c.length * w] for c in cols])
        if data.numel() == 0:
            data = torch.zeros(w, dtype=torch.uint8, device=dev)
        return cls(t, n, data=data, valid=valid, voff=0)

    def to_arrow(self) -> pa.Array:
        n, t = self.length, self.type
        vbuf = None
        if self.valid is not None:
            vb = self.valid.cpu().numpy()
            if self.voff:  # re-base the bitmap at bit 0
                bits = np.unpackbits(vb, bitorder="little")[self.voff:self.voff + n]
                vb = np.packbits(bits, bitorder="little")
            vbuf = pa.py_buffer(vb.tobytes())
        if _is_var(t):
            offs = self.offsets.cpu().numpy()
            vals = self.values.cpu().numpy()[: int(offs[-1]) if n else 0]
            return pa.Array.from_buffers(t, n, [vbuf, pa.py_buffer(offs.tobytes()), pa.py_buffer(vals.tobytes())])
        raw = self.data.cpu().numpy()
        if pa.types.is_boolean(t):
            bits = np.packbits(raw[:n].astype(bool), bitorder="little")
            return pa.Array.from_buffers(t, n, [vbuf, pa.py_buffer(bits.tobytes())])
        w = _fixed_width(t)
        return pa.Array.from_buffers(t, n, [vbuf, pa.py_buffer(raw[: n * w].tobytes())])


def _key_column(c: DeviceColumn) -> "_lib.HjKeyColumn":
    """hj_key_column of a device column (fixed width or Utf8 / Binary)."""
    vptr = c.valid.data_ptr() if c.valid is not None else None
    if _is_var(c.type):
        return _lib.HjKeyColumn(c.values.data_ptr(), c.offsets.data_ptr(), vptr, c.voff, 0, _VAR[c.type])
    return _lib.HjKeyColumn(c.data.data_ptr(), None, vptr, c.voff, _fixed_width(c.type), 0)


def _key_columns(cols: list[DeviceColumn]):
    arr = (_lib.HjKeyColumn * len(cols))()
    for i, c in enumerate(cols):
        arr[i] = _key_column(c)
    return arr


def composite_keys(cols: list[DeviceColumn]) -> tuple[torch.Tensor, torch.Tensor]:
    """hj_composite_keys: one int64 key per row from every key column (calculate_hash over
    all key columns, src/shared/shared.rs:11-16) and the LSB validity bitmap (uint8
    device tensor, bit i = no key column null at row i)."""
    L = _lib.load()
    n = cols[0].length
    if any(c.length != n for c in cols):
        raise ValueError("key columns of unequal length")
    dev = cols[0].device
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    valid = torch.zeros(max(_bitmap_bytes(n), 8), dtype=torch.uint8, device=dev)
    check(L.hj_composite_keys(len(cols), _key_columns(cols), n, keys.data_ptr(), valid.data_ptr(), _stream(dev)))
    return keys[:n], valid


def filter_equal_pairs(build_cols: list[DeviceColumn], probe_cols: list[DeviceColumn], b: torch.Tensor,
                       p: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """hj_filter_equal_pairs (equal_rows_arr, src/shared/datafusion_private.rs:52-73): the
    candidate pairs whose key tuples are equal in every column, order kept."""
    L = _lib.load()
    n = b.numel()
    dev = b.device
    ob = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    op = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_equal_pairs_workspace_bytes(n), dtype=torch.uint8, device=dev)
    b, p = b.contiguous(), p.contiguous()
    check(L.hj_filter_equal_pairs(len(build_cols), _key_columns(build_cols), _key_columns(probe_cols),
                                  b.data_ptr() if n else None, p.data_ptr() if n else None, n, ob.data_ptr(),
                                  op.data_ptr(), cnt.data_ptr(), ws.data_ptr(), _stream(dev)))
    m = int(cnt.item())
    return ob[:m], op[:m]


_CMP_OPS = {"==": _lib.HJ_CMP_EQ, "=": _lib.HJ_CMP_EQ, "!=": _lib.HJ_CMP_NE, "<>": _lib.HJ_CMP_NE,
            "<": _lib.HJ_CMP_LT, "<=": _lib.HJ_CMP_LE, ">": _lib.HJ_CMP_GT, ">=": _lib.HJ_CMP_GE}


def _value_class(t: pa.DataType) -> int:
    """The pair filter's value class (HJ_VAL_*) of an Arrow type; TypeError for a type the
    device does not compare (float16, decimals, nested types, ...)."""
    ty = pa.types
    if ty.is_boolean(t) or ty.is_unsigned_integer(t):
        return _lib.HJ_VAL_UINT  # a boolean is one byte, 0 / 1, on the device
    if ty.is_signed_integer(t) or ty.is_date(t) or ty.is_timestamp(t) or ty.is_time(t) or ty.is_duration(t):
        return _lib.HJ_VAL_INT
    if ty.is_float32(t) or ty.is_float64(t):
        return _lib.HJ_VAL_FLOAT
    if _is_var(t):
        return _lib.HJ_VAL_BYTES
    raise TypeError(f"the device pair filter does not compare values of type {t}")


def _plain_number(t: pa.DataType) -> bool:
    return pa.types.is_integer(t) or pa.types.is_floating(t)


class PairPredicate:
    """An hj_pair_predicate over device columns: a conjunction of comparisons on the pairs
    (build row, probe row). `terms`: (lhs, op, rhs) with lhs = ("build", i) or ("probe", i),
    an index into `build_cols` / `probe_cols`; op one of == != < <= > >= (also = and <>);
    rhs a column reference like lhs, or a Python scalar (a constant). The Arrow types choose
    the value class: ints INT, uints and booleans UINT, float32 / float64 FLOAT (IEEE
    totalOrder), date / timestamp / time / duration INT of their width (both operands of one
    Arrow type), Utf8 / LargeUtf8 / Binary / LargeBinary BYTES (no constants). Anything else
    - float16, decimals, signed against unsigned, int against float, a boolean against a
    number - raises TypeError here: there is no host fallback. The object keeps the ctypes
    arrays and the columns alive; `struct` is what the C ABI takes."""

    def __init__(self, build_cols: list[DeviceColumn], probe_cols: list[DeviceColumn], terms,
                 build_rows: int | None = None, probe_rows: int | None = None):
        terms = list(terms)
        if not 1 <= len(terms) <= 16:
            raise ValueError("a pair predicate has 1..16 terms")
        if len(build_cols) > 16 or len(probe_cols) > 16:
            raise ValueError("a pair predicate reads at most 16 columns of each side")
        self.build_cols, self.probe_cols = list(build_cols), list(probe_cols)
        sides = {"build": (_lib.HJ_SIDE_BUILD, self.build_cols), "probe": (_lib.HJ_SIDE_PROBE, self.probe_cols)}

        def column(ref):
            if not (isinstance(ref, tuple) and len(ref) == 2 and ref[0] in sides):
                return None
            side, cols = sides[ref[0]]
            if not 0 <= ref[1] < len(cols):
                raise IndexError(f"{ref[0]} column {ref[1]} is outside the predicate's columns")
            return side, int(ref[1]), cols[ref[1]]

        self._terms = (_lib.HjPairTerm * len(terms))()
        for k, (lhs, op, rhs) in enumerate(terms):
            if op not in _CMP_OPS:
                raise ValueError(f"term {k}: unknown comparison {op!r}")
            lc = column(lhs)
            if lc is None:
                raise TypeError(f"term {k}: the left operand must be a column")
            cls = _value_class(lc[2].type)
            rc = column(rhs)
            if rc is not None:
                lt, rt = lc[2].type, rc[2].type
                if _value_class(rt) != cls or (not (_plain_number(lt) and _plain_number(rt)) and lt != rt
                                               and not (_is_var(lt) and _is_var(rt))):
                    raise TypeError(f"term {k}: the device pair filter does not compare {lt} with {rt}")
                self._terms[k] = _lib.HjPairTerm(_CMP_OPS[op], cls, lc[0], lc[1], rc[0], rc[1], 0)
            else:
                self._terms[k] = _lib.HjPairTerm(_CMP_OPS[op], cls, lc[0], lc[1], _lib.HJ_SIDE_CONST, 0,
                                                 _encode_constant(rhs, lc[2].type, cls, k))
        self._bcols = _key_columns(self.build_cols) if self.build_cols else None
        self._pcols = _key_columns(self.probe_cols) if self.probe_cols else None

        def rows(given, cols, side):
            if given is not None:
                return int(given)
            if not cols:  # no column to take it from, and 0 would fail every pair
                raise ValueError(f"{side}_rows is needed when the predicate reads no {side} column")
            return cols[0].length

        self.struct = _lib.HjPairPredicate(
            len(terms), self._terms, len(self.build_cols), self._bcols, rows(build_rows, self.build_cols, "build"),
            len(self.probe_cols), self._pcols, rows(probe_rows, self.probe_cols, "probe"))
        if any(c.length < self.struct.build_rows for c in self.build_cols) or \
                any(c.length < self.struct.probe_rows for c in self.probe_cols):
            raise ValueError("a predicate column is shorter than its side's row count")

    @property
    def device(self):
        return (self.build_cols or self.probe_cols)[0].device


def _encode_constant(v, t: pa.DataType, cls: int, k: int) -> int:
    """rhs_const of a Python scalar compared with a column of type t (as a signed int64)."""
    if cls == _lib.HJ_VAL_BYTES:
        raise TypeError(f"term {k}: the device pair filter takes no string / binary constants")
    if isinstance(v, np.generic):
        v = v.item()
    if cls == _lib.HJ_VAL_FLOAT:
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"term {k}: a {t} column needs a number, not {type(v).__name__}")
        return int(np.float64(v).view(np.int64))
    if pa.types.is_boolean(t):
        if not isinstance(v, bool):
            raise TypeError(f"term {k}: a boolean column needs a bool constant")
        return int(v)
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"term {k}: a {t} column needs an int constant, not {type(v).__name__}")
    if cls == _lib.HJ_VAL_UINT:
        if not 0 <= v < 2**64:
            raise TypeError(f"term {k}: {v} is not an unsigned 64-bit value")
        return v - 2**64 if v >= 2**63 else v
    if not -2**63 <= v < 2**63:
        raise TypeError(f"term {k}: {v} is not a signed 64-bit value")
    return v


def _pair_args(pred: PairPredicate, b: torch.Tensor, p: torch.Tensor):
    if b.dtype != torch.int64 or p.dtype != torch.int32 or b.numel() != p.numel():
        raise TypeError("pairs are an int64 build and an int32 probe index tensor of one length")
    return b.contiguous(), p.contiguous(), b.numel(), b.device


def pair_filter_test(pred: PairPredicate, b: torch.Tensor, p: torch.Tensor) -> tuple[torch.Tensor, int]:
    """hj_pair_filter_test: the Arrow LSB bitmap (uint8 device tensor, ceil(n / 64) * 8
    bytes) of the candidate pairs that pass the predicate, and their number."""
    L = _lib.load()
    b, p, n, dev = _pair_args(pred, b, p)
    bitmap = torch.empty(max(_bitmap_bytes(n), 8), dtype=torch.uint8, device=dev)
    if n == 0:
        bitmap.zero_()
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    check(L.hj_pair_filter_test(pred.struct, b.data_ptr() if n else None, p.data_ptr() if n else None, n,
                                bitmap.data_ptr(), cnt.data_ptr(), _stream(dev)))
    return bitmap, int(cnt.item())


def pair_filter_select(pred: PairPredicate, b: torch.Tensor, p: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """hj_pair_filter_select (apply_join_filter_to_indices,
    src/shared/datafusion_private.rs:295-328): the candidate pairs that pass the predicate,
    order kept. Only the count comes to the host."""
    L = _lib.load()
    b, p, n, dev = _pair_args(pred, b, p)
    ob = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    op = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_pair_filter_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(L.hj_pair_filter_select(pred.struct, b.data_ptr() if n else None, p.data_ptr() if n else None, n,
                                  ob.data_ptr(), op.data_ptr(), cnt.data_ptr(), ws.data_ptr(), _stream(dev)))
    m = int(cnt.item())
    return ob[:m], op[:m]


def mark_rows(idx: torch.Tensor, nflags: int, flags: torch.Tensor | None = None) -> torch.Tensor:
    """flags[idx[i]] = 1 (uint8 device tensor of nflags; -1 / out-of-range ignored)."""
    L = _lib.load()
    dev = idx.device
    if flags is None:
        flags = torch.zeros(max(nflags, 1), dtype=torch.uint8, device=dev)
    idx = idx.contiguous()
    ib = 8 if idx.dtype == torch.int64 else 4
    if idx.numel():
        check(L.hj_mark_rows(idx.data_ptr(), ib, idx.numel(), flags.data_ptr(), nflags, _stream(dev)))
    return flags


def select_rows(flags: torch.Tensor, want: int, n: int | None = None) -> torch.Tensor:
    """Ascending positions i < n with flags[i] == want (int64 device tensor)."""
    L = _lib.load()
    dev = flags.device
    n = flags.numel() if n is None else n
    out = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_select_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(L.hj_select_rows(flags.data_ptr() if n else None, n, want, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                           _stream(dev)))
    return out[: int(cnt.item())]


def select_bitmap(bitmap: torch.Tensor, n: int, want: int, base: int = 0, bit_offset: int = 0) -> torch.Tensor:
    """Ascending base + i, i < n, whose bit bit_offset + i of the Arrow LSB bitmap (uint8
    device tensor, e.g. HashTable.probe_match's) equals want (0 or 1): hj_select_bitmap,
    an int32 device tensor (the bits of uint32 rows, as the probe's probe_idx)."""
    L = _lib.load()
    dev = bitmap.device
    if bitmap.dtype != torch.uint8 or not bitmap.is_contiguous():
        raise TypeError("bitmap must be a contiguous uint8 tensor")
    if (bit_offset + n + 7) // 8 > bitmap.numel():
        raise ValueError("bitmap is shorter than bit_offset + n bits")
    out = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.hj_select_bitmap_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(L.hj_select_bitmap(bitmap.data_ptr() if n else None, bit_offset, n, want, base, out.data_ptr(),
                             cnt.data_ptr(), ws.data_ptr(), _stream(dev)))
    return out[: int(cnt.item())]


class DeviceRecordBatch:
    """The concatenated build RecordBatch, resident in HBM (row i <-> build index i): what
    the reference hands every partition's consumer with the lookup
    (src/operator/lookup_consumers.rs:4-9). `num_rows`, `schema` and the device columns
    need no host copy; `column(i)` / `to_batch()` bring columns to the host on demand."""

    def __init__(self, schema: pa.Schema, columns: list[DeviceColumn], num_rows: int):
        self.schema = schema
        self.device_columns = columns
        self.num_rows = num_rows
        self._host: pa.RecordBatch | None = None

    @property
    def num_columns(self) -> int:
        return len(self.device_columns)

    def to_batch(self) -> pa.RecordBatch:
        if self._host is None:
            if not self.device_columns:
                self._host = pa.RecordBatch.from_pylist([], schema=self.schema)
            else:
                self._host = pa.RecordBatch.from_arrays([c.to_arrow() for c in self.device_columns],
                                                        schema=self.schema)
        return self._host

    def column(self, i: int | str) -> pa.Array:
        if isinstance(i, str):
            i = self.schema.get_field_index(i)
        return self.device_columns[i].to_arrow()

    @property
    def columns(self) -> list[pa.Array]:
        return self.to_batch().columns
