"""Device key filter (``hj_key_filter`` of the C ABI): a bitmap over the build key range
(exact) or a one-word blocked Bloom filter, filled from the build keys and applied to a
probe batch before it reads the table, so that rows which cannot match are dropped early.

    f = KeyFilter.from_keys(build_keys)                 # hj_key_minmax -> create -> add
    b, p = table.probe(probe_keys, device_output=True, prefilter=f)

The pairs are those of the unfiltered probe, in the same order. The word layouts are
stated in ``include/hj.h``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HJ_FILTER_AUTO, HJ_FILTER_BLOOM, HJ_FILTER_RANGE, HJ_INPUT_DEVICE, check
from .table import KeyInput, as_key_input

try:  # pyarrow is optional for the device path
    import pyarrow as pa
except ImportError:  # pragma: no cover
    pa = None

_KINDS = {"auto": HJ_FILTER_AUTO, "range": HJ_FILTER_RANGE, "bloom": HJ_FILTER_BLOOM}
_KIND_NAMES = {HJ_FILTER_RANGE: "range", HJ_FILTER_BLOOM: "bloom"}
INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)


def _kind(kind) -> int:
    if isinstance(kind, str):
        if kind.lower() not in _KINDS:
            raise ValueError(f"unknown filter kind {kind!r} (auto, range or bloom)")
        return _KINDS[kind.lower()]
    return int(kind)


def plan(kind, key_lo: int, key_hi: int, expected_keys: int) -> tuple[str, int]:
    """hj_key_filter_plan: the (kind, number of uint64 words) a filter of these parameters
    takes ("auto" resolved). Needs no GPU."""
    k, nw = ctypes.c_int(), ctypes.c_uint64()
    check(_lib.load().hj_key_filter_plan(_kind(kind), int(key_lo), int(key_hi), int(expected_keys),
                                         ctypes.byref(k), ctypes.byref(nw)))
    return _KIND_NAMES[k.value], nw.value


def _device_input(keys, valid, valid_offset: int, device: torch.device) -> KeyInput:
    """as_key_input of a key column in device memory; host columns are uploaded first."""
    if pa is not None and isinstance(keys, (pa.Array, pa.ChunkedArray)):
        if valid is not None:
            raise ValueError("pyarrow arrays carry their own validity")
        from .columns import DeviceColumn

        col = DeviceColumn.from_arrow(keys, device)
        keys, valid, valid_offset = col.key_tensor(), col.valid, col.voff
    elif not isinstance(keys, torch.Tensor):
        keys = torch.from_numpy(np.ascontiguousarray(np.asarray(keys)))
    if not keys.is_cuda:
        keys = keys.to(device)
    if valid is not None and not isinstance(valid, torch.Tensor):
        valid = torch.from_numpy(np.ascontiguousarray(np.asarray(valid)))
    ki = as_key_input(keys, valid, valid_offset)
    assert ki.flags & HJ_INPUT_DEVICE
    return ki


def _stream(device) -> int | None:
    return torch.cuda.current_stream(device).cuda_stream or None


class KeyFilter:
    """RAII wrapper of one ``hj_key_filter`` on GPU `device`."""

    def __init__(self, device: int = 0, kind: str | int = "auto", key_lo: int = 0, key_hi: int = -1,
                 expected_keys: int = 0):
        """kind "auto" | "range" | "bloom"; [key_lo, key_hi]: the build key range (a range
        filter's domain; key_lo > key_hi = an empty build); expected_keys sizes a Bloom
        filter (16 bits per key) and decides "auto" (range when the key range spans at most
        64 values per expected key)."""
        self._L = _lib.load()
        self._h = None
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        h = ctypes.c_void_p()
        check(self._L.hj_key_filter_create(self.device, _kind(kind), int(key_lo), int(key_hi), int(expected_keys),
                                           _stream(self._dev) if torch.cuda.is_available() else None,
                                           ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_keys(cls, keys, valid=None, kind: str | int = "auto", valid_offset: int = 0,
                  device: int | None = None) -> "KeyFilter":
        """A filter over the build keys' own range (hj_key_minmax), sized for their number
        and filled with them. `keys`: a device tensor (its device is the filter's), or a
        host column, uploaded to `device`."""
        if device is None:
            device = keys.device.index or 0 if isinstance(keys, torch.Tensor) and keys.is_cuda else 0
        dev = torch.device("cuda", int(device))
        L = _lib.load()
        ki = _device_input(keys, valid, valid_offset, dev)
        lo, hi = INT64_MAX, INT64_MIN  # hj_key_minmax of no rows
        if ki.n:
            mm = torch.empty(2, dtype=torch.int64, device=dev)
            ws = torch.empty(L.hj_key_minmax_workspace_bytes(), dtype=torch.uint8, device=dev)
            check(L.hj_key_minmax(ki.key_type, ki.ptr, ki.valid_ptr, ki.voff, ki.n, mm.data_ptr(), ws.data_ptr(),
                                  _stream(dev)))
            lo, hi = (int(v) for v in mm.tolist())
        f = cls(int(device), kind, lo, hi, ki.n)
        f._add(ki)
        return f

    def _handle(self):
        if not self._h:
            raise ValueError("the filter is closed")
        return self._h

    # -- fill ---------------------------------------------------------------
    def _add(self, ki: KeyInput) -> None:
        check(self._L.hj_key_filter_add(self._handle(), ki.key_type, ki.ptr or None, ki.valid_ptr, ki.voff, ki.n,
                                        _stream(self._dev)))

    def add(self, keys, valid=None, valid_offset: int = 0) -> None:
        """Set the bits of the valid keys of one build batch (any number of batches, in any
        order). valid: bool mask or LSB bitmap from bit valid_offset (as_key_input)."""
        self._add(_device_input(keys, valid, valid_offset, self._dev))

    # -- apply --------------------------------------------------------------
    def test(self, keys, valid=None, valid_offset: int = 0) -> tuple[torch.Tensor, int]:
        """-> (LSB bitmap, uint8 device tensor of ceil(n / 64) * 8 bytes: bit i = row i is
        valid and present; the number of set bits). The bitmap serves any probe as its
        `valid`."""
        ki = _device_input(keys, valid, valid_offset, self._dev)
        bitmap = torch.empty(max((ki.n + 63) // 64, 1), dtype=torch.int64, device=self._dev).view(torch.uint8)
        cnt = torch.zeros(1, dtype=torch.int64, device=self._dev)
        check(self._L.hj_key_filter_test(self._handle(), ki.key_type, ki.ptr or None, ki.valid_ptr, ki.voff, ki.n,
                                         bitmap.data_ptr(), cnt.data_ptr(), _stream(self._dev)))
        return bitmap[: (ki.n + 63) // 64 * 8], int(cnt.item())

    def select(self, keys, valid=None, valid_offset: int = 0, probe_base: int = 0
               ) -> tuple[torch.Tensor, torch.Tensor]:
        """-> (keys, ids) of the valid and present rows in row order: device tensors of the
        keys' dtype and int32 (the u32 ids probe_base + row), the input of
        ``HashTable.probe_async(probe_ids_ptr=...)``. Reads the count (one host sync)."""
        ki = _device_input(keys, valid, valid_offset, self._dev)
        dt = torch.int64 if ki.key_type == _lib.HJ_INT64 else torch.int32
        ok = torch.empty(max(ki.n, 1), dtype=dt, device=self._dev)
        oi = torch.empty(max(ki.n, 1), dtype=torch.int32, device=self._dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=self._dev)
        ws = torch.empty(self._L.hj_key_filter_select_workspace_bytes(ki.n) + 8, dtype=torch.uint8, device=self._dev)
        check(self._L.hj_key_filter_select(self._handle(), ki.key_type, ki.ptr or None, ki.valid_ptr, ki.voff, ki.n,
                                           int(probe_base), ok.data_ptr(), oi.data_ptr(), cnt.data_ptr(),
                                           ws.data_ptr(), _stream(self._dev)))
        m = int(cnt.item())
        return ok[:m], oi[:m]

    # -- inspection -----------------------------------------------------------
    def words(self) -> torch.Tensor:
        """A copy of the filter's uint64 words as an int64 device tensor (same bits)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        check(self._L.hj_key_filter_words(self._handle(), ctypes.byref(p), ctypes.byref(n)))
        out = torch.empty(n.value, dtype=torch.int64, device=self._dev)
        check(self._L.hj_key_filter_export(self._handle(), out.data_ptr(), _stream(self._dev)))
        return out

    def info(self) -> dict:
        """hj_key_filter_info: kind ("range" | "bloom"), exact, nwords, key_lo, key_hi,
        expected_keys, dropped_adds (waits for the last add)."""
        s = _lib.HjKeyFilterInfo()
        check(self._L.hj_key_filter_info_get(self._handle(), ctypes.byref(s)))
        d = {f: getattr(s, f) for f, _ in s._fields_}
        d["kind"] = _KIND_NAMES[d["kind"]]
        d["exact"] = bool(d["exact"])
        return d

    # -- lifetime -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.hj_key_filter_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
