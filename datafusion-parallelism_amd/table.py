"""Thin RAII wrapper of one device hash table (``hj_table``) of the C ABI.

Accepts key columns as pyarrow Int32/Int64 arrays (host, zero-copy pointers incl. the
validity bitmap and offset), numpy int32/int64 arrays (+ optional boolean validity), or
torch int32/int64 tensors (device tensors are passed as device pointers).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import _lib
from ._lib import HJ_BORROW, HJ_BORROW_KEEP, HJ_IDS_U31, HJ_INPUT_DEVICE, HJ_INT32, HJ_INT64, HJ_OUTPUT_HOST, check

try:  # pyarrow is optional for the device path
    import pyarrow as pa
except ImportError:  # pragma: no cover
    pa = None


@dataclass
class KeyInput:
    ptr: int
    valid_ptr: int | None
    voff: int
    n: int
    flags: int
    key_type: int
    keepalive: Any


def _key_type_of_dtype(dt) -> int:
    if dt in (np.int64, torch.int64) or str(dt) in ("int64",):
        return HJ_INT64
    if dt in (np.int32, torch.int32) or str(dt) in ("int32",):
        return HJ_INT32
    raise TypeError(f"join keys must be int32 or int64, got {dt}")


def as_key_input(keys, valid=None, valid_offset: int = 0) -> KeyInput:
    """Normalise a key column into raw pointers for the C ABI. `valid`: a bool mask (one
    per row), or an LSB validity bitmap (uint8 tensor / array) whose bit `valid_offset` is
    row 0 — a device bitmap goes to the ABI as is (no host round trip)."""
    if pa is not None and isinstance(keys, pa.ChunkedArray):
        keys = keys.combine_chunks()
    if pa is not None and isinstance(keys, pa.Array):
        if pa.types.is_int64(keys.type):
            kt, isz = HJ_INT64, 8
        elif pa.types.is_int32(keys.type):
            kt, isz = HJ_INT32, 4
        else:
            raise TypeError(f"join keys must be Int32 or Int64, got {keys.type}")
        if valid is not None:
            raise ValueError("pyarrow arrays carry their own validity")
        bufs = keys.buffers()
        data = bufs[1]
        ptr = (data.address if data is not None else 0) + keys.offset * isz
        vptr = bufs[0].address if (bufs[0] is not None and keys.null_count > 0) else None
        return KeyInput(ptr, vptr, keys.offset if vptr else 0, len(keys), 0, kt, keys)
    if isinstance(keys, torch.Tensor):
        kt = _key_type_of_dtype(keys.dtype)
        t = keys.contiguous()
        flags = HJ_INPUT_DEVICE if t.is_cuda else 0
        vptr, keep_v, voff = None, None, 0
        if valid is not None:
            vb = torch.as_tensor(valid)
            if vb.dtype == torch.bool:  # mask -> LSB bitmap
                if valid_offset:
                    raise ValueError("valid_offset applies to a bitmap, not to a bool mask")
                bits = np.packbits(vb.cpu().numpy(), bitorder="little")
                vb = torch.from_numpy(bits)
            elif vb.dtype == torch.uint8:
                voff = int(valid_offset)
            else:
                raise TypeError("validity must be a bool mask or a uint8 bitmap")
            if t.is_cuda and not vb.is_cuda:
                vb = vb.to(t.device)
            keep_v = vb.contiguous()
            vptr = keep_v.data_ptr()
        return KeyInput(t.data_ptr(), vptr, voff, t.numel(), flags, kt, (t, keep_v))
    a = np.ascontiguousarray(np.asarray(keys))
    kt = _key_type_of_dtype(a.dtype)
    vptr, keep_v, voff = None, None, 0
    if valid is not None:
        va = np.asarray(valid)
        if va.dtype == np.uint8:  # already a bitmap
            bits, voff = np.ascontiguousarray(va), int(valid_offset)
        else:
            bits = np.packbits(va.astype(bool), bitorder="little")
        keep_v = bits
        vptr = bits.ctypes.data
    return KeyInput(a.ctypes.data if a.size else 0, vptr, voff, a.size, 0, kt, (a, keep_v))


def _producer_stream(keys, device: int) -> int | None:
    """torch's current stream for device tensors (the stream that produced them)."""
    if isinstance(keys, torch.Tensor) and keys.is_cuda:
        return torch.cuda.current_stream(keys.device).cuda_stream or None
    return None


def set_device_budget(nbytes: int) -> int:
    """hj_set_device_budget: per-table device byte budget of later builds (0 = none); a
    one-device build above it raises HjError(HJ_ERR_OOM). -> the previous budget."""
    return _lib.load().hj_set_device_budget(int(nbytes))


def is_budget_error(e: Exception) -> bool:
    """The HjError a build raises when it exceeds the device budget."""
    return isinstance(e, _lib.HjError) and e.status == _lib.HJ_ERR_OOM and "device budget" in str(e)


class MatchResult:
    """Result of HashTable.probe_match: `bitmap` (uint8 device tensor, an Arrow LSB bitmap of
    ceil(n/64)*8 bytes, bit i = row i has a partner; usable as a `valid` bitmap), `counts`
    (int32 device tensor of the rows' pair counts, the bits of a uint32; or None) and the
    lazily read statistics `matched`, `pairs` and `candidates` (the only host
    synchronisation). Under a predicate (hj_probe_match_filtered) bitmap, counts, matched and
    pairs speak of the pairs that pass it, candidates of all pairs of the probe; `matched` /
    `pairs` are None where the library computed none (-1: no bitmap or counts / no counts
    were asked for), and `bitmap` is None when none was asked for."""

    def __init__(self, n: int, bitmap: torch.Tensor | None, counts: torch.Tensor | None, d_stats: torch.Tensor):
        self.n, self.bitmap, self.counts, self._d_stats, self._stats = n, bitmap, counts, d_stats, None

    def _read(self) -> tuple:
        if self._stats is None:
            st = [int(v) for v in self._d_stats.cpu().tolist()]
            if len(st) == 2:  # the unfiltered probe: every pair is a candidate
                self._stats = (st[0], st[1], st[1])
            else:
                self._stats = (None if st[0] < 0 else st[0], None if st[1] < 0 else st[1], st[2])
        return self._stats

    @property
    def matched(self) -> int | None:
        """Probe rows with a partner (set bits of the bitmap)."""
        return self._read()[0]

    @property
    def pairs(self) -> int | None:
        """Pairs an inner probe of the same rows would produce (may exceed 2^32); under a
        predicate, those of them that pass it."""
        return self._read()[1]

    @property
    def candidates(self) -> int:
        """Pairs of the probe before any predicate (d_stats[2]; without one: `pairs`)."""
        return self._read()[2]


class PairPlan:
    """Result of HashTable.pair_plan: the pairs of one probe call, to be had in windows of the
    canonical order. `total` (the pair count, may exceed 2^32) is read lazily and is the only
    host synchronisation; the windows are device work on torch's current stream."""

    def __init__(self, table: "HashTable", n: int, plan: torch.Tensor, d_total: torch.Tensor,
                 probe_ids: torch.Tensor | None, probe_base: int):
        self._table, self.n, self._plan, self._d_total = table, n, plan, d_total
        self._ids, self._base, self._total = probe_ids, probe_base, None

    @property
    def total(self) -> int:
        if self._total is None:
            self._total = int(self._d_total.item())
        return self._total

    def window(self, lo: int, cap: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Pairs [lo, lo + cap) of the canonical order as device tensors (build int64, probe
        int32) of exactly w = clamp(total - lo, 0, cap) elements."""
        if lo < 0 or cap < 0:
            raise ValueError("lo and cap must not be negative")
        w = max(min(self.total - lo, cap), 0)
        dev = self._plan.device
        ob = torch.empty(w, dtype=torch.int64, device=dev)
        op = torch.empty(w, dtype=torch.int32, device=dev)
        if w:
            self._table.pair_window_async(self._plan.data_ptr(), self.n, lo, w, ob.data_ptr(), op.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream,
                                          probe_ids_ptr=None if self._ids is None else self._ids.data_ptr(),
                                          probe_base=self._base)
        return ob, op

    def windows(self, max_pairs: int):
        """Consecutive windows of at most max_pairs pairs that cover every pair once."""
        if max_pairs < 1:
            raise ValueError("max_pairs must be at least 1")
        for lo in range(0, self.total, max_pairs):
            yield self.window(lo, max_pairs)


class FilteredPairPlan(PairPlan):
    """Result of HashTable.pair_plan(predicate=...): the pairs of one probe call that pass the
    predicate (F), in windows of the canonical order; no candidate pair is ever written.
    `total` (|F|), `candidates` (|S|, the equi-join's fan-out) and `matched` (probe rows with
    a pair in F) read the statistics once, lazily: the only host synchronisation. `bitmap`:
    the matched-probe bitmap over F (uint8 device tensor, as MatchResult.bitmap) when asked
    for, else None. The plan keeps the predicate, and with it the column buffers, alive."""

    def __init__(self, table: "HashTable", n: int, plan: torch.Tensor, d_stats: torch.Tensor,
                 probe_ids: torch.Tensor | None, probe_base: int, predicate, bitmap: torch.Tensor | None):
        super().__init__(table, n, plan, d_stats, probe_ids, probe_base)
        self._pred, self.bitmap, self._stats = predicate, bitmap, None

    def _read(self) -> tuple:
        if self._stats is None:
            self._stats = tuple(int(v) for v in self._d_total.cpu().tolist())
        return self._stats

    @property
    def matched(self) -> int:
        """Probe rows with a pair in F (set bits of the bitmap)."""
        return self._read()[0]

    @property
    def total(self) -> int:
        """|F|: the pairs that pass the predicate (may exceed 2^32)."""
        return self._read()[1]

    @property
    def candidates(self) -> int:
        """|S|: the pairs of the probe before the predicate."""
        return self._read()[2]

    def window(self, lo: int, cap: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Pairs [lo, lo + cap) of F as device tensors (build int64, probe int32) of exactly
        w = clamp(total - lo, 0, cap) elements."""
        if lo < 0 or cap < 0:
            raise ValueError("lo and cap must not be negative")
        w = max(min(self.total - lo, cap), 0)
        dev = self._plan.device
        ob = torch.empty(w, dtype=torch.int64, device=dev)
        op = torch.empty(w, dtype=torch.int32, device=dev)
        if w:
            self._table.pair_window_filtered_async(self._plan.data_ptr(), self.n, self._pred, lo, w, ob.data_ptr(),
                                                   op.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                                                   probe_ids_ptr=None if self._ids is None else self._ids.data_ptr(),
                                                   probe_base=self._base)
        return ob, op

    def all(self) -> tuple[torch.Tensor, torch.Tensor]:
        """Every pair of F: window(0, total)."""
        return self.window(0, self.total)


class HashTable:
    """One shared build table for `parallelism` partitions (hj_build_begin .. finish)."""

    def __init__(self, parallelism: int = 1, key_type: str | int = "int64", device: int = 0,
                 expected_rows: int = 0, devices: list[int] | None = None, plan: int | str = 0):
        """devices: a multi-GPU table over these GPUs (hj_build_begin_multi; repeats
        allowed), `plan` 0/"auto", 1/"broadcast" or 2/"radix"; else one table on `device`."""
        self._L = _lib.load()
        kt = key_type if isinstance(key_type, int) else (HJ_INT64 if key_type == "int64" else HJ_INT32)
        if key_type not in ("int64", "int32", HJ_INT32, HJ_INT64):
            raise TypeError(f"unsupported key type {key_type}")
        self.key_type = kt
        self.parallelism = parallelism
        self.device = devices[0] if devices else device
        self.devices = list(devices) if devices else None
        h = ctypes.c_void_p()
        if devices is not None:
            plan = {"auto": 0, "broadcast": 1, "radix": 2}.get(plan, plan) if isinstance(plan, str) else plan
            arr = (ctypes.c_int * len(devices))(*devices)
            check(self._L.hj_build_begin_multi(len(devices), arr, parallelism, kt, expected_rows, int(plan),
                                               ctypes.byref(h)))
        else:
            check(self._L.hj_build_begin(device, parallelism, kt, expected_rows, ctypes.byref(h)))
        self._h = h
        self._keep = []  # borrowed device inputs stay alive until the table is freed

    # -- build --------------------------------------------------------------
    def append(self, partition: int, keys, valid=None, ids=None, borrow: bool = True, ids_u31: bool = False,
               valid_offset: int = 0) -> None:
        """ids_u31: the explicit ids are < 2^31 and ascend in canonical row order (the
        table then stores them in place of row numbers, HJ_IDS_U31). valid: bool mask or
        LSB bitmap starting at bit valid_offset (as_key_input)."""
        ki = as_key_input(keys, valid, valid_offset)
        if ki.n and ki.key_type != self.key_type:
            raise TypeError("key type of the batch differs from the table's")
        # borrowed device inputs are kept alive (self._keep) until close(), which frees the
        # table first: the build may run on after finish() (HJ_BORROW_KEEP)
        flags = ki.flags | (HJ_BORROW | HJ_BORROW_KEEP if (borrow and ki.flags & HJ_INPUT_DEVICE) else 0)
        if ids is not None and ids_u31:
            flags |= HJ_IDS_U31
        ids_ptr, keep_ids = None, None
        if ids is not None:
            if isinstance(ids, torch.Tensor):
                keep_ids = ids.to(torch.int64).contiguous()
                ids_ptr = keep_ids.data_ptr()
            else:
                keep_ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
                ids_ptr = keep_ids.ctypes.data
        check(self._L.hj_build_append(self._h, partition, ki.ptr or None, ki.valid_ptr, ki.voff, ids_ptr, ki.n,
                                      flags, _producer_stream(keys, self.device)))
        if flags & HJ_BORROW:
            self._keep.append((ki.keepalive, keep_ids))

    def key_range(self, lo: int, hi: int) -> None:
        """hj_build_key_range: every valid build key lies in [lo, hi] (before the barrier);
        the build skips its key-range reduction."""
        check(self._L.hj_build_key_range(self._h, int(lo), int(hi)))

    def dense(self) -> None:
        """hj_build_dense: direct-addressed over the key_range whatever the density."""
        check(self._L.hj_build_dense(self._h))

    def key_base(self, base: int) -> None:
        """hj_build_key_base: this int32 table's build keys are offsets from `base`; once
        built, the table is keyed by base + offset and takes int64 probe keys (a
        direct-addressed table only; before the barrier)."""
        check(self._L.hj_build_key_base(self._h, int(base)))
        self._rekey = True

    def finish(self, partition: int) -> None:
        check(self._L.hj_build_finish(self._h, partition))
        if getattr(self, "_rekey", False):
            self.key_type = HJ_INT64

    def finish_all(self) -> None:
        """Call the barrier for every partition concurrently (one thread each), as
        DataFusion's executor does for the reference's partitions."""
        import threading

        errs = []

        def run(p):
            try:
                self.finish(p)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=run, args=(p,)) for p in range(self.parallelism)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        if errs:
            raise errs[0]

    def build(self, keys, valid=None, ids=None) -> "HashTable":
        """Single-partition convenience: append + finish."""
        self.append(0, keys, valid, ids)
        self.finish(0)
        return self

    def partition_offset(self, partition: int) -> int:
        v = ctypes.c_int64()
        check(self._L.hj_build_partition_offset(self._h, partition, ctypes.byref(v)))
        return v.value

    def stream_wait(self, stream: int = 0) -> None:
        """Order `stream` (a hipStream_t, 0 = the null stream) after the device build
        (hj_table_stream_wait; probes on any stream already wait by themselves)."""
        check(self._L.hj_table_stream_wait(self._h, stream or None))

    def build_ns(self) -> int:
        """Device time of the build (HIP events), no device work."""
        return self._L.hj_table_build_ns(self._h)

    def device_bytes(self) -> int:
        """Peak device bytes the build held (the device budget's measure; a multi-GPU
        table: its largest shard's)."""
        v = ctypes.c_int64()
        check(self._L.hj_table_device_bytes(self._h, ctypes.byref(v)))
        return v.value

    def stats(self) -> dict:
        s = _lib.HjTableStats()
        check(self._L.hj_table_stats_get(self._h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    # -- lookups ------------------------------------------------------------
    def lookup(self, key: int) -> list[int]:
        """IndexLookup::get_iter: build rows of `key`, newest first (descending)."""
        cnt = ctypes.c_int64()
        check(self._L.hj_table_lookup(self._h, int(key), None, 0, ctypes.byref(cnt)))
        out = np.empty(max(cnt.value, 1), dtype=np.uint64)
        check(self._L.hj_table_lookup(self._h, int(key), out.ctypes.data, cnt.value, ctypes.byref(cnt)))
        return [int(x) for x in out[: cnt.value]]

    def chain_links(self, nrows: int) -> np.ndarray:
        out = np.empty(max(nrows, 1), dtype=np.int64)
        check(self._L.hj_table_chain_links(self._h, out.ctypes.data, nrows))
        return out[:nrows]

    # -- probe --------------------------------------------------------------
    def probe(self, keys, valid=None, device_output: bool = False, valid_offset: int = 0, prefilter=None):
        """Synchronous probe; returns (build_idx uint64, probe_idx uint32) in canonical
        order as numpy arrays, or as torch device tensors (int64, int32) with
        device_output=True (then keys must be a device tensor; a device bitmap `valid`
        with `valid_offset` is read in place). prefilter (device output only): a KeyFilter
        filled from this table's build keys; the rows it rejects are dropped before the
        probe (hj_key_filter_select -> hj_probe_async_ids) and the pairs stay the same, in
        the same order."""
        if device_output:
            return self._probe_device(keys, valid, valid_offset, prefilter)
        if prefilter is not None:
            raise TypeError("prefilter needs device_output=True (the filter runs on device columns)")
        ki = as_key_input(keys, valid, valid_offset)
        if ki.n and ki.key_type != self.key_type:
            raise TypeError("probe key type differs from the build key type")
        pr = _lib.HjPairs()
        flags = ki.flags | HJ_OUTPUT_HOST
        check(self._L.hj_probe(self._h, ki.ptr or None, ki.valid_ptr, ki.voff, ki.n, flags,
                               _producer_stream(keys, self.device), ctypes.byref(pr)))
        try:
            n = pr.count
            b = np.ctypeslib.as_array(pr.build_idx, shape=(n,)).copy() if n else np.empty(0, np.uint64)
            p = np.ctypeslib.as_array(pr.probe_idx, shape=(n,)).copy() if n else np.empty(0, np.uint32)
            return b, p
        finally:
            self._L.hj_pairs_free(ctypes.byref(pr))

    def _probe_device(self, keys: torch.Tensor, valid=None, valid_offset: int = 0, prefilter=None):
        if not (isinstance(keys, torch.Tensor) and keys.is_cuda):
            raise TypeError("device_output=True takes a device tensor of keys")
        ki = as_key_input(keys, valid, valid_offset)
        if ki.n and ki.key_type != self.key_type:
            raise TypeError("probe key type differs from the build key type")
        dev = keys.device
        ids_ptr = None
        if prefilter is not None:
            # the passing rows, compacted in row order with their row numbers as ids: the
            # workspace and the first output capacity follow the passing count
            if prefilter.device != (dev.index or 0):
                raise ValueError("the prefilter lives on another device than the probe keys")
            fkeys, fids = prefilter.select(keys, valid, valid_offset)
            if fkeys.numel() == 0:
                return (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
            ki = KeyInput(fkeys.data_ptr(), None, 0, fkeys.numel(), ki.flags, ki.key_type, (fkeys, fids))
            ids_ptr = fids.data_ptr()
        ws = torch.empty(self.workspace_bytes(ki.n), dtype=torch.uint8, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        cap = max(ki.n, 1)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for _ in range(2):
            ob = torch.empty(cap, dtype=torch.int64, device=dev)
            op = torch.empty(cap, dtype=torch.int32, device=dev)
            self.probe_async(ki.ptr, ki.n, ob.data_ptr(), op.data_ptr(), cap, d_total.data_ptr(), ws.data_ptr(),
                             stream, ki.valid_ptr, ki.voff, probe_ids_ptr=ids_ptr)
            total = int(d_total.item())
            if int(ws[8:16].view(torch.int64).item()) != 0:
                raise _lib.HjError(_lib.HJ_ERR_HIP, "probe look-back timed out")
            if total <= cap:
                return ob[:total], op[:total]
            cap = total
        raise RuntimeError("unreachable")

    def probe_async(self, keys_ptr: int, n: int, out_build_ptr: int, out_probe_ptr: int, capacity: int,
                    d_total_ptr: int, workspace_ptr: int, stream: int = 0, valid_ptr: int | None = None,
                    voff: int = 0, probe_ids_ptr: int | None = None, probe_base: int = 0) -> None:
        """hj_probe_async(_ids, _base) on raw device pointers (no sync, no allocation):
        probe_idx = row, probe_ids[row], or probe_base + row (ids and a base together are
        refused: the ids are the probe indices)."""
        if probe_ids_ptr is not None and probe_base:
            raise ValueError("probe_ids_ptr and probe_base are exclusive: add the base to the ids")
        if probe_ids_ptr is None and probe_base:
            check(self._L.hj_probe_async_base(self._h, keys_ptr, valid_ptr, voff, n, probe_base, out_build_ptr,
                                              out_probe_ptr, capacity, d_total_ptr, workspace_ptr, stream or None))
        elif probe_ids_ptr is None:
            check(self._L.hj_probe_async(self._h, keys_ptr, valid_ptr, voff, n, out_build_ptr, out_probe_ptr,
                                         capacity, d_total_ptr, workspace_ptr, stream or None))
        else:
            check(self._L.hj_probe_async_ids(self._h, keys_ptr, valid_ptr, voff, probe_ids_ptr, n, out_build_ptr,
                                             out_probe_ptr, capacity, d_total_ptr, workspace_ptr, stream or None))

    # -- match probe (hj_probe_match): matches and counts without pairs -------------------
    def match_workspace_bytes(self, n: int) -> int:
        """hj_probe_match_workspace_bytes (depends on the table's layout; no device work)."""
        v = self._L.hj_probe_match_workspace_bytes(self._h, int(n))
        if v < 0:
            check(_lib.HJ_ERR_INVALID, self._L)
        return v

    def probe_match_async(self, keys_ptr: int, n: int, bitmap_ptr: int | None, workspace_ptr: int | None = None,
                          stream: int = 0, valid_ptr: int | None = None, voff: int = 0, counts_ptr: int | None = None,
                          build_flags_ptr: int | None = None, nflags: int = 0, d_stats_ptr: int | None = None,
                          predicate=None) -> None:
        """hj_probe_match on raw device pointers (no sync, no allocation); every output
        pointer is optional. predicate (a columns.PairPredicate): hj_probe_match_filtered
        instead - no workspace (workspace_ptr is ignored), d_stats is an int64[3]."""
        if predicate is not None:
            check(self._L.hj_probe_match_filtered(self._h, keys_ptr or None, valid_ptr, voff, n, predicate.struct,
                                                  bitmap_ptr, counts_ptr, build_flags_ptr, nflags, d_stats_ptr,
                                                  stream or None), self._L)
            return
        check(self._L.hj_probe_match(self._h, keys_ptr or None, valid_ptr, voff, n, bitmap_ptr, counts_ptr,
                                     build_flags_ptr, nflags, d_stats_ptr, workspace_ptr, stream or None), self._L)

    def _probe_match_filtered(self, ki: KeyInput, dev, counts: bool, build_flags: torch.Tensor | None, predicate,
                              bitmap: bool) -> "MatchResult":
        n = ki.n
        bm = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev) if bitmap else None
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
        d_stats = torch.empty(3, dtype=torch.int64, device=dev)
        self.probe_match_async(ki.ptr, n, None if bm is None else bm.data_ptr(), None,
                               torch.cuda.current_stream(dev).cuda_stream, ki.valid_ptr, ki.voff,
                               None if cnt is None else cnt.data_ptr(),
                               None if build_flags is None else build_flags.data_ptr(),
                               0 if build_flags is None else build_flags.numel(), d_stats.data_ptr(), predicate)
        # the key tensors and the predicate's columns are released in stream order by torch's allocator
        return MatchResult(n, bm, cnt, d_stats)

    def probe_match(self, keys: torch.Tensor, valid=None, valid_offset: int = 0, counts: bool = False,
                    build_flags: torch.Tensor | None = None, predicate=None, bitmap: bool = True) -> "MatchResult":
        """Per probe row whether (and, with counts=True, how often) its key occurs in the
        table, without materialising pairs: what a semi or anti join needs. keys: a device
        tensor; valid: bool mask or LSB bitmap from bit valid_offset (as_key_input);
        build_flags: a uint8 device tensor, one byte per build row (or id), updated in place:
        the rows the probe's pairs would name are set to 1, nothing is cleared, so one
        tensor accumulates over batches. Not for a multi-GPU table (HJ_ERR_INVALID). No
        host synchronisation: MatchResult.matched / .pairs read the statistics lazily.
        predicate: a columns.PairPredicate over the build side's columns and this batch's
        (row i of a probe column belongs to keys[i]): only the pairs that pass it count
        (hj_probe_match_filtered: a semi / anti join under a join filter; the walk over a
        key's build rows stops at the first passing pair unless counts or flags are asked
        for). bitmap=False (with a predicate only) asks for no bitmap: with build_flags as the
        only output, candidates whose flag is already set are skipped."""
        if not (isinstance(keys, torch.Tensor) and keys.is_cuda):
            raise TypeError("probe_match takes a device tensor of keys")
        ki = as_key_input(keys, valid, valid_offset)
        if ki.n and ki.key_type != self.key_type:
            raise TypeError("probe key type differs from the build key type")
        if build_flags is not None and not (build_flags.is_cuda and build_flags.dtype == torch.uint8 and
                                            build_flags.is_contiguous()):
            raise TypeError("build_flags must be a contiguous uint8 device tensor")
        dev = keys.device
        if predicate is not None:
            return self._probe_match_filtered(ki, dev, counts, build_flags, predicate, bitmap)
        n = ki.n
        bitmap = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
        d_stats = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(self.match_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.probe_match_async(ki.ptr, n, bitmap.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                               ki.valid_ptr, ki.voff, None if cnt is None else cnt.data_ptr(),
                               None if build_flags is None else build_flags.data_ptr(),
                               0 if build_flags is None else build_flags.numel(), d_stats.data_ptr())
        # ws and the key tensors are released in stream order by torch's allocator
        return MatchResult(n, bitmap, cnt, d_stats)

    # -- pair plan / pair window (hj_pair_plan, hj_pair_window): pairs in bounded slices ---
    def pair_plan_bytes(self, n: int) -> int:
        """hj_pair_plan_bytes (no device work)."""
        v = self._L.hj_pair_plan_bytes(self._h, int(n))
        if v < 0:
            check(_lib.HJ_ERR_INVALID, self._L)
        return v

    def pair_plan_async(self, keys_ptr: int, n: int, plan_ptr: int, d_total_ptr: int | None = None, stream: int = 0,
                        valid_ptr: int | None = None, voff: int = 0) -> None:
        """hj_pair_plan on raw device pointers (no sync, no allocation)."""
        check(self._L.hj_pair_plan(self._h, keys_ptr or None, valid_ptr, voff, n, plan_ptr, d_total_ptr,
                                   stream or None), self._L)

    def pair_window_async(self, plan_ptr: int, n: int, pair_lo: int, capacity: int, out_build_ptr: int | None,
                          out_probe_ptr: int | None, stream: int = 0, d_written_ptr: int | None = None,
                          probe_ids_ptr: int | None = None, probe_base: int = 0) -> None:
        """hj_pair_window on raw device pointers (no sync, no allocation): pairs
        [pair_lo, pair_lo + capacity) of the plan of n rows; probe_idx = row, probe_ids[row]
        or probe_base + row (ids and a base together are refused, as in probe_async)."""
        if probe_ids_ptr is not None and probe_base:
            raise ValueError("probe_ids_ptr and probe_base are exclusive: add the base to the ids")
        check(self._L.hj_pair_window(self._h, plan_ptr, n, probe_ids_ptr, probe_base, pair_lo, capacity,
                                     out_build_ptr, out_probe_ptr, d_written_ptr, stream or None), self._L)

    # -- filtered pair plan (hj_pair_plan_filtered, hj_pair_window_filtered) ----------------
    def pair_plan_filtered_bytes(self, n: int) -> int:
        """hj_pair_plan_filtered_bytes (no device work)."""
        v = self._L.hj_pair_plan_filtered_bytes(self._h, int(n))
        if v < 0:
            check(_lib.HJ_ERR_INVALID, self._L)
        return v

    def pair_plan_filtered_async(self, keys_ptr: int, n: int, predicate, plan_ptr: int, stream: int = 0,
                                 valid_ptr: int | None = None, voff: int = 0, bitmap_ptr: int | None = None,
                                 build_flags_ptr: int | None = None, nflags: int = 0,
                                 d_stats_ptr: int | None = None) -> None:
        """hj_pair_plan_filtered on raw device pointers (no sync, no allocation); predicate: a
        columns.PairPredicate; d_stats: an int64[3]."""
        check(self._L.hj_pair_plan_filtered(self._h, keys_ptr or None, valid_ptr, voff, n, predicate.struct, plan_ptr,
                                            bitmap_ptr, build_flags_ptr, nflags, d_stats_ptr, stream or None), self._L)

    def pair_window_filtered_async(self, plan_ptr: int, n: int, predicate, pair_lo: int, capacity: int,
                                   out_build_ptr: int | None, out_probe_ptr: int | None, stream: int = 0,
                                   d_written_ptr: int | None = None, probe_ids_ptr: int | None = None,
                                   probe_base: int = 0) -> None:
        """hj_pair_window_filtered on raw device pointers (no sync, no allocation): passing
        pairs [pair_lo, pair_lo + capacity) of the filtered plan of n rows, under the predicate
        the plan was made with; probe_idx = row, probe_ids[row] or probe_base + row."""
        if probe_ids_ptr is not None and probe_base:
            raise ValueError("probe_ids_ptr and probe_base are exclusive: add the base to the ids")
        check(self._L.hj_pair_window_filtered(self._h, plan_ptr, n, predicate.struct, probe_ids_ptr, probe_base,
                                              pair_lo, capacity, out_build_ptr, out_probe_ptr, d_written_ptr,
                                              stream or None), self._L)

    def _pair_plan_filtered(self, ki: KeyInput, dev, probe_ids, probe_base: int, predicate,
                            build_flags: torch.Tensor | None, bitmap: bool) -> "FilteredPairPlan":
        n = ki.n
        plan = torch.empty(self.pair_plan_filtered_bytes(n), dtype=torch.uint8, device=dev)
        bm = torch.empty(((n + 63) // 64) * 8, dtype=torch.uint8, device=dev) if bitmap else None
        d_stats = torch.empty(3, dtype=torch.int64, device=dev)
        self.pair_plan_filtered_async(ki.ptr, n, predicate, plan.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream, ki.valid_ptr, ki.voff,
                                      None if bm is None else bm.data_ptr(),
                                      None if build_flags is None else build_flags.data_ptr(),
                                      0 if build_flags is None else build_flags.numel(), d_stats.data_ptr())
        # the key tensors are released in stream order by torch's allocator; the plan keeps the predicate
        return FilteredPairPlan(self, n, plan, d_stats, probe_ids, probe_base, predicate, bm)

    def pair_plan(self, keys: torch.Tensor, valid=None, valid_offset: int = 0, probe_ids: torch.Tensor | None = None,
                  probe_base: int = 0, prefilter=None, predicate=None, build_flags: torch.Tensor | None = None,
                  bitmap: bool = False) -> "PairPlan":
        """Look every probe row up once and return a PairPlan, whose windows give the pairs
        probe(keys, valid, device_output=True) would return, in the same order, in slices of
        a size the caller chooses: peak memory is the window's, not the join's fan-out. keys:
        a device tensor; valid: bool mask or LSB bitmap from bit valid_offset (as_key_input);
        probe_ids: an int32 device tensor (the bits of a uint32) of the rows' probe indices,
        or probe_base + row, not both. prefilter: a KeyFilter filled from this table's build
        keys; the rows it rejects are dropped before the plan (they have no pairs), the
        windows name the surviving rows by their ids. Not for a multi-GPU table
        (HJ_ERR_INVALID). No host synchronisation here: PairPlan.total reads the pair count
        lazily. Plan and windows run on torch's current stream.
        predicate: a columns.PairPredicate over the build side's columns and this batch's (row
        i of a probe column belongs to keys[i], whatever probe_ids says): the result is a
        FilteredPairPlan, whose windows hold only the pairs that pass it, in the same order
        (hj_pair_plan_filtered: the candidates are evaluated in registers, none is written).
        With it, build_flags (a uint8 device tensor, one byte per build row or id, OR'ed in
        place) marks the build rows of the passing pairs and bitmap=True asks for the
        matched-probe bitmap over them - an outer join's bookkeeping from the same walk. The
        key filter is not used under a predicate (prefilter must be None)."""
        if not (isinstance(keys, torch.Tensor) and keys.is_cuda):
            raise TypeError("pair_plan takes a device tensor of keys")
        if predicate is None and (build_flags is not None or bitmap):
            raise ValueError("build_flags and bitmap belong to a filtered plan: give a predicate")
        if predicate is not None and prefilter is not None:
            raise ValueError("the filtered pair plan does not use a key filter")
        if build_flags is not None and not (build_flags.is_cuda and build_flags.dtype == torch.uint8 and
                                            build_flags.is_contiguous()):
            raise TypeError("build_flags must be a contiguous uint8 device tensor")
        if probe_ids is not None and probe_base:
            raise ValueError("probe_ids and probe_base are exclusive: add the base to the ids")
        if probe_ids is not None and not (probe_ids.is_cuda and probe_ids.dtype == torch.int32 and
                                          probe_ids.is_contiguous() and probe_ids.numel() == keys.numel()):
            raise TypeError("probe_ids must be a contiguous int32 device tensor, one per key")
        ki = as_key_input(keys, valid, valid_offset)
        if ki.n and ki.key_type != self.key_type:
            raise TypeError("probe key type differs from the build key type")
        dev = keys.device
        if predicate is not None:
            return self._pair_plan_filtered(ki, dev, probe_ids, probe_base, predicate, build_flags, bitmap)
        if prefilter is not None:
            if prefilter.device != (dev.index or 0):
                raise ValueError("the prefilter lives on another device than the probe keys")
            fkeys, fids = prefilter.select(keys, valid, valid_offset, probe_base=probe_base)
            if probe_ids is not None:
                fids = probe_ids[fids.to(torch.int64)]
            ki = KeyInput(fkeys.data_ptr(), None, 0, fkeys.numel(), ki.flags, ki.key_type, (fkeys, fids))
            probe_ids, probe_base = fids, 0
        plan = torch.empty(self.pair_plan_bytes(ki.n), dtype=torch.uint8, device=dev)
        d_total = torch.empty(1, dtype=torch.int64, device=dev)
        self.pair_plan_async(ki.ptr, ki.n, plan.data_ptr(), d_total.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream, ki.valid_ptr, ki.voff)
        # the key tensors are released in stream order by torch's allocator
        return PairPlan(self, ki.n, plan, d_total, probe_ids, probe_base)

    # -- sharded-build broadcast plan (hj_table_dense_piece / hj_table_wrap_dense) -------
    def dense_piece(self) -> dict:
        """A built direct-addressed table's arrays (device pointers): refs, nvalues,
        key_min, dup_rows, dup_used (device pointer to a u64), packed."""
        refs, dup, used = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nv, kmin, packed = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_int()
        check(self._L.hj_table_dense_piece(self._h, ctypes.byref(refs), ctypes.byref(nv), ctypes.byref(kmin),
                                           ctypes.byref(dup), ctypes.byref(used), ctypes.byref(packed)))
        return {"refs": refs.value or 0, "nvalues": nv.value, "key_min": kmin.value, "dup_rows": dup.value or 0,
                "dup_used": used.value or 0, "packed": bool(packed.value)}

    def dense_export(self, refs: torch.Tensor | None = None, v0: int = 0, dup: torch.Tensor | None = None,
                     dup_used: torch.Tensor | None = None, stream: int = 0) -> None:
        """Device copies of the refs [v0, v0 + refs.numel()), the first dup.numel() segment
        words and the segment words in use (one int64) into the given tensors, on `stream`."""
        check(self._L.hj_table_dense_export(self._h, None if refs is None else refs.data_ptr(), v0,
                                            0 if refs is None else refs.numel(),
                                            None if dup is None else dup.data_ptr(), 0 if dup is None else dup.numel(),
                                            None if dup_used is None else dup_used.data_ptr(), stream or None))

    @classmethod
    def wrap_dense(cls, device: int, key_type: str | int, key_min: int, refs: torch.Tensor,
                   dup_rows: torch.Tensor, packed: bool, stream: int = 0) -> "HashTable":
        """A probe-only table over device tensors (int32/uint32 views of the u32 refs and
        segments), kept alive by the table: refs[v] for key key_min + v."""
        self = cls.__new__(cls)
        self._L = _lib.load()
        kt = key_type if isinstance(key_type, int) else (HJ_INT64 if key_type == "int64" else HJ_INT32)
        self.key_type, self.parallelism, self.device, self.devices = kt, 1, device, None
        h = ctypes.c_void_p()
        check(self._L.hj_table_wrap_dense(device, kt, int(key_min), refs.numel(), refs.data_ptr(),
                                          dup_rows.data_ptr(), int(bool(packed)), stream or None, ctypes.byref(h)))
        self._h = h
        self._keep = [refs, dup_rows]
        return self

    @classmethod
    def from_handle(cls, handle: ctypes.c_void_p, device: int, key_type: str | int, keep=(), lib=None) -> "HashTable":
        """Adopt a built table handle another entry point returned (hj_dist_build_sharded);
        `keep`: tensors its build still reads, kept alive until close(); `lib`: the library
        that made it (tests: the thread-transport build), default the product library."""
        self = cls.__new__(cls)
        self._L = lib or _lib.load()
        kt = key_type if isinstance(key_type, int) else (HJ_INT64 if key_type == "int64" else HJ_INT32)
        self.key_type, self.parallelism, self.device, self.devices = kt, 1, device, None
        self._h = handle
        self._keep = list(keep)
        return self

    @staticmethod
    def rebase_dups(refs: torch.Tensor, base: int, packed: bool, stream: int = 0) -> None:
        """hj_dense_rebase_dups on a (view of a) u32 refs tensor."""
        check(_lib.load().hj_dense_rebase_dups(refs.data_ptr(), refs.numel(), int(base), int(bool(packed)),
                                               stream or None))

    @staticmethod
    def workspace_bytes(n: int) -> int:
        return _lib.load().hj_probe_workspace_bytes(n)

    # -- lifetime -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.hj_table_free(self._h)
            self._h = None
            self._keep.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
