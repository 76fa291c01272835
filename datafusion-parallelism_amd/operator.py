"""Host-side mirror of the reference's operator/plugin interface for the hot path.

The reference (Rust, DataFusion 40) plugs build strategies in behind
``BuildImplementation`` and hands the built table to the probe side through the
``IndexLookup`` / ``IndexLookupConsumer`` seam. This module restates that surface in
Python over pyarrow RecordBatches, with a single new strategy, ``JoinReplacement.Gpu``,
whose build and probe run on the gfx950 kernels through the C ABI (``include/hj.h``):

  reference                                                   here
  ---------------------------------------------------------   ---------------------------------
  JoinReplacement (src/parse_sql.rs:12-24)                    JoinReplacement (+ Gpu)
  BuildImplementation::new (src/operator/build_implementation.rs:34-48)
                                                              BuildImplementation(...)
  BuildImplementation::build_side (…:50-112)                  BuildImplementation.build_side
  IndexLookup::get_iter (src/utils/index_lookup.rs:1-6)       GpuIndexLookup.get_iter
  IndexLookupConsumer::call (src/operator/lookup_consumers.rs:4-9)
                                                              consumer.call(lookup, record_batch)
  get_matching_indices + equal_rows_arr (src/shared/shared.rs:29-47,
    src/shared/datafusion_private.rs:40-80)                   GpuIndexLookup.matching_indices
  lookup_inner_join_probe_batch (src/operator/probe_lookup_implementation/inner.rs:79-129)
                                                              lookup_inner_join_probe_batch
  ParallelHashJoin::execute (src/operator/parallel_hash_join.rs:140-167)
                                                              ParallelHashJoin.execute / collect

  ProbeLookupStreamImplementation (src/operator/probe_lookup_implementation/
    probe_lookup_implementation.rs:19-80): Inner, Left, Right, Full, LeftSemi, LeftAnti,
    RightSemi, RightAnti                                      JoinType + _probe_batch /
                                                              _finalize_build_side
  apply_join_filter_to_indices (src/shared/datafusion_private.rs:295-328)
                                                              JoinFilter (host callable),
                                                              CompareFilter (device, hj_pair_filter_select;
                                                              semi / anti joins under match_probe:
                                                              hj_probe_match_filtered, no pairs)

Join keys: one Int32/Int64 column goes to the table as is (exact keys); several key
columns, or a key of any other fixed-width or Utf8/Binary type, go through
hj_composite_keys (one 64-bit key per row from all key columns, the reference's
calculate_hash) and the candidate pairs through hj_filter_equal_pairs (equal_rows_arr).
Output columns are materialised on the GPU
(columns.DeviceColumn.take: the build side is uploaded once after the barrier, each probe
batch once). The reference's CPU strategies (Original, New..New10) are not part of this
package.
"""
from __future__ import annotations

import enum
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterable, Sequence

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

from ._lib import HjError, HJ_ERR_INVALID
from .columns import (DeviceColumn, DeviceRecordBatch, PairPredicate, composite_keys, filter_equal_pairs, mark_rows,
                      pair_filter_select, select_bitmap, select_rows)
from .key_filter import KeyFilter
from .table import HashTable


class JoinReplacement(enum.Enum):
    """src/parse_sql.rs:12-24, plus the MI355X strategy."""
    Original = "Original"
    New = "New"
    New3 = "New3"
    New4 = "New4"
    New5 = "New5"
    New6 = "New6"
    New7 = "New7"
    New8 = "New8"
    New9 = "New9"
    New10 = "New10"
    Gpu = "Gpu"


def evaluate_expressions(expressions: Sequence[str | int], batch: pa.RecordBatch) -> list[pa.Array]:
    """src/shared/shared.rs:18-22 for plain column expressions (name or index)."""
    out = []
    for e in expressions:
        out.append(batch.column(e) if isinstance(e, int) else batch.column(batch.schema.get_field_index(e)))
    return out


def _key_type(arr: pa.Array) -> str:
    if pa.types.is_int64(arr.type):
        return "int64"
    if pa.types.is_int32(arr.type):
        return "int32"
    raise HjError(HJ_ERR_INVALID, f"join key type {arr.type} is not an Int32/Int64 key")


def _is_simple_key(arrays: Sequence[pa.Array]) -> bool:
    """One Int32/Int64 key column: the table takes it as is; anything else is composite."""
    return len(arrays) == 1 and (pa.types.is_int64(arrays[0].type) or pa.types.is_int32(arrays[0].type))


class JoinType(enum.Enum):
    """datafusion_common::JoinType as supported by the reference's probe side
    (probe_lookup_implementation.rs:32-43). Left = build side, right = probe side."""
    Inner = "inner"
    Left = "left"
    Right = "right"
    Full = "full"
    LeftSemi = "leftsemi"
    LeftAnti = "leftanti"
    RightSemi = "rightsemi"
    RightAnti = "rightanti"

    @classmethod
    def parse(cls, v: "JoinType | str") -> "JoinType":
        if isinstance(v, JoinType):
            return v
        key = str(v).lower().replace("_", "").replace(" ", "").replace("outer", "")
        for jt in cls:
            if jt.value == key:
                return jt
        raise HjError(HJ_ERR_INVALID, f"unknown join type {v!r}")

    @property
    def marks_build(self) -> bool:  # build-side visited bitset (ConcurrentBitSet)
        return self in (JoinType.Left, JoinType.Full, JoinType.LeftSemi, JoinType.LeftAnti)


class JoinFilter:
    """A non-equi join condition applied to the equal-key candidate pairs
    (apply_join_filter_to_indices, src/shared/datafusion_private.rs:295-328):
    `expression(left_rows, right_rows)` gets the candidate rows of the `left_columns` /
    `right_columns` it reads (pyarrow RecordBatches, one row per pair) and returns a
    BooleanArray; null counts as false."""

    def __init__(self, expression: Callable[[pa.RecordBatch, pa.RecordBatch], pa.Array],
                 left_columns: Sequence[str] | None = None, right_columns: Sequence[str] | None = None):
        self.expression = expression
        self.left_columns = left_columns
        self.right_columns = right_columns


class L:
    """A build (left) column of a CompareFilter term, by name."""

    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"L({self.name!r})"


class R:
    """A probe (right) column of a CompareFilter term, by name."""

    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"R({self.name!r})"


_FLIP = {"==": "==", "=": "==", "!=": "!=", "<>": "!=", "<": ">", "<=": ">=", ">": "<", ">=": "<="}
_PC_OPS = {"==": pc.equal, "=": pc.equal, "!=": pc.not_equal, "<>": pc.not_equal, "<": pc.less,
           "<=": pc.less_equal, ">": pc.greater, ">=": pc.greater_equal}


class CompareFilter:
    """A declarative non-equi join condition that runs on the device: a conjunction of
    comparisons between build columns (`L(name)`), probe columns (`R(name)`) and constants
    (bare Python scalars), e.g.

        CompareFilter([(L("value"), "!=", R("value")), (R("ts"), ">=", L("lo")), (L("qty"), "<", 10)])

    The candidate pairs are filtered by hj_pair_filter_select over the resident build and
    probe columns (apply_join_filter_to_indices, src/shared/datafusion_private.rs:295-328):
    no column is gathered and only the count of survivors comes to the host. Operators:
    == != < <= > >= (also = and <>). A null operand fails the pair. Floats compare in IEEE
    totalOrder (include/hj.h): unlike pyarrow, NaN equals the NaN of the same bits and
    -0.0 < +0.0. Types the device does not compare (columns.PairPredicate) raise TypeError at
    the first probe batch; there is no host fallback. `as_callable()` gives the equivalent
    JoinFilter for the host path."""

    def __init__(self, terms):
        self.terms = []
        for lhs, op, rhs in terms:
            if op not in _FLIP:
                raise ValueError(f"unknown comparison {op!r}")
            if not isinstance(lhs, (L, R)):
                if not isinstance(rhs, (L, R)):
                    raise ValueError("a term compares at least one column")
                lhs, op, rhs = rhs, _FLIP[op], lhs  # constant on the left: c < x is x > c
            self.terms.append((lhs, op, rhs))
        if not 1 <= len(self.terms) <= 16:
            raise ValueError("a CompareFilter has 1..16 terms")

    def _names(self, kind) -> list[str]:
        out = []
        for lhs, _, rhs in self.terms:
            for x in (lhs, rhs):
                if isinstance(x, kind) and x.name not in out:
                    out.append(x.name)
        return out

    def predicate(self, build_cols: Sequence[DeviceColumn], build_names: Sequence[str],
                  probe_cols: Sequence[DeviceColumn], probe_names: Sequence[str], build_rows: int,
                  probe_rows: int, eq_keys: Sequence[tuple[DeviceColumn, DeviceColumn]] = ()) -> PairPredicate:
        """The PairPredicate over the columns the terms name (each column listed once).
        eq_keys: (build column, probe column) pairs, one `==` term each after the filter's
        own (the exact key equality of a composite-key match probe)."""
        lnames, rnames = self._names(L), self._names(R)
        bnames, pnames = list(build_names), list(probe_names)

        def ref(x):
            if isinstance(x, L):
                return ("build", lnames.index(x.name))
            if isinstance(x, R):
                return ("probe", rnames.index(x.name))
            return x

        for n, names, side in [(n, bnames, "build") for n in lnames] + [(n, pnames, "probe") for n in rnames]:
            if n not in names:
                raise HjError(HJ_ERR_INVALID, f"CompareFilter: the {side} side has no column {n!r}")
        return PairPredicate([build_cols[bnames.index(n)] for n in lnames] + [b for b, _ in eq_keys],
                             [probe_cols[pnames.index(n)] for n in rnames] + [p for _, p in eq_keys],
                             [(ref(a), op, ref(b)) for a, op, b in self.terms] +
                             [(("build", len(lnames) + i), "==", ("probe", len(rnames) + i))
                              for i in range(len(eq_keys))], build_rows, probe_rows)

    def as_callable(self) -> "JoinFilter":
        """The same condition as a host JoinFilter over pyarrow compute calls (IEEE float
        comparison there: it differs from the device path on NaN and signed zeros only)."""
        terms = list(self.terms)

        def expression(left: pa.RecordBatch, right: pa.RecordBatch) -> pa.Array:
            def operand(x, other):
                if isinstance(x, L):
                    return left.column(x.name)
                if isinstance(x, R):
                    return right.column(x.name)
                t = other.type
                return pa.scalar(x) if pa.types.is_floating(t) else pa.scalar(x, type=t)

            mask = None
            for lhs, op, rhs in terms:
                a = operand(lhs, None)
                m = _PC_OPS[op](a, operand(rhs, a))
                mask = m if mask is None else pc.and_kleene(mask, m)
            return mask

        return JoinFilter(expression, self._names(L), self._names(R))


def _batch(cols: Sequence[DeviceColumn], names: Sequence[str]) -> pa.RecordBatch:
    return pa.RecordBatch.from_arrays([c.to_arrow() for c in cols], names=list(names))


class GpuIndexLookup:
    """The read-only shared table handed to every partition (IndexLookup<u64>), with the
    build RecordBatch's columns resident in HBM for output materialisation."""

    def __init__(self, table: HashTable, shared: "_SharedBuild | None" = None):
        self.table = table
        self._shared = shared

    @property
    def device(self) -> torch.device:
        return torch.device("cuda", self.table.device)

    def get_iter(self, key: int):
        """Build rows of `key` in chain order (newest first)
        (src/operator/version10/lookup_implementation_3.rs:22-59). The reference keys
        the lookup by hash; the GPU table is keyed by the exact key (its hash is
        internal), which the equality re-check makes equivalent."""
        return iter(self.table.lookup(key))

    def matching_indices_device(self, probe_keys: pa.Array | Sequence[pa.Array],
                                build_side_records: pa.RecordBatch | None = None
                                ) -> tuple[torch.Tensor, torch.Tensor]:
        """get_matching_indices + equal_rows_arr on the GPU: ProbeBuildIndices after the
        equality filter as device tensors (build int64, probe int32). One Int32/Int64
        key: the table compares exact keys (fused). Composite keys: candidates of equal
        composite key, then hj_filter_equal_pairs on the key columns."""
        arrays = ([probe_keys] if isinstance(probe_keys, (pa.Array, pa.ChunkedArray, DeviceColumn))
                  else list(probe_keys))
        if self.build_is_empty:
            return (torch.empty(0, dtype=torch.int64, device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device))
        if self._shared is not None and (self._shared.composite or not _is_simple_key(arrays)):
            return self._composite_matches(arrays, build_side_records)
        if not _is_simple_key(arrays):
            raise HjError(HJ_ERR_INVALID, "probe keys do not match the build keys (one Int32/Int64 column)")
        probe_keys = arrays[0]
        n = probe_keys.length if isinstance(probe_keys, DeviceColumn) else len(probe_keys)
        if n == 0:
            return (torch.empty(0, dtype=torch.int64, device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device))
        keys = probe_keys if isinstance(probe_keys, DeviceColumn) else DeviceColumn.from_arrow(probe_keys, self.device)
        # the device validity bitmap goes to the probe as is, from bit voff (no host read)
        return self.table.probe(keys.key_tensor(), keys.valid, device_output=True, valid_offset=keys.voff,
                                prefilter=self._prefilter())

    @property
    def build_is_empty(self) -> bool:
        """No build row in any partition. The table's key type comes with the first non-empty
        build batch; without one the table is an empty Int64 table whatever the join's key
        is, so a probe does not ask it: there are no pairs."""
        return self._shared is not None and self._shared.build_rows() == 0

    def _prefilter(self) -> "KeyFilter | None":
        return self._shared.key_filter() if self._shared is not None else None

    def _composite_matches(self, arrays: list[pa.Array], build_side_records: pa.RecordBatch | None):
        sh = self._shared
        if len(arrays) != len(sh.key_exprs):
            raise HjError(HJ_ERR_INVALID, f"{len(arrays)} probe key columns for {len(sh.key_exprs)} build key columns")
        pcols = [a if isinstance(a, DeviceColumn) else DeviceColumn.from_arrow(a, self.device) for a in arrays]
        n = pcols[0].length
        if n == 0:
            return (torch.empty(0, dtype=torch.int64, device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device))
        keys, valid = composite_keys(pcols)
        b, p = self.table.probe(keys, valid, device_output=True, prefilter=self._prefilter())
        rb = build_side_records if build_side_records is not None else sh.concatenated()
        bcols = self.build_columns(rb)
        kidx = [e if isinstance(e, int) else rb.schema.get_field_index(e) for e in sh.key_exprs]
        return filter_equal_pairs([bcols[i] for i in kidx], pcols, b, p)

    def matching_windows(self, probe_keys: Sequence[DeviceColumn], max_pairs: int,
                         build_side_records: pa.RecordBatch | None = None):
        """matching_indices_device in slices: an iterator over the same pairs, in the same
        order, as consecutive windows of at most max_pairs candidate pairs (HashTable.pair_plan:
        one lookup, then one window at a time), each after the equality re-check of a
        composite key. No pair buffer exceeds max_pairs elements."""
        pcols = list(probe_keys)
        sh = self._shared
        composite = sh is not None and (sh.composite or not _is_simple_key(pcols))
        if not composite and not _is_simple_key(pcols):
            raise HjError(HJ_ERR_INVALID, "probe keys do not match the build keys (one Int32/Int64 column)")
        if composite and len(pcols) != len(sh.key_exprs):
            raise HjError(HJ_ERR_INVALID, f"{len(pcols)} probe key columns for {len(sh.key_exprs)} build key columns")
        if pcols[0].length == 0 or self.build_is_empty:
            return
        if composite:
            keys, valid = composite_keys(pcols)
            plan = self.table.pair_plan(keys, valid, prefilter=self._prefilter())
            rb = build_side_records if build_side_records is not None else sh.concatenated()
            bcols = self.build_columns(rb)
            kcols = [bcols[e if isinstance(e, int) else rb.schema.get_field_index(e)] for e in sh.key_exprs]
            for b, p in plan.windows(max_pairs):
                yield filter_equal_pairs(kcols, pcols, b, p)
        else:
            k = pcols[0]
            plan = self.table.pair_plan(k.key_tensor(), k.valid, valid_offset=k.voff, prefilter=self._prefilter())
            yield from plan.windows(max_pairs)

    def matching_indices(self, probe_keys: pa.Array) -> tuple[pa.UInt64Array, pa.UInt32Array]:
        """Host form of matching_indices_device (UInt64 build, UInt32 probe)."""
        b, p = self.table.probe(probe_keys)
        return pa.array(b, type=pa.uint64()), pa.array(p, type=pa.uint32())

    def build_columns(self, build_side_records) -> list[DeviceColumn]:
        if isinstance(build_side_records, DeviceRecordBatch):  # resident since the build
            return build_side_records.device_columns
        if self._shared is not None:
            return self._shared.device_columns(build_side_records, self.device)
        return [DeviceColumn.from_arrow(c, self.device) for c in build_side_records.columns]


class _SharedBuild:
    """State shared by all partitions of one build (JoinStateInstances)."""

    def __init__(self, parallelism: int, device: int, devices: Sequence[int] | None = None, plan: str = "auto",
                 prefilter: bool = False, match_probe: bool = False, max_output_rows: int | None = None,
                 filtered_probe: bool = False):
        self.parallelism = parallelism
        self.filtered_probe = filtered_probe  # pair joins under a device predicate emit only passing pairs
        self.max_output_rows = max_output_rows  # probe batches emit in windows of at most this many rows
        self.prefilter = prefilter      # probes go through a key filter over the build keys
        self.match_probe = match_probe  # semi / anti joins probe for matches, not pairs (probe_batch)
        self._filter: KeyFilter | None = None
        self.device = devices[0] if devices else device
        self.devices = list(devices) if devices else None
        self.plan = plan
        self.lock = threading.Lock()
        self.table: HashTable | None = None
        self.key_type: str | None = None
        # per partition, its batches' columns uploaded once on arrival (DeviceColumn) and
        # their row counts
        self.batches: list[list[tuple[list[DeviceColumn], int]]] = [[] for _ in range(parallelism)]
        self.taken = [False] * parallelism
        self.ready = threading.Barrier(parallelism)
        self.record_batch: DeviceRecordBatch | None = None
        self.schema: pa.Schema | None = None
        self._dev_cols: list[DeviceColumn] | None = None
        self.composite = False          # keys through hj_composite_keys (several / non-integer columns)
        self.key_exprs: list = []       # the build key expressions (the equality filter's columns)

    def table_for(self, key_type: str) -> HashTable:
        with self.lock:
            if self.table is None:
                self.key_type = key_type
                # one table on one GPU, or one table over a node's GPUs (hj_build_begin_multi:
                # broadcast or radix shards behind the same build / probe calls)
                self.table = HashTable(self.parallelism, key_type, self.device, devices=self.devices,
                                       plan=self.plan)
            elif key_type != self.key_type:
                raise HjError(HJ_ERR_INVALID, "all build batches must have the same key type")
            return self.table

    def build_rows(self) -> int:
        """Rows of all partitions' build batches (complete once the barrier is passed)."""
        return sum(n for part in self.batches for _, n in part)

    def concatenated(self) -> DeviceRecordBatch:
        """Build RecordBatch in canonical order (partition 0 batches, then 1, ...): row i
        <-> build index i, concatenated on the device from the batches' resident columns
        (cooperatively_concatenate_arrow_arrays,
        src/operator/version10/parallel_join_execution_state.rs:256-298): no host
        combine_chunks and no second upload."""
        with self.lock:
            if self.record_batch is None:
                parts = [b for part in self.batches for b in part]
                schema = self.schema or pa.schema([])
                if parts:
                    ncol = len(parts[0][0])
                    cols = [DeviceColumn.concat([p[0][j] for p in parts]) for j in range(ncol)]
                    self.record_batch = DeviceRecordBatch(schema, cols, sum(p[1] for p in parts))
                    # the per-batch columns are no longer needed (the table keeps the key
                    # tensors it borrows alive itself): drop them, keep the row counts
                    self.batches = [[(None, n) for _, n in part] for part in self.batches]
                else:
                    dev = torch.device("cuda", self.device)
                    empty = [DeviceColumn.from_arrow(pa.array([], type=f.type), dev) for f in schema]
                    self.record_batch = DeviceRecordBatch(schema, empty, 0)
            return self.record_batch

    def key_filter(self) -> "KeyFilter | None":
        """With prefilter on: one filter for all partitions, built by the first probe from
        the concatenated build batch's key column (the composite int64 keys of several /
        non-integer key columns: hashes, so the automatic kind is a Bloom filter)."""
        if not self.prefilter:
            return None
        rb = self.concatenated()  # takes the lock itself
        with self.lock:
            if self._filter is None:
                kcols = [rb.device_columns[e if isinstance(e, int) else rb.schema.get_field_index(e)]
                         for e in self.key_exprs]
                if rb.num_rows == 0:
                    self._filter = KeyFilter(self.device)  # an empty build: rejects every row
                elif self.composite:
                    keys, valid = composite_keys(kcols)
                    self._filter = KeyFilter.from_keys(keys, valid)
                else:
                    k = kcols[0]
                    self._filter = KeyFilter.from_keys(k.key_tensor(), k.valid, valid_offset=k.voff)
            return self._filter

    def device_columns(self, rb: pa.RecordBatch, device) -> list[DeviceColumn]:
        """A host build batch's columns in HBM, uploaded once for all partitions (callers
        that pass their own RecordBatch instead of the resident one)."""
        with self.lock:
            if self._dev_cols is None:
                self._dev_cols = [DeviceColumn.from_arrow(c, device) for c in rb.columns]
            return self._dev_cols


class BuildImplementation:
    """src/operator/build_implementation.rs:20-112 with the `Gpu` arm only."""

    def __init__(self, build_implementation_version: JoinReplacement, parallelism: int,
                 input_schema: pa.Schema | None = None, device: int = 0, devices: Sequence[int] | None = None,
                 plan: str = "auto", prefilter: bool = False, match_probe: bool = False,
                 max_output_rows: int | None = None, filtered_probe: bool = False):
        """max_output_rows: None (default) changes nothing. An integer N >= 1 bounds the memory
        of every probe batch by N instead of by the join's fan-out: the batch's pairs are
        planned once (HashTable.pair_plan) and taken window by window, each of at most N
        candidate pairs, which pass the equality re-check and the JoinFilter, are marked and
        gathered before the next window is written, so no pair buffer and no gathered column
        exceeds N rows. probe_batch then returns a list of RecordBatches of at most N rows
        each - the same rows in the same order as without the bound - and
        finalize_build_side emits in chunks of at most N as well. Not with `devices=` (a
        multi-GPU table has no pair plan): HjError(HJ_ERR_INVALID) here, since a memory
        bound that is silently ignored is worse than an error. match_probe=True keeps its
        path for the joins it takes; its selected rows are chunked.
        prefilter: every probe first drops the rows a key filter over the build keys
        rejects (KeyFilter; same output for every join type: the filter only removes rows
        that have no pair).
        match_probe: LeftSemi, LeftAnti, RightSemi and RightAnti probe batches ask the table
        only whether each row has a partner (HashTable.probe_match: a bitmap and the build
        marks, no pairs) when the table lives on one device and the join has no filter or a
        CompareFilter - then the partner must also pass it (hj_probe_match_filtered: the walk
        over a key's build rows and the comparisons stay in registers and stop at the first
        passing pair). The key is one Int32/Int64 column, or a composite key of integer,
        boolean, date / time / timestamp / duration and Utf8 / Binary columns (the same type
        on both sides): its 64-bit hash goes to the table and one `==` term per key column
        joins the predicate. The remaining cases silently take the pair path: a callable
        JoinFilter, `devices=`, float / decimal key columns, and predicates beyond 16 terms
        or 16 columns of a side. The
        output is the same. The match path does not use the key filter: with prefilter=True
        too, the filter serves only the probes that take the pair path. Off by default: the
        match path reads the table at random where the pair path's sliced probe reads it out
        of LDS, and on large uniform joins it measured slower (C2 RightSemi 1.16 ms against
        0.89 ms, LeftSemi 1.61 against 1.55 ms). It wins where keys repeat: a
        key of c build rows hit by m probe rows costs m + c, not m * c (1000 rows per key:
        0.08 ms against 22.9 ms), and it runs joins whose pairs no buffer holds.
        filtered_probe: Inner, Left, Right and Full probe batches under a CompareFilter - or
        on a composite key without a filter, whose candidates then only have to pass the key
        equalities - write only the pairs that pass (HashTable.pair_plan(predicate=...),
        hj_pair_plan_filtered): a count walk evaluates every candidate in registers and also
        leaves the visited build rows (Left / Full) and the matched-probe bitmap (Right /
        Full), a second walk writes the passing pairs at scanned offsets. The candidate pairs
        of the equi-join, hj_filter_equal_pairs and the select never touch memory. The same
        conditions as match_probe's: the table on one device, a non-empty build side, one
        Int32/Int64 key column or a composite key of exact `==` columns within 16 terms and
        columns. With max_output_rows=N every emitted batch then has up to N *passing* pairs
        and no window is empty. The remaining cases silently take the pair path: a callable
        JoinFilter, `devices=`, float / decimal / 16-byte key columns, more than 16 terms or
        columns, and semi / anti joins (match_probe's). Output rows and their order are the
        same. This path does not use the key filter: with prefilter=True too, the filter
        serves only the probes that take the pair path. Off by default: every candidate is
        evaluated twice. Measured: on 10^9 candidates of which 9.5 % pass,
        1.16 GB of buffers instead of 24 GB at 5 % more time; 1.31 x faster where nearly all
        pass; 0.40 x on a join of one pair per match; and 0.13 x with max_output_rows = 2^20
        over keys of 1000 rows, where a window keeps only a few workgroups busy.
        devices: build one table over these GPUs of the node (hj_build_begin_multi;
        DataFusion runs every partition in one process, so the in-process multi-GPU table
        is the drop-in's node-wide form); plan "auto" | "broadcast" | "radix" (the build
        side sharded by key hash, 1/G per GPU: builds larger than one GPU). Batches and
        probe keys live on devices[0]; the table moves rows to the other GPUs itself."""
        if build_implementation_version is not JoinReplacement.Gpu:
            raise NotImplementedError(
                f"{build_implementation_version} is one of the reference's CPU strategies; this package "
                "implements JoinReplacement.Gpu")
        if devices is not None and len(devices) < 1:
            raise HjError(HJ_ERR_INVALID, "devices must name at least one GPU")
        if max_output_rows is not None:
            if isinstance(max_output_rows, bool) or not isinstance(max_output_rows, int) or max_output_rows < 1:
                raise HjError(HJ_ERR_INVALID, "max_output_rows must be None or an integer >= 1")
            if devices is not None:
                raise HjError(HJ_ERR_INVALID, "max_output_rows is not available on a multi-GPU table (devices=): "
                                              "the pair plan is defined for one-device tables")
        self.parallelism = parallelism
        self._shared = _SharedBuild(parallelism, device, devices, plan, prefilter, match_probe, max_output_rows,
                                    bool(filtered_probe))
        self._shared.schema = input_schema

    def build_side(self, partition: int, stream: Iterable[pa.RecordBatch], build_expressions: Sequence[str | int],
                   consumer):
        """Consume one partition's build stream, take part in the cross-partition
        barrier, and hand (lookup, build RecordBatch) to `consumer`. All `parallelism`
        partitions must call this concurrently (the last arriver builds the table)."""
        sh = self._shared
        with sh.lock:
            if partition < 0 or partition >= sh.parallelism:
                raise HjError(HJ_ERR_INVALID, f"bad partition {partition}")
            if sh.taken[partition]:
                raise HjError(HJ_ERR_INVALID, f"State already consumed for partition {partition}")
            sh.taken[partition] = True
        if len(build_expressions) < 1:
            raise HjError(HJ_ERR_INVALID, "an equi-join needs at least one key column")
        with sh.lock:
            sh.key_exprs = list(build_expressions)
        dev = torch.device("cuda", sh.device)
        for batch in stream:
            with sh.lock:
                if sh.schema is None:
                    sh.schema = batch.schema
            if batch.num_rows == 0:
                continue
            # the batch's columns go to HBM once: the table reads its key column there, and
            # the concatenated build batch is assembled from them on the device
            dcols = [DeviceColumn.from_arrow(c, dev) for c in batch.columns]
            sh.batches[partition].append((dcols, batch.num_rows))
            arrays = evaluate_expressions(build_expressions, batch)
            kcols = [dcols[e if isinstance(e, int) else batch.schema.get_field_index(e)] for e in build_expressions]
            if _is_simple_key(arrays):
                k = kcols[0]
                sh.table_for(_key_type(arrays[0])).append(partition, k.key_tensor(), valid=k.valid,
                                                          valid_offset=k.voff)
            else:  # calculate_hash over every key column -> one int64 key per row
                keys, valid = composite_keys(kcols)
                with sh.lock:
                    sh.composite = True
                sh.table_for("int64").append(partition, keys, valid=valid)
        # every partition waits for every other before the table exists for all of them
        sh.ready.wait()
        table = sh.table_for(sh.key_type or "int64")
        table.finish(partition)
        return consumer.call(GpuIndexLookup(table, sh), sh.concatenated())


def _apply_filter(flt: "JoinFilter | CompareFilter", build_cols: list[DeviceColumn], build_names: Sequence[str],
                  probe_cols: list[DeviceColumn], probe_names: Sequence[str], b: torch.Tensor, p: torch.Tensor):
    """apply_join_filter_to_indices: evaluate the filter on the candidate rows, keep the
    pairs where it is true (order preserved)."""
    if b.numel() == 0:
        return b, p
    if isinstance(flt, CompareFilter):  # on the device: nothing is gathered or copied to the host
        nb = build_cols[0].length if build_cols else 0
        np_ = probe_cols[0].length if probe_cols else 0
        return pair_filter_select(flt.predicate(build_cols, build_names, probe_cols, probe_names, nb, np_), b, p)
    lsel = [i for i, n in enumerate(build_names) if flt.left_columns is None or n in flt.left_columns]
    rsel = [i for i, n in enumerate(probe_names) if flt.right_columns is None or n in flt.right_columns]
    left = _batch([build_cols[i].take(b) for i in lsel], [build_names[i] for i in lsel])
    right = _batch([probe_cols[i].take(p) for i in rsel], [probe_names[i] for i in rsel])
    mask = flt.expression(left, right)
    if isinstance(mask, pa.ChunkedArray):
        mask = mask.combine_chunks()
    keep = np.asarray(mask.fill_null(False).to_numpy(zero_copy_only=False), dtype=np.uint8)
    rows = select_rows(torch.from_numpy(keep).to(b.device), 1, len(keep))
    return b[rows], p[rows]


_MATCH_JOINS = (JoinType.LeftSemi, JoinType.LeftAnti, JoinType.RightSemi, JoinType.RightAnti)


def _exact_eq_key_type(t: pa.DataType) -> bool:
    """Key column types whose pair-predicate `==` is equality of the key values: ints, uints,
    bool, date / time / timestamp / duration, Utf8 / LargeUtf8 / Binary / LargeBinary. Not
    floats (the totalOrder `==` of a widened float32 is not bit equality for signalling
    NaNs) and not 16-byte columns (no term can name them)."""
    ty = pa.types
    return (ty.is_integer(t) or ty.is_boolean(t) or ty.is_date(t) or ty.is_time(t) or ty.is_timestamp(t)
            or ty.is_duration(t) or t in (pa.string(), pa.large_string(), pa.binary(), pa.large_binary()))


def _simple_match_key(lookup: GpuIndexLookup, key_cols: Sequence[DeviceColumn]) -> bool:
    return not lookup._shared.composite and _is_simple_key(key_cols)


def _takes_match_path(jt: JoinType, filter, lookup: GpuIndexLookup, key_cols: Sequence[DeviceColumn], n: int,
                      build_side_records=None) -> bool:
    """BuildImplementation(match_probe=True): a semi / anti join on a one-device table, without
    a filter or under a CompareFilter (a callable JoinFilter needs gathered rows: the pair
    path). Keyed by one Int32/Int64 column, or by a composite key whose every column has an
    exact `==` term (_exact_eq_key_type, the same type on both sides): the table only holds
    the 64-bit hashes of such keys, one `==` term per key column after the filter's own makes
    the match exact. More than 16 terms, or 16 columns of a side, keep the pair path."""
    sh = lookup._shared
    if not (sh is not None and sh.match_probe and jt in _MATCH_JOINS and n > 0 and lookup.table.devices is None):
        return False
    if lookup.build_is_empty:  # the pair path answers without the table
        return False
    return _device_predicate_ok(filter, lookup, key_cols, build_side_records)


def _device_predicate_ok(filter, lookup: GpuIndexLookup, key_cols: Sequence[DeviceColumn], build_side_records) -> bool:
    """The rule _takes_match_path states for the filter and the key (shared with the filtered
    pair plan): no filter or a CompareFilter; one Int32/Int64 key column, or a composite key
    of exact `==` columns whose terms and columns stay within 16 with the filter's."""
    sh = lookup._shared
    if filter is not None and not isinstance(filter, CompareFilter):
        return False
    if _simple_match_key(lookup, key_cols):
        return True
    if build_side_records is None or len(key_cols) != len(sh.key_exprs):
        return False
    schema = build_side_records.schema
    for e, k in zip(sh.key_exprs, key_cols):
        bt = schema.field(e).type
        if bt != k.type or not _exact_eq_key_type(bt):
            return False
    nk = len(key_cols)
    nt, nl, nr = (len(filter.terms), len(filter._names(L)), len(filter._names(R))) if filter is not None else (0, 0, 0)
    return nt + nk <= 16 and nl + nk <= 16 and nr + nk <= 16


def _probe_keys_and_predicate(filter: "CompareFilter | None", build_side_records, lookup: GpuIndexLookup,
                              probe_batch: pa.RecordBatch, probe_cols: list[DeviceColumn],
                              key_cols: list[DeviceColumn]):
    """(keys, valid, valid_offset, predicate) of one probe batch for the table's predicate
    calls (_device_predicate_ok holds): the key tensor of one Int32/Int64 column or the
    composite hashes, and the predicate _apply_filter would build plus one `==` term per
    column of a composite key. predicate is None without a filter on one Int32/Int64 key."""
    n = probe_batch.num_rows
    simple = _simple_match_key(lookup, key_cols)
    if simple:
        k = key_cols[0]
        keys, valid, voff = k.key_tensor(), k.valid, k.voff
    else:
        (keys, valid), voff = composite_keys(key_cols), 0
    if simple and filter is None:
        return keys, valid, voff, None
    build_cols = lookup.build_columns(build_side_records)
    bnames, nb = list(build_side_records.schema.names), build_side_records.num_rows
    eq = []
    if not simple:
        sh = lookup._shared
        eq = [(build_cols[e if isinstance(e, int) else build_side_records.schema.get_field_index(e)], k)
              for e, k in zip(sh.key_exprs, key_cols)]
    if filter is not None:
        pred = filter.predicate(build_cols, bnames, probe_cols, list(probe_batch.schema.names), nb, n, eq_keys=eq)
    else:
        pred = PairPredicate([b for b, _ in eq], [p for _, p in eq],
                             [(("build", i), "==", ("probe", i)) for i in range(len(eq))], nb, n)
    return keys, valid, voff, pred


_PAIR_JOINS = (JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.Full)


def _takes_filtered_path(jt: JoinType, filter, lookup: GpuIndexLookup, key_cols: Sequence[DeviceColumn], n: int,
                         build_side_records=None) -> bool:
    """BuildImplementation(filtered_probe=True): an Inner, Left, Right or Full join on a
    one-device table under a CompareFilter - or on a composite key without a filter, whose
    predicate is the key equalities alone - with a key _device_predicate_ok accepts. Then only
    the pairs that pass reach memory (HashTable.pair_plan(predicate=...)). Everything else
    keeps the pair path."""
    sh = lookup._shared
    if not (sh is not None and sh.filtered_probe and jt in _PAIR_JOINS and n > 0 and lookup.table.devices is None):
        return False
    if lookup.build_is_empty:
        return False
    if not _device_predicate_ok(filter, lookup, key_cols, build_side_records):
        return False
    return filter is not None or not _simple_match_key(lookup, key_cols)


def _filtered_plan(jt: JoinType, filter: "CompareFilter | None", build_side_records, lookup: GpuIndexLookup,
                   probe_batch: pa.RecordBatch, probe_cols: list[DeviceColumn], key_cols: list[DeviceColumn],
                   build_visited: torch.Tensor | None):
    """The filtered pair plan of one probe batch (_takes_filtered_path holds). The one count
    walk also leaves the outer joins' bookkeeping: the visited build rows of Left / Full
    (set_ones) and the matched-probe bitmap of Right / Full, so no mark_rows over pairs."""
    keys, valid, voff, pred = _probe_keys_and_predicate(filter, build_side_records, lookup, probe_batch, probe_cols,
                                                        key_cols)
    flags = build_visited if jt in (JoinType.Left, JoinType.Full) else None
    return lookup.table.pair_plan(keys, valid, valid_offset=voff, predicate=pred, build_flags=flags,
                                  bitmap=jt in (JoinType.Right, JoinType.Full))


def _match_probe(jt: JoinType, filter: "CompareFilter | None", build_side_records, lookup: GpuIndexLookup,
                 probe_batch: pa.RecordBatch, probe_cols: list[DeviceColumn], key_cols: list[DeviceColumn],
                 build_visited: torch.Tensor | None) -> torch.Tensor | None:
    """The match path of one probe batch (_takes_match_path holds): no pairs. Left joins mark
    `build_visited` (set_ones) and return None; right joins return the selected probe rows
    (get_semi_indices / get_anti_indices) from the matched-probe bitmap. Without a filter on
    one Int32/Int64 key: HashTable.probe_match as is. Else the filtered match probe, under the
    predicate _apply_filter would build, plus the key equalities of a composite key."""
    left = jt in (JoinType.LeftSemi, JoinType.LeftAnti)
    flags = build_visited if left else None
    keys, valid, voff, pred = _probe_keys_and_predicate(filter, build_side_records, lookup, probe_batch, probe_cols,
                                                        key_cols)
    n = probe_batch.num_rows
    if pred is None:
        m = lookup.table.probe_match(keys, valid, valid_offset=voff, build_flags=flags)
    else:
        m = lookup.table.probe_match(keys, valid, valid_offset=voff, build_flags=flags, predicate=pred,
                                     bitmap=not left)
    if left:
        return None
    return select_bitmap(m.bitmap, n, 1 if jt is JoinType.RightSemi else 0)


def probe_batch(join_type: JoinType, probe_expressions: Sequence[str | int], build_expressions: Sequence[str | int],
                filter: "JoinFilter | CompareFilter | None", build_side_records: pa.RecordBatch, read_only_join_map: GpuIndexLookup,
                probe_batch: pa.RecordBatch, build_visited: torch.Tensor | None = None
                ) -> pa.RecordBatch | list[pa.RecordBatch] | None:
    """One probe batch of any join type: the lookup_*_probe_batch functions of
    src/operator/probe_lookup_implementation/{inner,left_outer,right_outer,full,left_semi,
    left_anti,right_semi,right_anti}.rs. Build-side join types only mark `build_visited`
    here (their rows are emitted by finalize_build_side). Under max_output_rows
    (BuildImplementation) the result is a list of RecordBatches of at most that many rows."""
    jt = JoinType.parse(join_type)
    lookup = read_only_join_map
    dev = lookup.device
    n = probe_batch.num_rows
    # the probe batch goes to HBM once: its key columns feed the lookup, all columns the take
    probe_cols = [DeviceColumn.from_arrow(c, dev) for c in probe_batch.columns]
    key_cols = [probe_cols[e if isinstance(e, int) else probe_batch.schema.get_field_index(e)]
                for e in probe_expressions]
    limit = lookup._shared.max_output_rows if lookup._shared is not None else None
    if limit is not None:
        return _probe_batch_windowed(jt, filter, build_side_records, lookup, probe_batch, probe_cols, key_cols,
                                     build_visited, limit)
    if _takes_match_path(jt, filter, lookup, key_cols, n, build_side_records):
        # no pairs: the matched-probe bitmap (get_semi_indices / get_anti_indices) and the
        # visited build rows (set_ones) straight from the lookup
        rows = _match_probe(jt, filter, build_side_records, lookup, probe_batch, probe_cols, key_cols, build_visited)
        if rows is None:
            return None
        return _batch([c.take(rows) for c in probe_cols], list(probe_batch.schema.names))
    if _takes_filtered_path(jt, filter, lookup, key_cols, n, build_side_records):
        # only the passing pairs are written; marks and the unmatched probe rows come from the plan
        plan = _filtered_plan(jt, filter, build_side_records, lookup, probe_batch, probe_cols, key_cols, build_visited)
        b, p = plan.all()
        if jt in (JoinType.Right, JoinType.Full):
            unmatched = select_bitmap(plan.bitmap, n, 0)
            b = torch.cat([b, torch.full((unmatched.numel(),), -1, dtype=torch.int64, device=dev)])
            p = torch.cat([p, unmatched])
        build_cols = lookup.build_columns(build_side_records)
        return _batch([c.take(b) for c in build_cols] + [c.take(p) for c in probe_cols],
                      list(build_side_records.schema.names) + list(probe_batch.schema.names))
    b, p = lookup.matching_indices_device(key_cols, build_side_records)
    build_cols = lookup.build_columns(build_side_records)
    bnames, pnames = list(build_side_records.schema.names), list(probe_batch.schema.names)
    if filter is not None:
        b, p = _apply_filter(filter, build_cols, bnames, probe_cols, pnames, b, p)
    if jt.marks_build and build_visited is not None:
        mark_rows(b, build_side_records.num_rows, build_visited)
    if jt in (JoinType.LeftSemi, JoinType.LeftAnti):
        return None
    if jt in (JoinType.RightSemi, JoinType.RightAnti):
        flags = mark_rows(p, n)
        rows = select_rows(flags, 1 if jt is JoinType.RightSemi else 0, n).to(torch.int32)
        return _batch([c.take(rows) for c in probe_cols], pnames)
    if jt in (JoinType.Right, JoinType.Full):
        # append_right_indices(preserve_order = false): unmatched probe rows after the pairs
        unmatched = select_rows(mark_rows(p, n), 0, n).to(torch.int32)
        b = torch.cat([b, torch.full((unmatched.numel(),), -1, dtype=torch.int64, device=dev)])
        p = torch.cat([p, unmatched])
    return _batch([c.take(b) for c in build_cols] + [c.take(p) for c in probe_cols], bnames + pnames)


def _row_chunks(rows: torch.Tensor, limit: int) -> list[torch.Tensor]:
    """`rows` in consecutive pieces of at most `limit` (one empty piece for no rows: the
    unbounded path emits an empty batch there too)."""
    return [rows[lo:lo + limit] for lo in range(0, rows.numel(), limit)] or [rows]


def _probe_batch_windowed(jt: JoinType, filter: "JoinFilter | CompareFilter | None", build_side_records: pa.RecordBatch,
                          lookup: GpuIndexLookup, probe_batch: pa.RecordBatch, probe_cols: list[DeviceColumn],
                          key_cols: list[DeviceColumn], build_visited: torch.Tensor | None,
                          limit: int) -> list[pa.RecordBatch]:
    """probe_batch under max_output_rows: the same rows in the same order as the unbounded
    path, as RecordBatches of at most `limit` rows. The pairs come window by window
    (GpuIndexLookup.matching_windows); each window is re-checked, filtered, marked and
    gathered before the next one exists. The flags of both sides accumulate over the
    windows; the once-per-batch rows (unmatched probe rows of Right / Full, the selected
    rows of RightSemi / RightAnti) follow the last window in chunks."""
    dev = lookup.device
    n = probe_batch.num_rows
    pnames = list(probe_batch.schema.names)
    if _takes_match_path(jt, filter, lookup, key_cols, n, build_side_records):
        rows = _match_probe(jt, filter, build_side_records, lookup, probe_batch, probe_cols, key_cols, build_visited)
        if rows is None:
            return []
        return [_batch([c.take(r) for c in probe_cols], pnames) for r in _row_chunks(rows, limit)]
    build_cols = lookup.build_columns(build_side_records)
    bnames = list(build_side_records.schema.names)
    emits_pairs = jt in (JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.Full)
    probe_side = jt in (JoinType.Right, JoinType.Full, JoinType.RightSemi, JoinType.RightAnti)
    if _takes_filtered_path(jt, filter, lookup, key_cols, n, build_side_records):
        # windows of passing pairs: every batch has up to `limit` of them, none is empty
        plan = _filtered_plan(jt, filter, build_side_records, lookup, probe_batch, probe_cols, key_cols, build_visited)
        out = [_batch([c.take(b) for c in build_cols] + [c.take(p) for c in probe_cols], bnames + pnames)
               for b, p in plan.windows(limit)]
        if jt in (JoinType.Right, JoinType.Full):
            unmatched = select_bitmap(plan.bitmap, n, 0)
            for r in _row_chunks(unmatched, limit) if unmatched.numel() else []:
                nulls = torch.full((r.numel(),), -1, dtype=torch.int64, device=dev)
                out.append(_batch([c.take(nulls) for c in build_cols] + [c.take(r) for c in probe_cols],
                                  bnames + pnames))
        if not out:  # no row at all: the empty batch the unbounded path returns
            e_b = torch.empty(0, dtype=torch.int64, device=dev)
            e_p = torch.empty(0, dtype=torch.int32, device=dev)
            out.append(_batch([c.take(e_b) for c in build_cols] + [c.take(e_p) for c in probe_cols], bnames + pnames))
        return out
    probe_flags = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) if probe_side else None
    out = []
    for b, p in lookup.matching_windows(key_cols, limit, build_side_records):
        if filter is not None:
            b, p = _apply_filter(filter, build_cols, bnames, probe_cols, pnames, b, p)
        if b.numel() == 0:
            continue
        if jt.marks_build and build_visited is not None:
            mark_rows(b, build_side_records.num_rows, build_visited)
        if probe_side:
            mark_rows(p, n, probe_flags)
        if emits_pairs:
            out.append(_batch([c.take(b) for c in build_cols] + [c.take(p) for c in probe_cols], bnames + pnames))
    if jt in (JoinType.LeftSemi, JoinType.LeftAnti):
        return []
    if jt in (JoinType.RightSemi, JoinType.RightAnti):
        rows = select_rows(probe_flags, 1 if jt is JoinType.RightSemi else 0, n).to(torch.int32)
        return [_batch([c.take(r) for c in probe_cols], pnames) for r in _row_chunks(rows, limit)]
    if jt in (JoinType.Right, JoinType.Full):
        # append_right_indices(preserve_order = false): unmatched probe rows after the pairs
        unmatched = select_rows(probe_flags, 0, n).to(torch.int32)
        for r in _row_chunks(unmatched, limit) if unmatched.numel() else []:
            nulls = torch.full((r.numel(),), -1, dtype=torch.int64, device=dev)
            out.append(_batch([c.take(nulls) for c in build_cols] + [c.take(r) for c in probe_cols], bnames + pnames))
    if not out:  # no row at all: the empty batch the unbounded path returns
        e_b = torch.empty(0, dtype=torch.int64, device=dev)
        e_p = torch.empty(0, dtype=torch.int32, device=dev)
        out.append(_batch([c.take(e_b) for c in build_cols] + [c.take(e_p) for c in probe_cols], bnames + pnames))
    return out


def finalize_build_side(join_type: JoinType, build_side_records: pa.RecordBatch, lookup: GpuIndexLookup,
                        build_visited: torch.Tensor, probe_schema: pa.Schema
                        ) -> pa.RecordBatch | list[pa.RecordBatch] | None:
    """The once-only build-side emission of the last finishing partition
    (emit_matched_build_records / emit_unmatched_build_records, e.g.
    left_semi.rs:166-178, left_outer.rs:174-193, full.rs:181-200). Under max_output_rows: a
    list of RecordBatches of at most that many rows each."""
    jt = JoinType.parse(join_type)
    if not jt.marks_build:
        return None
    nb = build_side_records.num_rows
    rows = select_rows(build_visited, 1 if jt is JoinType.LeftSemi else 0, nb)
    cols = lookup.build_columns(build_side_records)
    limit = lookup._shared.max_output_rows if lookup._shared is not None else None

    def emit(r: torch.Tensor) -> pa.RecordBatch:
        out = [c.take(r).to_arrow() for c in cols]
        names = list(build_side_records.schema.names)
        if jt in (JoinType.Left, JoinType.Full):
            out += [pa.nulls(r.numel(), type=f.type) for f in probe_schema]
            names += list(probe_schema.names)
        return pa.RecordBatch.from_arrays(out, names=names)

    if limit is not None:
        return [emit(r) for r in _row_chunks(rows, limit)]
    return emit(rows)


def lookup_inner_join_probe_batch(probe_expressions: Sequence[str | int], build_expressions: Sequence[str | int],
                                  filter, build_side_records: pa.RecordBatch, read_only_join_map: GpuIndexLookup,
                                  probe_batch: pa.RecordBatch, output_schema: pa.Schema | None = None
                                  ) -> pa.RecordBatch | list[pa.RecordBatch]:
    """src/operator/probe_lookup_implementation/inner.rs:79-129 (a list of RecordBatches
    under max_output_rows)."""
    rb = globals()["probe_batch"](JoinType.Inner, probe_expressions, build_expressions, filter, build_side_records,
                                  read_only_join_map, probe_batch)
    if isinstance(rb, list):
        return [pa.RecordBatch.from_arrays(r.columns, schema=output_schema) if output_schema is not None else r
                for r in rb]
    if output_schema is not None:
        return pa.RecordBatch.from_arrays(rb.columns, schema=output_schema)
    return rb


class _Finalizer:
    """LimitedRc<()> over `parallelism` copies: the last release runs the build-side
    emission (src/utils/limited_rc.rs, InitializeCopiesOnce)."""

    def __init__(self, parallelism: int):
        self.left = parallelism
        self.lock = threading.Lock()
        self.visited: torch.Tensor | None = None

    def visited_for(self, nrows: int, device) -> torch.Tensor:
        with self.lock:
            if self.visited is None:
                self.visited = torch.zeros(max(nrows, 1), dtype=torch.uint8, device=device)
            return self.visited

    def release(self) -> bool:
        with self.lock:
            self.left -= 1
            return self.left == 0


class _ProbeConsumer:
    """PerformProbeLookup (src/operator/parallel_hash_join_executor.rs:20-68)."""

    def __init__(self, probe_stream, probe_expressions, build_expressions, join_type=JoinType.Inner, filter=None,
                 finalizer: _Finalizer | None = None, probe_schema: pa.Schema | None = None):
        self.probe_stream = probe_stream
        self.probe_expressions = probe_expressions
        self.build_expressions = build_expressions
        self.join_type = JoinType.parse(join_type)
        self.filter = filter
        self.finalizer = finalizer
        self.probe_schema = probe_schema

    def call(self, lookup: GpuIndexLookup, record_batch: pa.RecordBatch):
        jt = self.join_type
        visited = None
        if jt.marks_build:
            visited = self.finalizer.visited_for(record_batch.num_rows, lookup.device)
        out = []
        for b in self.probe_stream:
            rb = probe_batch(jt, self.probe_expressions, self.build_expressions, self.filter, record_batch, lookup, b,
                             visited)
            if isinstance(rb, list):  # max_output_rows: the batch's output in bounded pieces
                out.extend(rb)
            elif rb is not None:
                out.append(rb)
        if jt.marks_build and self.finalizer.release():
            rb = finalize_build_side(jt, record_batch, lookup, visited, self.probe_schema)
            if isinstance(rb, list):
                out.extend(rb)
            elif rb is not None:
                out.append(rb)
        return out


class ParallelHashJoin:
    """src/operator/parallel_hash_join.rs:16-168: `left` is the build side, `right` the
    probe side, each a list of partitions (lists of RecordBatches); `join_type` one of
    JoinType (names as DataFusion's); `filter` an optional JoinFilter (host
    callable) or CompareFilter (comparisons, filtered on the device). Output
    partitioning follows the probe side (RoundRobinBatch(N), 85-91); build-side rows of
    Left / Full / LeftSemi / LeftAnti joins come from the last partition to finish."""

    def __init__(self, left: list[list[pa.RecordBatch]], right: list[list[pa.RecordBatch]],
                 on: Sequence[tuple[str, str]], join_type: JoinType | str = JoinType.Inner, device: int = 0,
                 replacement: JoinReplacement = JoinReplacement.Gpu, filter: "JoinFilter | CompareFilter | None" = None,
                 right_schema: pa.Schema | None = None, devices: Sequence[int] | None = None, plan: str = "auto",
                 prefilter: bool = False, match_probe: bool = False, max_output_rows: int | None = None,
                 filtered_probe: bool = False):
        """max_output_rows: None, or the most rows any output batch, pair buffer or gathered
        column may have (BuildImplementation; same rows in the same order, in more batches;
        not with `devices=`);
        devices / plan: one build table over several GPUs (BuildImplementation);
        prefilter: probe through a key filter over the build keys (BuildImplementation);
        match_probe: semi and anti joins on one device, without a filter or under a
        CompareFilter, probe for matches instead of pairs (BuildImplementation; same output;
        the match path ignores the key filter; a callable JoinFilter, float / decimal key
        columns and other joins silently take the pair path);
        filtered_probe: Inner / Left / Right / Full joins on one device under a CompareFilter,
        or on a composite key, write only the pairs that pass (BuildImplementation; same
        output; ignores the key filter; the other cases silently take the pair path)."""
        if len(on) < 1:
            raise HjError(HJ_ERR_INVALID, "an equi-join needs at least one (left, right) key pair")
        self.join_type = JoinType.parse(join_type)
        n = max(len(left), len(right), 1)
        self.left = list(left) + [[] for _ in range(n - len(left))]
        self.right = list(right) + [[] for _ in range(n - len(right))]
        self.parallelism = n
        self.on = list(on)
        self.filter = filter
        self.right_schema = right_schema or next((b.schema for part in self.right for b in part), None)
        self._build = BuildImplementation(replacement, n, device=device, devices=devices, plan=plan,
                                          prefilter=prefilter, match_probe=match_probe,
                                          max_output_rows=max_output_rows, filtered_probe=filtered_probe)
        self._finalizer = _Finalizer(n)

    def execute(self, partition: int) -> list[pa.RecordBatch]:
        lkeys, rkeys = [l for l, _ in self.on], [r for _, r in self.on]
        consumer = _ProbeConsumer(self.right[partition], rkeys, lkeys, self.join_type, self.filter, self._finalizer,
                                  self.right_schema)
        return self._build.build_side(partition, self.left[partition], lkeys, consumer)

    def collect(self) -> list[pa.RecordBatch]:
        """DataFusion `collect`: execute every partition concurrently."""
        with ThreadPoolExecutor(max_workers=self.parallelism) as ex:
            futs = [ex.submit(self.execute, p) for p in range(self.parallelism)]
            out = []
            for f in futs:
                out.extend(f.result())
        return out
