"""Plain Python model of a join's output *rows*, written from the text of include/hj.h
(hj_key_column: "a null key never matches", "values compare byte-exactly ... for floats ...
equal bits") and the row rules of model() in test_gpu_join_types.py. Shared by the CPU and GPU
tests; no GPU and no library call in here.

  join_rows(left, right, on, join_type)   the rows of the join as a list of tuples of Python
                                          values (Table.to_pylist's), left = build side,
                                          right = probe side, left columns then right columns
  canon(rows)                             the rows as a sorted list with every float replaced
                                          by its bit pattern: joins compare as multisets

The second half makes the inputs of the tests: sides(kind, ...) gives a build and a probe
RecordBatch with the key columns of one key kind and payload columns of every column type.
"""
import datetime
import decimal
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

JOIN_TYPES = ["inner", "left", "right", "full", "leftsemi", "leftanti", "rightsemi", "rightanti"]


# ---- the model ---------------------------------------------------------------------

def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _key_atoms(col: pa.ChunkedArray | pa.Array) -> list:
    """One hashable atom per row whose equality is equality of the value's bytes; None for a
    null. Floats: the bit pattern, read from the column's buffer (0.0 != -0.0, a NaN equals
    the NaN of the same bits). Utf8 / Binary: the bytes. Everything else: the Python value
    (ints, bools, dates, decimals of one scale: equal values have equal bytes)."""
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    t = col.type
    valid = col.is_valid().to_numpy(zero_copy_only=False)
    if pa.types.is_floating(t):
        raw = pc.fill_null(col, 0.0).to_numpy(zero_copy_only=False)
        ints = raw.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[raw.dtype.itemsize])
        return [("f", int(b)) if v else None for b, v in zip(ints, valid)]
    vals = col.to_pylist()
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return [None if v is None else v.encode("utf-8") for v in vals]
    return vals


def join_rows(left: pa.Table, right: pa.Table, on, join_type: str) -> list[tuple]:
    """`on`: (left name, right name) pairs. A row whose key tuple holds a null matches
    nothing; inner pairs for every (build row, probe row) of equal key tuples; `left` adds
    the unmatched build rows with a null probe side, `right` the unmatched probe rows with a
    null build side, `full` both; leftsemi / leftanti the build rows with / without a
    partner, rightsemi / rightanti the probe rows."""
    if join_type not in JOIN_TYPES:
        raise ValueError(join_type)
    lrows = list(zip(*[c.to_pylist() for c in left.columns])) if left.num_columns else []
    rrows = list(zip(*[c.to_pylist() for c in right.columns])) if right.num_columns else []
    lrows = lrows if left.num_rows else []
    rrows = rrows if right.num_rows else []
    lkeys = list(zip(*[_key_atoms(left.column(l)) for l, _ in on])) if left.num_rows else []
    rkeys = list(zip(*[_key_atoms(right.column(r)) for _, r in on])) if right.num_rows else []
    table: dict[tuple, list[int]] = {}
    for i, k in enumerate(lkeys):
        if None not in k:
            table.setdefault(k, []).append(i)
    lnull, rnull = (None,) * left.num_columns, (None,) * right.num_columns
    matched_l = [False] * len(lrows)
    matched_r = [False] * len(rrows)
    inner = []
    for j, k in enumerate(rkeys):
        for i in table.get(k, ()) if None not in k else ():
            matched_l[i] = matched_r[j] = True
            inner.append(lrows[i] + rrows[j])
    um_l = [lrows[i] for i in range(len(lrows)) if not matched_l[i]]
    um_r = [rrows[j] for j in range(len(rrows)) if not matched_r[j]]
    return {
        "inner": lambda: inner,
        "left": lambda: inner + [r + rnull for r in um_l],
        "right": lambda: inner + [lnull + r for r in um_r],
        "full": lambda: inner + [lnull + r for r in um_r] + [r + rnull for r in um_l],
        "leftsemi": lambda: [lrows[i] for i in range(len(lrows)) if matched_l[i]],
        "leftanti": lambda: um_l,
        "rightsemi": lambda: [rrows[j] for j in range(len(rrows)) if matched_r[j]],
        "rightanti": lambda: um_r,
    }[join_type]()


def _tag(v):
    # None sorts before every value; a float is its bits (NaN has no order, -0.0 == 0.0)
    if v is None:
        return (0,)
    if isinstance(v, float):
        return (1, _bits(v))
    return (1, v)


def canon(rows) -> list[tuple]:
    return sorted(tuple(_tag(v) for v in r) for r in rows)


def table_rows(t: pa.Table) -> list[tuple]:
    return list(zip(*[c.to_pylist() for c in t.columns])) if t.num_rows and t.num_columns else []


# ---- inputs --------------------------------------------------------------------------

NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]   # the default quiet NaN
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000ABC))[0]   # negative, with a payload
KEY_KINDS = ["int32", "utf8", "int64_large_utf8", "date32_bool_int16", "float64", "decimal128", "int64_utf8"]
_DEC = pa.decimal128(20, 2)
_STR_LENS = [0, 1, 63, 64, 65, 200]


def _text(i: int, nbytes: int) -> str:
    """A string of exactly nbytes UTF-8 bytes that starts with the row number and goes on in
    3-, 2- and 1-byte characters."""
    head = str(i)[:nbytes]
    left = nbytes - len(head)
    n3 = left // 3 if i % 2 else left // 6
    left -= 3 * n3
    return head + "€漢"[i % 2] * n3 + "éß"[i % 2] * (left // 2) + "x" * (left % 2)


def _key_pool(kind: str, rng, size: int) -> list[tuple]:
    """`size` distinct key tuples of the kind (no nulls), near misses first: tuples that agree
    in all but one column, strings that share a prefix, +0.0 / -0.0 and two NaNs."""
    def strings(n, tag):
        return [f"{tag}-key-{i // 7}-" + "é" * (i % 7) for i in range(n)]
    if kind == "int32":
        pool = [(int(v),) for v in rng.choice(np.arange(-2**31, 2**31, 997), size, replace=False)]
    elif kind == "utf8":
        pool = [("",), ("\x00",), ("a",), ("ab",)] + [(s,) for s in strings(size - 4, "u")]
    elif kind in ("int64_large_utf8", "int64_utf8"):
        ss = strings(40, "l") + [""]
        pool = [(int(x) * 2**33 - 5, ss[(i * 7 + x) % len(ss)]) for i, x in
                enumerate(np.repeat(np.arange(size // 4 + 1), 4)[:size])]
        pool = list(dict.fromkeys(pool))
        i = 0
        while len(pool) < size:  # the repeat above makes duplicates: top up with fresh tuples
            pool.append((-1 - i, ss[i % len(ss)]))
            i += 1
    elif kind == "date32_bool_int16":
        d0 = datetime.date(1999, 12, 25)
        pool = [(d0 + datetime.timedelta(days=i // 8), bool(i & 1), (i // 2) % 4 - 2) for i in range(size)]
    elif kind == "float64":
        special = [0.0, -0.0, NAN_A, NAN_B, float("inf"), float("-inf"), 5e-324, -5e-324, 1.0, -1.0]
        pool = [(v,) for v in special] + [(float(v),) for v in rng.standard_normal(size - len(special)) * 1e6]
    elif kind == "decimal128":
        pool = [(decimal.Decimal(int(v)).scaleb(-2) * (10**9 if i % 3 == 0 else 1),)
                for i, v in enumerate(rng.choice(np.arange(-10**8, 10**8), size, replace=False))]
    else:
        raise ValueError(kind)
    assert len(pool) == size and len({tuple(_tag(v) for v in k) for k in pool}) == size, kind
    return pool


_KEY_TYPES = {
    "int32": [pa.int32()], "utf8": [pa.string()], "int64_large_utf8": [pa.int64(), pa.large_string()],
    "int64_utf8": [pa.int64(), pa.string()], "date32_bool_int16": [pa.date32(), pa.bool_(), pa.int16()],
    "float64": [pa.float64()], "decimal128": [_DEC],
}


def _masked(values: list, mask, t) -> pa.Array:
    return pa.array([None if m else v for v, m in zip(values, mask)], type=t)


def _payload(rng, n: int, clean: slice, prefix: str) -> dict:
    """Payload columns of every column type, each about 10 % null (none in rows `clean`); one
    column without nulls and one entirely null."""
    def mask():
        m = rng.random(n) < 0.10
        m[clean] = False
        return m
    f64 = [0.0, -0.0, float("inf"), float("-inf"), NAN_A, NAN_B]
    # float32: the same NaNs after narrowing (both quiet, so widening back is exact)
    lens = rng.choice(_STR_LENS, n)
    cols = {
        "i8": _masked([int(v) for v in rng.integers(-128, 128, n)], mask(), pa.int8()),
        "i16": _masked([int(v) for v in rng.integers(-2**15, 2**15, n)], mask(), pa.int16()),
        "f32": _masked([f64[i % 6] if i % 5 == 0 else float(np.float32(v)) for i, v in
                        enumerate(rng.standard_normal(n))], mask(), pa.float32()),
        "f64": _masked([f64[i % 6] if i % 4 == 0 else float(v) for i, v in enumerate(rng.standard_normal(n))],
                       mask(), pa.float64()),
        "flag": _masked([bool(v) for v in rng.integers(0, 2, n)], mask(), pa.bool_()),
        "day": _masked([datetime.date(2001, 1, 1) + datetime.timedelta(days=int(v)) for v in
                        rng.integers(0, 9000, n)], mask(), pa.date32()),
        "dec": _masked([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**17, 10**17, n)], mask(), _DEC),
        "s": _masked([_text(i, int(k)) for i, k in enumerate(lens)], mask(), pa.string()),
        "ls": _masked([f"row {i} " + "ß" * (i % 9) for i in range(n)], mask(), pa.large_string()),
        "bin": _masked([bytes(rng.integers(0, 3, int(k) % 67).astype(np.uint8)) for k in lens], mask(), pa.binary()),
        "rowid": pa.array(np.arange(n), pa.int64()),                      # no nulls at all
        "void": pa.array([None] * n, pa.string()),                        # entirely null
    }
    return {prefix + k: v for k, v in cols.items()}


def sides(kind: str, nb: int, np_: int, seed: int, clean_b: slice = slice(0, 0), clean_p: slice = slice(0, 0),
          payload: bool = True) -> tuple[pa.RecordBatch, pa.RecordBatch, list[tuple[str, str]]]:
    """(build batch, probe batch, on) of one key kind. Build keys repeat: most 1 to 3 times, a
    few about 20 times; about half the probe rows carry a build key; 3-5 % of the values of
    every key column are null, independently (none in the rows `clean_*`). Build columns are
    named l_*, probe columns r_*."""
    rng = np.random.default_rng(seed)
    nkeys = max(nb // 3, 4)
    pool = _key_pool(kind, rng, 2 * nkeys)
    # build rows: keys [0, nkeys), every 16th of them heavy
    weights = np.where(np.arange(nkeys) % 16 == 3, 20.0, 1.5)
    bsel = rng.choice(nkeys, nb, p=weights / weights.sum())
    psel = rng.integers(0, 2 * nkeys, np_)
    out = []
    for prefix, sel, n, clean in (("l_", bsel, nb, clean_b), ("r_", psel, np_, clean_p)):
        cols = {}
        for j, t in enumerate(_KEY_TYPES[kind]):
            m = rng.random(n) < 0.04
            m[clean] = False
            cols[f"{prefix}k{j}"] = _masked([pool[i][j] for i in sel], m, t)
        if payload:
            cols.update(_payload(rng, n, clean, prefix))
        out.append(pa.RecordBatch.from_pydict(cols))
    on = [(f"l_k{j}", f"r_k{j}") for j in range(len(_KEY_TYPES[kind]))]
    return out[0], out[1], on
