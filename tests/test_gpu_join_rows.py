"""GPU: the operator's output *rows* against the plain model of tests/join_rows_ref.py.

Every join type over every key kind, with payload columns of every column type on both sides
(strings around the 64-byte wave pass, binaries with zero bytes, decimals, floats with signed
zeros, infinities and NaNs, null-bearing, null-free and all-null columns), so that a gathered
value on the wrong row, a validity bit off by one or a re-based offset that is wrong shows as a
wrong row. Both sides arrive in batches cut from one table at offsets that are no multiple of
8: every array has a non-zero Arrow offset, every Utf8 / Binary piece offsets that do not
start at 0, and DeviceColumn.concat joins null-free pieces (valid is None) with null-bearing
ones, an empty partition included. Rows compare as multisets (canon): partition interleaving
is free, as in test_gpu_join_types.py."""
import functools

import pyarrow as pa
import pytest

import join_rows_ref as ref
from join_rows_ref import JOIN_TYPES, canon, join_rows

pytestmark = pytest.mark.gpu

NB, NP = 3000, 5000
LEAD = 13  # rows before the first batch: no batch starts at Arrow offset 0
# batch boundaries (rows of the side after LEAD); 790..1303 / 1990..2613 hold no null
B_CUTS = [0, 13, 13, 790, 1303, 2100, NB]
P_CUTS = [0, 1990, 2613, 2613, 3132, 4444, NP]
B_CLEAN, P_CLEAN = slice(LEAD + 790, LEAD + 1303), slice(LEAD + 1990, LEAD + 2613)


def _batches(rb: pa.RecordBatch, cuts) -> list[pa.RecordBatch]:
    return [rb.slice(LEAD + a, b - a) for a, b in zip(cuts, cuts[1:])]


@functools.lru_cache(maxsize=None)
def inputs(kind: str):
    """(build partitions, probe partitions, build table, probe table, on). Build: 4 batches
    (one of 13 rows, one empty, one null-free), no batch at all, 2 batches; probe: 1 (ending in
    the null-free rows' neighbour), 3 (one null-free, one empty), 2."""
    left, right, on = ref.sides(kind, LEAD + NB, LEAD + NP, seed=100 + ref.KEY_KINDS.index(kind),
                                clean_b=B_CLEAN, clean_p=P_CLEAN)
    lb, rbs = _batches(left, B_CUTS), _batches(right, P_CUTS)
    assert [b.num_rows for b in lb].count(0) == 1 and [b.num_rows for b in rbs].count(0) == 1
    assert all(c.offset % 8 for b in lb + rbs for c in b.columns)
    assert lb[3].column("l_s").null_count == 0 and lb[2].column("l_s").null_count > 0
    assert rbs[1].column("r_bin").null_count == 0 and rbs[0].column("r_bin").null_count > 0
    return ([lb[:4], [], lb[4:]], [rbs[:1], rbs[1:4], rbs[4:]],
            pa.Table.from_batches([left.slice(LEAD)]), pa.Table.from_batches([right.slice(LEAD)]), on)


@functools.lru_cache(maxsize=None)
def expected(kind: str, jt: str):
    _, _, left, right, on = inputs(kind)
    return canon(join_rows(left, right, on, jt))


def out_schema(jt: str, left: pa.Schema, right: pa.Schema) -> pa.Schema:
    if jt in ("leftsemi", "leftanti"):
        return left
    if jt in ("rightsemi", "rightanti"):
        return right
    return pa.schema(list(left) + list(right))


def run_join(lparts, rparts, on, jt, right_schema, **opts):
    from datafusion_parallelism_amd.operator import ParallelHashJoin

    return ParallelHashJoin(lparts, rparts, on=on, join_type=jt, right_schema=right_schema, **opts).collect()


def check(out, jt, left: pa.Schema, right: pa.Schema, want):
    schema = out_schema(jt, left, right)
    for b in out:
        assert b.schema.names == schema.names and b.schema.types == schema.types
    got = [r for b in out for r in ref.table_rows(pa.Table.from_batches([b]))]
    assert len(got) == len(want)
    assert canon(got) == want


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("kind", ["int32", "utf8", "int64_large_utf8", "date32_bool_int16", "float64", "decimal128"])
def test_rows_every_key_kind(dfp, kind, jt):
    lparts, rparts, left, right, on = inputs(kind)
    out = run_join(lparts, rparts, on, jt, right.schema)
    check(out, jt, left.schema, right.schema, expected(kind, jt))


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("option", ["prefilter", "match_probe", "max_output_rows"])
def test_rows_under_options(dfp, option, jt):
    """The (int64, utf8) key under the key filter, the match probe and bounded output windows:
    the same rows. 257 is no multiple of 64 and smaller than the pairs of a few probe rows of
    a heavy key (about 20 build rows each)."""
    lparts, rparts, left, right, on = inputs("int64_utf8")
    opts = {"prefilter": {"prefilter": True}, "match_probe": {"match_probe": True},
            "max_output_rows": {"max_output_rows": 257}}[option]
    out = run_join(lparts, rparts, on, jt, right.schema, **opts)
    if option == "max_output_rows":
        assert out and max(b.num_rows for b in out) <= 257
    check(out, jt, left.schema, right.schema, expected("int64_utf8", jt))


def test_inputs_fan_out():
    """What the cases above rely on: heavy keys of about 20 build rows, about half the probe
    rows matched, more inner rows than either side has rows."""
    _, _, left, right, on = inputs("int64_utf8")
    semi = len(join_rows(left, right, on, "rightsemi"))
    assert 0.3 * NP < semi < 0.6 * NP
    per_key = {}
    for r in ref.table_rows(left.select([l for l, _ in on])):
        if None not in r:
            per_key[r] = per_key.get(r, 0) + 1
    assert 15 <= max(per_key.values()) <= 40
    assert len(expected("int64_utf8", "inner")) > NP


@pytest.mark.parametrize("jt", ["inner", "left", "right", "full", "rightanti"])
@pytest.mark.parametrize("kind", ["int32", "int64_utf8"])
@pytest.mark.parametrize("empty", ["build", "probe"])
def test_rows_one_side_empty(dfp, empty, kind, jt):
    """A side of zero rows in total (one empty batch, so its schema is known): the outer rows
    of the other side, nothing else."""
    left, right, on = ref.sides(kind, 70, 90, seed=7)
    if empty == "build":
        left = left.slice(5, 0)
    else:
        right = right.slice(5, 0)
    lt, rt = pa.Table.from_batches([left]), pa.Table.from_batches([right])
    want = canon(join_rows(lt, rt, on, jt))
    assert len(want) == {"inner": 0, "left": left.num_rows, "right": right.num_rows,
                         "full": left.num_rows + right.num_rows, "rightanti": right.num_rows}[jt]
    out = run_join([[left], []], [[right.slice(0, right.num_rows // 2)], [right.slice(right.num_rows // 2)]], on, jt,
                   right.schema)
    check(out, jt, left.schema, right.schema, want)
