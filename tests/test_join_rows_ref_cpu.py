"""CPU: the row model of tests/join_rows_ref.py is itself tested before the GPU tests lean on
it - against Acero (pyarrow.Table.join, an independent hash join) on the key kinds whose
equality both define alike, and against rows written out by hand for the float keys where
the project's rule (equal bits) is its own."""
import pyarrow as pa
import pytest

import join_rows_ref as ref
from join_rows_ref import NAN_A, NAN_B, canon, join_rows

ACERO = {"inner": "inner", "left": "left outer", "right": "right outer", "full": "full outer",
         "leftsemi": "left semi", "leftanti": "left anti", "rightsemi": "right semi", "rightanti": "right anti"}
KINDS = ["int32", "utf8", "int64_large_utf8", "date32_bool_int16", "decimal128"]


@pytest.fixture(scope="module", params=KINDS)
def tables(request):
    """350 build and 450 probe rows: nulls in keys and payloads, keys repeated on both sides."""
    left, right, on = ref.sides(request.param, 350, 450, seed=KINDS.index(request.param) + 1)
    return pa.Table.from_batches([left]), pa.Table.from_batches([right]), on


@pytest.mark.parametrize("jt", ref.JOIN_TYPES)
def test_model_matches_acero(tables, jt):
    left, right, on = tables
    want = left.join(right, keys=[l for l, _ in on], right_keys=[r for _, r in on], join_type=ACERO[jt],
                     coalesce_keys=False)
    names = {"leftsemi": left.column_names, "leftanti": left.column_names, "rightsemi": right.column_names,
             "rightanti": right.column_names}.get(jt, left.column_names + right.column_names)
    assert sorted(want.column_names) == sorted(names)
    got = join_rows(left, right, on, jt)
    assert canon(got) == canon(ref.table_rows(want.select(names)))
    assert all(len(r) == len(names) for r in got)


def test_inputs_have_what_the_tests_need(tables):
    """Duplicated keys on both sides, null keys and null payloads, matches and misses."""
    left, right, on = tables
    for t, k in ((left, on[0][0]), (right, on[0][1])):
        vals = [v for v in t.column(k).to_pylist() if v is not None]
        assert len(set(vals)) < len(vals) and t.column(k).null_count > 0
        assert t.column(t.column_names[-1]).null_count == t.num_rows            # the all-null payload
        assert t.column(t.column_names[-2]).null_count == 0                     # the null-free payload
        assert all(t.column(c).null_count > 0 for c in t.column_names[len(on):-2])
    assert 0 < len(join_rows(left, right, on, "rightsemi")) < right.num_rows
    assert 0 < len(join_rows(left, right, on, "leftanti")) < left.num_rows


def _ft(keys, tags, prefix):
    return pa.table({prefix + "k": pa.array(keys, pa.float64()), prefix + "v": pa.array(tags, pa.string())})


ON = [("l_k", "r_k")]


def test_float_keys_signed_zero():
    """0.0 and -0.0 are different keys: they differ in the sign bit."""
    left = _ft([0.0, -0.0, 1.5], ["l+0", "l-0", "l1.5"], "l_")
    right = _ft([-0.0, 0.0, 0.0], ["r-0", "r+0a", "r+0b"], "r_")
    assert canon(join_rows(left, right, ON, "inner")) == canon([
        (0.0, "l+0", 0.0, "r+0a"), (0.0, "l+0", 0.0, "r+0b"), (-0.0, "l-0", -0.0, "r-0")])
    assert canon(join_rows(left, right, ON, "leftanti")) == canon([(1.5, "l1.5")])
    assert join_rows(left, right, ON, "rightanti") == []


def test_float_keys_nan_by_bits():
    """A NaN key matches the NaN of the same bits and no other."""
    left = _ft([NAN_A, NAN_B, 2.0], ["lA", "lB", "l2"], "l_")
    right = _ft([NAN_A, NAN_A, 3.0], ["rA1", "rA2", "r3"], "r_")
    assert canon(join_rows(left, right, ON, "inner")) == canon([(NAN_A, "lA", NAN_A, "rA1"), (NAN_A, "lA", NAN_A, "rA2")])
    assert canon(join_rows(left, right, ON, "leftsemi")) == canon([(NAN_A, "lA")])
    assert canon(join_rows(left, right, ON, "leftanti")) == canon([(NAN_B, "lB"), (2.0, "l2")])
    assert canon(join_rows(left, right, ON, "rightanti")) == canon([(3.0, "r3")])
    # canon tells the two NaNs and the two zeros apart
    assert canon([(NAN_A,)]) != canon([(NAN_B,)]) and canon([(0.0,)]) != canon([(-0.0,)])


def test_float_keys_full_join_with_nulls():
    """Null keys match nothing, not even each other; every row of both sides appears."""
    left = _ft([None, -0.0, NAN_B, 7.0], ["lnull", "l-0", "lB", "l7"], "l_")
    right = _ft([None, 0.0, NAN_B, 7.0, 7.0], ["rnull", "r+0", "rB", "r7a", "r7b"], "r_")
    assert canon(join_rows(left, right, ON, "full")) == canon([
        (NAN_B, "lB", NAN_B, "rB"), (7.0, "l7", 7.0, "r7a"), (7.0, "l7", 7.0, "r7b"),
        (None, "lnull", None, None), (-0.0, "l-0", None, None),
        (None, None, None, "rnull"), (None, None, 0.0, "r+0")])
    assert canon(join_rows(left, right, ON, "left")) == canon([
        (NAN_B, "lB", NAN_B, "rB"), (7.0, "l7", 7.0, "r7a"), (7.0, "l7", 7.0, "r7b"),
        (None, "lnull", None, None), (-0.0, "l-0", None, None)])
    assert canon(join_rows(left, right, ON, "rightsemi")) == canon([(NAN_B, "rB"), (7.0, "r7a"), (7.0, "r7b")])
