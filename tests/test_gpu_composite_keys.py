"""GPU: what hj_composite_keys promises (include/hj.h), through the C ABI with hj_key_column
structs made by hand, so that pointers, offsets and alignment are the test's:

* equal tuples give equal keys, wherever the row stands, however the columns are sliced,
  whatever the offset width and whatever the alignment of a `values` pointer (the byte-wise
  branch of fixed_word in csrc/hj_keys.hip runs only for a misaligned pointer, which the
  Python wrappers never make);
* bit i of out_valid = no key column is null at row i, and the ceil(n / 64) words are written
  whole (one ballot word per 64 rows: zeros past n), nothing after them;
* distinct tuples get distinct keys on a set built from the near misses a weak combiner
  confuses. A join's pairs do not depend on the hash (hj_filter_equal_pairs re-checks), so
  nothing end to end would notice a hash that collides on them - only the candidates grow.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


def dev():
    return torch.device("cuda", 0)


def to_dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev())  # a copy: some inputs are read-only views of bytes


def bitmap_bytes(n: int) -> int:
    return ((n + 63) // 64) * 8


class Col:
    """A host key column: fixed width (`data` uint8 [n, width]) or variable width (`items`, a
    list of bytes), and a bool validity per row. device() lays it out in device memory as the
    caller says and returns the hj_key_column fields; the tensors stay alive in self.keep."""

    def __init__(self, valid: np.ndarray, data: np.ndarray | None = None, items: list | None = None):
        self.valid, self.data, self.items = np.asarray(valid, bool), data, items
        self.keep = []

    @property
    def n(self):
        return len(self.valid)

    def rows(self, order) -> "Col":
        order = np.asarray(order)
        return Col(self.valid[order], None if self.data is None else self.data[order],
                   None if self.items is None else [self.items[i] for i in order])

    def device(self, lead_rows: int = 0, voff: int | None = 0, misalign: int = 0, offset_bytes: int = 4):
        """lead_rows: rows of other data before row 0 in the buffers (a sliced column: values
        start lead_rows in, offsets do not start at 0); voff: bit offset of the validity
        bitmap, None = no bitmap (the column must have no null); misalign: bytes by which a
        fixed-width values pointer is off an aligned address."""
        from datafusion_parallelism_amd._lib import HjKeyColumn

        rng = np.random.default_rng(lead_rows + 7)
        vptr, vo = None, 0
        if voff is not None:
            bits = np.concatenate([rng.random(voff) < 0.5, self.valid])
            t = to_dev(np.packbits(bits, bitorder="little"))
            self.keep.append(t)
            vptr, vo = t.data_ptr(), voff
        else:
            assert self.valid.all()
        if self.data is not None:
            w = self.data.shape[1]
            lead = rng.integers(0, 256, (lead_rows, w), dtype=np.uint8)
            raw = np.concatenate([lead, self.data]).reshape(-1)
            buf = torch.zeros(raw.size + 16 + misalign, dtype=torch.uint8, device=dev())
            buf[misalign:misalign + raw.size] = to_dev(raw)
            self.keep.append(buf)
            assert buf.data_ptr() % 16 == 0
            return HjKeyColumn(buf.data_ptr() + misalign + lead_rows * w, None, vptr, vo, w, 0)
        lead = [bytes(rng.integers(0, 256, 3 + i, dtype=np.uint8)) for i in range(lead_rows)]
        lens = np.array([len(x) for x in lead + self.items], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64 if offset_bytes == 8 else np.int32)
        vals = np.frombuffer(b"".join(lead + self.items) + b"\xEE", dtype=np.uint8)
        d_offs, d_vals = to_dev(offs), to_dev(vals)
        self.keep += [d_offs, d_vals]
        return HjKeyColumn(d_vals.data_ptr(), d_offs.data_ptr() + lead_rows * offset_bytes, vptr, vo, 0, offset_bytes)


def key_array(structs):
    from datafusion_parallelism_amd._lib import HjKeyColumn

    arr = (HjKeyColumn * max(len(structs), 1))()
    for i, s in enumerate(structs):
        arr[i] = s
    return arr


def composite(structs, n: int, ncols: int | None = None):
    """Raw hj_composite_keys over pre-filled outputs: (status, keys int64 [n], bitmap bytes with
    the guard, the key buffer with its guard)."""
    from datafusion_parallelism_amd import _lib
    from datafusion_parallelism_amd.columns import _stream

    L = _lib.load()
    keys = torch.full((n + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev())
    valid = torch.full((bitmap_bytes(n) + GUARD,), 0xFF, dtype=torch.uint8, device=dev())
    valid[bitmap_bytes(n):] = FILL
    st = L.hj_composite_keys(len(structs) if ncols is None else ncols, key_array(structs), n, keys.data_ptr(),
                             valid.data_ptr(), _stream(dev()))
    torch.cuda.synchronize()
    return st, keys.cpu().numpy(), valid.cpu().numpy()


def keys_of(structs, n: int) -> np.ndarray:
    from datafusion_parallelism_amd._lib import HJ_OK

    st, keys, _ = composite(structs, n)
    assert st == HJ_OK
    assert (keys[n:] == 0x5A5A5A5A5A5A5A5A).all()
    return keys[:n]


# ---- validity --------------------------------------------------------------------------

def three_columns(rng, n: int, null_free: int | None) -> list[Col]:
    """An int32, a Utf8 and an int64 column of n rows, each about 15 % null except `null_free`."""
    def valid(j):
        return np.ones(n, bool) if j == null_free else rng.random(n) > 0.15
    return [Col(valid(0), data=rng.integers(0, 256, (n, 4), dtype=np.uint8)),
            Col(valid(1), items=[b"s%d" % (i % 11) for i in range(n)]),
            Col(valid(2), data=rng.integers(0, 256, (n, 8), dtype=np.uint8))]


VOFFS = [0, 5, 13, None]  # per-column validity: a bitmap from this bit, or NULL


@pytest.mark.parametrize("ncols", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_validity_is_the_and_of_the_columns(dfp, n, ncols):
    from datafusion_parallelism_amd._lib import HJ_OK

    rng = np.random.default_rng(100 * n + ncols)
    for rot in range(4):
        voffs = [VOFFS[(rot + j) % 4] for j in range(ncols)]
        null_free = voffs.index(None) if None in voffs else None
        cols = three_columns(rng, n, null_free)[:ncols]
        st, keys, valid = composite([c.device(voff=v) for c, v in zip(cols, voffs)], n)
        assert st == HJ_OK, voffs
        want = np.logical_and.reduce([c.valid for c in cols])
        nb = bitmap_bytes(n)
        bits = np.unpackbits(valid[:nb], bitorder="little").astype(bool)
        assert np.array_equal(bits[:n], want), voffs
        assert not bits[n:].any(), voffs            # the words are written whole: zeros past n
        assert (valid[nb:] == FILL).all(), voffs    # and nothing after them
        assert (keys[n:] == 0x5A5A5A5A5A5A5A5A).all(), voffs


def test_no_rows_writes_nothing(dfp):
    from datafusion_parallelism_amd._lib import HJ_OK

    cols = three_columns(np.random.default_rng(1), 4, None)
    st, keys, valid = composite([c.device() for c in cols], 0)
    assert st == HJ_OK
    assert (keys == 0x5A5A5A5A5A5A5A5A).all() and (valid == FILL).all()


# ---- position and layout independence ------------------------------------------------------

WIDTHS = [1, 2, 4, 8, 16]


@pytest.fixture(scope="module")
def tuples():
    """600 rows of: fixed columns of width 1, 2, 4, 8 and 16, a bool (one byte, 0 / 1), a
    float64 (signed zeros, NaNs), a Binary with zero bytes and empty values, a Utf8. Every
    tuple occurs a few times (rows drawn from 150 tuples), nulls in every column."""
    rng = np.random.default_rng(77)
    pick = rng.integers(0, 150, 600)
    fixed = [rng.integers(0, 256, (150, w), dtype=np.uint8)[pick] for w in WIDTHS]
    flag = rng.integers(0, 2, (150, 1), dtype=np.uint8)[pick]
    floats = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, 1.5] * 25)[pick].view(np.uint8).reshape(-1, 8)
    binary = [bytes(rng.integers(0, 2, i % 23, dtype=np.uint8)) for i in range(150)]
    text = [("k%d" % (i // 3) + "é" * (i % 3)).encode() for i in range(150)]
    valid = lambda: rng.random(600) > 0.08
    cols = [Col(valid(), data=d) for d in fixed] + [Col(valid(), data=flag), Col(valid(), data=floats),
                                                    Col(valid(), items=[binary[i] for i in pick]),
                                                    Col(valid(), items=[text[i] for i in pick])]
    return cols, pick


def test_equal_tuples_equal_keys_whatever_the_layout(dfp, tuples):
    cols, pick = tuples
    n = len(pick)
    base = keys_of([c.device() for c in cols], n)
    # rows of one tuple share a key; different tuples do not (150 tuples: no chance collision)
    first = {}
    for i, t in enumerate(pick):
        assert base[i] == base[first.setdefault(int(t), i)]
    assert len(set(base.tolist())) == len(first)
    # reverse row order
    reversed_cols = [c.rows(np.arange(n - 1, -1, -1)) for c in cols]  # named: they own their device buffers
    rev = keys_of([c.device() for c in reversed_cols], n)
    assert np.array_equal(rev[::-1], base)
    # every column sliced: values from a non-zero row, validity from a non-zero bit, offsets not from 0
    sliced = keys_of([c.device(lead_rows=3 + j, voff=(3, 5, 13)[j % 3]) for j, c in enumerate(cols)], n)
    assert np.array_equal(sliced, base)
    # the variable-width columns with 8-byte offsets (LargeBinary / LargeUtf8 of the same bytes)
    large = keys_of([c.device(offset_bytes=8) for c in cols], n)
    assert np.array_equal(large, base)
    # a shorter batch of the same rows: the key does not depend on n either
    head_cols = [c.rows(np.arange(65)) for c in cols]
    head = keys_of([c.device() for c in head_cols], 65)
    assert np.array_equal(head, base[:65])


@pytest.mark.parametrize("misalign", [1, 3, 7])
def test_equal_keys_from_misaligned_values(dfp, tuples, misalign):
    """Each fixed-width column of width 2, 4, 8 and 16 in turn - and all of them at once - at
    an address `misalign` bytes off: the same keys as from aligned buffers."""
    cols, pick = tuples
    n = len(pick)
    base = keys_of([c.device() for c in cols], n)
    wide = [j for j, c in enumerate(cols) if c.data is not None and c.data.shape[1] > 1]
    assert sorted({cols[j].data.shape[1] for j in wide}) == [2, 4, 8, 16]
    for chosen in [[j] for j in wide] + [wide]:
        structs = [c.device(misalign=misalign if j in chosen else 0) for j, c in enumerate(cols)]
        for j in chosen:
            assert structs[j].values % min(cols[j].data.shape[1], 8) != 0
        assert np.array_equal(keys_of(structs, n), base), chosen


def equal_pairs(bstructs, pstructs, b: np.ndarray, p: np.ndarray):
    """Raw hj_filter_equal_pairs: (status, kept build rows, kept probe rows)."""
    from datafusion_parallelism_amd import _lib
    from datafusion_parallelism_amd.columns import _stream

    L = _lib.load()
    n = len(b)
    d_b, d_p = to_dev(b.astype(np.int64)), to_dev(p.astype(np.int32))
    ob = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev())
    op = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev())
    cnt = torch.full((1,), -1, dtype=torch.int64, device=dev())
    ws = torch.full((L.hj_equal_pairs_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=dev())
    st = L.hj_filter_equal_pairs(len(bstructs), key_array(bstructs), key_array(pstructs), d_b.data_ptr(),
                                 d_p.data_ptr(), n, ob.data_ptr(), op.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                 _stream(dev()))
    torch.cuda.synchronize()
    m = int(cnt.item())
    return st, ob[:max(m, 0)].cpu().numpy(), op[:max(m, 0)].cpu().numpy()


def test_filter_equal_pairs_from_misaligned_values(dfp, tuples):
    """hj_filter_equal_pairs over the same columns, the build side's fixed-width values 3 bytes
    off and the probe side's 1 byte off or aligned: exactly the pairs of the numpy mask (the
    bytes of every column equal), in order."""
    from datafusion_parallelism_amd._lib import HJ_OK

    cols, pick = tuples
    n = len(pick)
    rng = np.random.default_rng(5)
    b = rng.integers(0, n, 5000)
    same = rng.random(5000) < 0.5
    # an equal pair: another row of the same tuple (or the row itself); else any row
    by_tuple = {}
    for i, t in enumerate(pick):
        by_tuple.setdefault(int(t), []).append(i)
    p = np.array([rng.choice(by_tuple[int(pick[i])]) if s else rng.integers(0, n) for i, s in zip(b, same)])
    mask = np.ones(5000, bool)
    for c in cols:
        if c.data is not None:
            mask &= (c.data[b] == c.data[p]).all(axis=1)
        else:
            mask &= np.array([c.items[i] == c.items[j] for i, j in zip(b, p)])
    assert np.array_equal(mask, pick[b] == pick[p]) and 0.4 < mask.mean() < 0.7
    bst = [c.device(misalign=3, lead_rows=2) for c in cols]
    for pmis in (1, 0):
        st, ob, op = equal_pairs(bst, [c.device(misalign=pmis) for c in cols], b, p)
        assert st == HJ_OK
        assert np.array_equal(ob, b[mask]) and np.array_equal(op, p[mask]), pmis


# ---- distinctness -------------------------------------------------------------------------

def near_miss_tuples() -> list[tuple]:
    """About 10^5 distinct tuples (Utf8 s1, Utf8 s2, int64 a, int64 b, 16-byte d) around the
    tuple (b"", b"", 0, 0, 0): families that differ from each other in one small way, then
    random tuples. An ideal 64-bit hash collides on 10^5 tuples with probability
    (10^5)^2 / 2^65 < 10^-9; the set is fixed by the seed."""
    rng = np.random.default_rng(2024)
    out = []
    add = lambda s1=b"", s2=b"", a=0, b=0, d=0: out.append((s1, s2, a, b, d))
    # the split of a concatenation, and a value moving from one column to the other
    for s1, s2 in ((b"ab", b"c"), (b"a", b"bc"), (b"abc", b""), (b"", b"abc"), (b"x", b""), (b"", b"x")):
        add(s1, s2)
    for k in range(1, 200):
        add(a=k, b=k + 1)
        add(a=k + 1, b=k)
        add(a=k)
        add(b=k)
        add(d=k)
        add(d=k << 64)              # the same 8 bytes in the other half
    # empty against zero bytes: equal words after zero padding, different lengths
    for k in range(0, 40):
        add(s1=b"\x00" * k)
        add(s2=b"\x00" * k, a=1)
    # strings that differ only in their last byte, at the lengths around the 8-byte words
    for ln in (7, 8, 9, 15, 16, 17):
        stem = bytes(rng.integers(1, 256, ln - 1, dtype=np.uint8))
        for last in range(256):
            add(s1=stem + bytes([last]), a=2)
            add(s2=stem + bytes([last]), a=2)
    # 16-byte values that differ only in the high half; int64 values that differ only in bit 63
    lo = int(rng.integers(0, 2**62))
    for k in range(1, 3000):
        add(d=lo | (k << 64), a=3)
        add(d=lo | (1 << (64 + k % 64)) | (k << 70), a=4)
    for x in rng.integers(0, 2**62, 3000):
        add(a=int(x), b=5)
        add(a=int(x) - 2**63, b=5)
        add(b=int(x), a=6)
        add(b=int(x) - 2**63, a=6)
    out = list(dict.fromkeys(out))
    words = [bytes(rng.integers(97, 100, int(k), dtype=np.uint8)) for k in rng.integers(0, 20, 4000)]
    while len(out) < 100_000:
        m = 100_000 - len(out)
        a, b = rng.integers(-2**63, 2**63, m), rng.integers(-4, 4, m)
        i1, i2 = rng.integers(0, len(words), m), rng.integers(0, len(words), m)
        hi = rng.integers(0, 2**62, m)
        out += [(words[i1[k]], words[i2[k]], int(a[k]), int(b[k]), (int(hi[k]) << 64) | (k % 3)) for k in range(m)]
        out = list(dict.fromkeys(out))
    return out


def int_bytes(vals, width: int) -> np.ndarray:
    return np.frombuffer(b"".join(int(v % (1 << (8 * width))).to_bytes(width, "little") for v in vals),
                         dtype=np.uint8).reshape(-1, width)


def test_distinct_tuples_distinct_keys(dfp):
    tup = near_miss_tuples()
    n = len(tup)
    assert n == 100_000 and len(set(tup)) == n
    ones = np.ones(n, bool)
    cols = [Col(ones, items=[t[0] for t in tup]), Col(ones, items=[t[1] for t in tup]),
            Col(ones, data=int_bytes([t[2] for t in tup], 8)), Col(ones, data=int_bytes([t[3] for t in tup], 8)),
            Col(ones, data=int_bytes([t[4] for t in tup], 16))]
    keys = keys_of([c.device(voff=None) for c in cols], n)
    uniq, first, counts = np.unique(keys, return_index=True, return_counts=True)
    clash = [(tup[i], [t for t, k in zip(tup, keys) if k == keys[i]][1]) for i in first[counts > 1][:5]]
    assert len(uniq) == n, f"{n - len(uniq)} tuples share a key, e.g. {clash}"


# ---- column-count limits ---------------------------------------------------------------

def test_sixteen_columns_join(dfp, oracle_mod):
    """ncols at its limit of 16: int8 columns of values 0..3 (2 bits each: the tuple packs into
    an int64 for the oracle), 300 build and 500 probe rows drawn from 120 tuples."""
    import pyarrow as pa
    from datafusion_parallelism_amd.columns import DeviceColumn, composite_keys, filter_equal_pairs

    rng = np.random.default_rng(16)
    pool = rng.integers(0, 4, (120, 16)).astype(np.int8)
    pool[1] = pool[0]
    pool[1, 15] ^= 1                 # two tuples that differ in the last column only
    pool[3] = pool[2]
    pool[3, 0] ^= 2                  # and in the first
    bsel, psel = rng.integers(0, 100, 300), rng.integers(0, 120, 500)
    bnull, pnull = rng.random((300, 16)) < 0.01, rng.random((500, 16)) < 0.01
    bt, pt = pool[bsel], pool[psel]
    pack = lambda t: (t.astype(np.int64) << (2 * np.arange(16))).sum(axis=1)
    assert len(set(pack(pool).tolist())) == len({tuple(r) for r in pool.tolist()})
    bcols = [DeviceColumn.from_arrow(pa.array(bt[:, j], pa.int8(), mask=bnull[:, j]), dev()) for j in range(16)]
    pcols = [DeviceColumn.from_arrow(pa.array(pt[:, j], pa.int8(), mask=pnull[:, j]), dev()) for j in range(16)]
    bk, bv = composite_keys(bcols)
    pk, pv = composite_keys(pcols)
    with dfp.HashTable(1, "int64", 0) as t:
        t.build(bk, bv)
        b, p = t.probe(pk, pv, device_output=True)
        b, p = filter_equal_pairs(bcols, pcols, b, p)
    ob, op = oracle_mod.inner_join(pack(bt), pack(pt), ~bnull.any(axis=1), ~pnull.any(axis=1))
    assert len(ob) > 500
    assert np.array_equal(p.cpu().numpy().view(np.uint32), op)
    assert np.array_equal(b.cpu().numpy().astype(np.uint64), ob)


def test_column_count_and_width_errors(dfp):
    from datafusion_parallelism_amd._lib import HJ_ERR_INVALID, HJ_OK

    rng = np.random.default_rng(3)
    n = 10
    cols = [Col(np.ones(n, bool), data=rng.integers(0, 256, (n, 1), dtype=np.uint8)) for _ in range(17)]
    structs = [c.device() for c in cols]
    for ncols in (0, 17, -1):
        st, keys, valid = composite(structs, n, ncols=ncols)
        assert st == HJ_ERR_INVALID, ncols
        assert (keys == 0x5A5A5A5A5A5A5A5A).all()   # an error writes nothing
    assert composite(structs[:16], n)[0] == HJ_OK
    # build and probe columns of different width
    four = Col(np.ones(n, bool), data=rng.integers(0, 256, (n, 4), dtype=np.uint8))
    eight = Col(np.ones(n, bool), data=rng.integers(0, 256, (n, 8), dtype=np.uint8))
    idx = np.arange(n)
    assert equal_pairs([four.device()], [eight.device()], idx, idx)[0] == HJ_ERR_INVALID
    st, ob, op = equal_pairs([four.device()], [four.device()], idx, idx[::-1].copy())
    assert st == HJ_OK and len(ob) == 0  # ten random 4-byte values: rows i and 9 - i differ
