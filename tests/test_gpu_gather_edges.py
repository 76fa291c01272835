"""GPU: hj_gather_fixed / hj_gather_var through the C ABI at the sizes where a wave's validity
word, the block, the scan segment of the offsets (kScanSeg = 4096) and the grid change, and
the DeviceColumn round trips (from_arrow / concat / to_arrow) on sliced arrays.

The gathers are raw calls over outputs pre-filled with a pattern and followed by guard bytes;
the expectation is numpy fancy indexing over host copies of the same buffers, so no object is
shared with the code under test. What include/hj.h promises and is checked here: dst[i] =
src[idx[i]] at valid rows, bit i of dst_valid = index not null and source row valid, nothing
written past n * width, ceil(n / 64) * 8 bitmap bytes, the n + 1 offsets; for hj_gather_var
also *d_values_len = bytes needed whatever values_cap is, and no byte written at or beyond
values_cap."""
import numpy as np
import pyarrow as pa
import pytest
import torch

from test_gpu_join_types import COLUMNS

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
GUARD, FILL = 64, 0xA5
NSRC = 301
VALIDITY = [None, 0, 3, 13]  # source validity: NULL, or a bitmap from this bit offset


def dev():
    return torch.device("cuda", 0)


def to_dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def filled(nbytes: int, value: int = FILL) -> torch.Tensor:
    return torch.full((nbytes,), value, dtype=torch.uint8, device=dev())


def bitmap_bytes(n: int) -> int:
    return ((n + 63) // 64) * 8


def make_indices(rng, n: int, nsrc: int, idx_bytes: int, force_null_ends: bool):
    """(source rows, null mask, device index tensor): about 10 % null indices (all-ones);
    source rows 0 and nsrc - 1 are used; with force_null_ends positions 0 and n - 1 are null."""
    rows = rng.integers(0, nsrc, n)
    null = rng.random(n) < 0.10
    if n >= 4:
        rows[1], rows[2] = 0, nsrc - 1
        null[1] = null[2] = False
    if force_null_ends and n:
        null[0] = null[n - 1] = True
    elif n:
        null[0] = null[n - 1] = False
    host = np.where(null, -1, rows).astype(np.int64 if idx_bytes == 8 else np.int32)
    return rows, null, to_dev(host)


def make_validity(rng, nsrc: int, voff):
    """(bool per source row, device bitmap or None)."""
    if voff is None:
        return np.ones(nsrc, bool), None
    bits = rng.random(voff + nsrc) < 0.8
    bits[voff], bits[voff + nsrc - 1] = True, False
    return bits[voff:], to_dev(np.packbits(bits, bitorder="little"))


def unpack(bitmap: torch.Tensor, n: int) -> np.ndarray:
    return np.unpackbits(bitmap.cpu().numpy(), bitorder="little")[:n].astype(bool)


def ptr(t):
    return None if t is None else t.data_ptr()


def end_variants(n: int):
    # positions 0 and n - 1 are null indices; where that leaves (almost) no row, the other way too
    return [True] if n >= 3 else [True, False]


@pytest.mark.parametrize("idx_bytes", [4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_gather_fixed_edges(dfp, n, idx_bytes):
    from datafusion_parallelism_amd import _lib
    from datafusion_parallelism_amd.columns import _stream, check

    L = _lib.load()
    rng = np.random.default_rng(10 * n + idx_bytes)
    for width in (1, 2, 4, 8, 16):
        src = rng.integers(0, 256, (NSRC, width), dtype=np.uint8)
        d_src = to_dev(src)
        for voff in VALIDITY:
            for ends in end_variants(n):
                svalid, d_svalid = make_validity(rng, NSRC, voff)
                rows, null, d_idx = make_indices(rng, n, NSRC, idx_bytes, ends)
                want_valid = ~null & svalid[rows]
                for with_valid in (True, False):
                    dst = filled(n * width + GUARD)
                    dvalid = filled(bitmap_bytes(n) + GUARD) if with_valid else None
                    check(L.hj_gather_fixed(d_src.data_ptr(), ptr(d_svalid), voff or 0, width, d_idx.data_ptr() if n
                                            else None, idx_bytes, n, dst.data_ptr(), ptr(dvalid), _stream(dev())))
                    got = dst.cpu().numpy()
                    where = (width, voff, ends, with_valid)
                    assert (got[n * width:] == FILL).all(), where
                    # null slots are unspecified (Arrow): compare the valid rows
                    assert np.array_equal(got[:n * width].reshape(n, width)[want_valid], src[rows[want_valid]]), where
                    if with_valid:
                        assert np.array_equal(unpack(dvalid, n), want_valid), where
                        assert (dvalid.cpu().numpy()[bitmap_bytes(n):] == FILL).all(), where


# source strings: the lengths where a row's byte copy ends its first 64-lane pass, takes a second, a third
VAR_LENS = [0, 1, 63, 64, 65, 129, 300]
VAR_NSRC = 71


def make_var_source(rng, nsrc: int, lens, offset_bytes: int):
    """(list of bytes per row, device offsets, device values): the offsets are a slice of a
    longer array, so the first one is not 0."""
    ln = np.array([lens[i % len(lens)] for i in range(nsrc)])
    # three rows (24 bytes) before the slice
    offs = np.concatenate([[0, 5, 11], 24 + np.concatenate([[0], np.cumsum(ln)])]).astype(np.int64)
    values = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    odt = np.int64 if offset_bytes == 8 else np.int32
    d_all = to_dev(offs.astype(odt))
    d_offs = d_all[3:]  # a view: the pointer moves, first offset 24
    assert int(d_offs[0]) == 24
    strs = [values[offs[3 + i]:offs[4 + i]].tobytes() for i in range(nsrc)]
    return strs, ln, offs[3:], d_all, d_offs, values, to_dev(values)


def var_expected(strs, rows, want_valid):
    out_lens = np.array([len(strs[r]) if v else 0 for r, v in zip(rows, want_valid)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64)
    vals = np.frombuffer(b"".join(strs[r] for r, v in zip(rows, want_valid) if v), dtype=np.uint8)
    return offs, vals


def run_gather_var(L, d_offs, offset_bytes, d_values, d_svalid, voff, d_idx, idx_bytes, n, cap):
    """One raw call over pre-filled outputs; returns (offsets bytes, values bytes, bitmap bytes,
    d_values_len) as host arrays."""
    from datafusion_parallelism_amd.columns import _stream, check

    out_off = filled((n + 1) * offset_bytes + GUARD)
    out_val = filled(cap + GUARD)
    dvalid = filled(bitmap_bytes(n) + GUARD)
    d_len = torch.full((1,), -1, dtype=torch.int64, device=dev())
    ws = filled(L.hj_gather_var_workspace_bytes(n), 0xFF)
    check(L.hj_gather_var(d_offs.data_ptr(), offset_bytes, d_values.data_ptr(), ptr(d_svalid), voff or 0,
                          d_idx.data_ptr() if n else None, idx_bytes, n, out_off.data_ptr(), out_val.data_ptr(), cap,
                          dvalid.data_ptr(), d_len.data_ptr(), ws.data_ptr(), _stream(dev())))
    return out_off.cpu().numpy(), out_val.cpu().numpy(), dvalid.cpu().numpy(), int(d_len.item())


def check_gather_var(res, n, offset_bytes, cap, want_offs, want_vals, want_valid, where):
    off_b, val_b, valid_b, d_len = res
    need = int(want_offs[-1])
    assert d_len == need, where
    got_offs = off_b[:(n + 1) * offset_bytes].view(np.int64 if offset_bytes == 8 else np.int32)
    assert np.array_equal(got_offs, want_offs), where
    assert (off_b[(n + 1) * offset_bytes:] == FILL).all(), where
    assert np.array_equal(np.unpackbits(valid_b[:bitmap_bytes(n)], bitorder="little")[:n].astype(bool), want_valid), where
    assert (valid_b[bitmap_bytes(n):] == FILL).all(), where
    # no byte at or beyond values_cap is written: the guard starts exactly at the cap
    assert (val_b[cap:] == FILL).all(), where
    # every row that ends at or before the cap holds its bytes (all of them when cap == need)
    fit = int(np.searchsorted(want_offs, cap, side="right")) - 1  # rows [0, fit) end at or before cap
    end = int(want_offs[fit])
    assert np.array_equal(val_b[:end], want_vals[:end]), where
    if cap >= need:
        assert fit == n and end == need, where


@pytest.mark.parametrize("idx_bytes", [4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_gather_var_edges(dfp, n, idx_bytes):
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(20 * n + idx_bytes)
    for offset_bytes in (4, 8):
        strs, _, _, _keep, d_offs, _, d_values = make_var_source(rng, VAR_NSRC, VAR_LENS, offset_bytes)
        for voff in VALIDITY:
            for ends in end_variants(n):
                svalid, d_svalid = make_validity(rng, VAR_NSRC, voff)
                rows, null, d_idx = make_indices(rng, n, VAR_NSRC, idx_bytes, ends)
                want_valid = ~null & svalid[rows]
                want_offs, want_vals = var_expected(strs, rows, want_valid)
                need = int(want_offs[-1])
                for cap in sorted({need, max(need - 1, 0), need // 2, 0}, reverse=True):
                    res = run_gather_var(L, d_offs, offset_bytes, d_values, d_svalid, voff, d_idx, idx_bytes, n, cap)
                    check_gather_var(res, n, offset_bytes, cap, want_offs, want_vals, want_valid,
                                     (offset_bytes, voff, ends, cap, need))


# The launchers' grid caps (csrc/hj_columns.hip): `grid` of launch_gather_fixed and of
# launch_gather_var (gather_var_len_kernel) is at most 16384 blocks of 256 rows, `cgrid` of
# launch_gather_var (gather_var_copy_kernel) at most 8192 blocks of 4 waves x 64 rows. One wave's
# word past each cap makes the grid-stride loops take a second turn; the sizes follow these two.
FIXED_GRID_ROWS = 16384 * 256
VAR_COPY_GRID_ROWS = 8192 * 256


@pytest.mark.parametrize("width", [1, 16])
def test_gather_fixed_past_the_grid(dfp, width):
    from datafusion_parallelism_amd import _lib
    from datafusion_parallelism_amd.columns import _stream, check

    L = _lib.load()
    n = FIXED_GRID_ROWS + 65
    rng = np.random.default_rng(width)
    nsrc = 5003
    src = rng.integers(0, 256, (nsrc, width), dtype=np.uint8)
    svalid, d_svalid = make_validity(rng, nsrc, 3)
    rows, null, d_idx = make_indices(rng, n, nsrc, 4, True)
    want_valid = ~null & svalid[rows]
    d_src = to_dev(src)
    dst = filled(n * width + GUARD)
    dvalid = filled(bitmap_bytes(n) + GUARD)
    check(L.hj_gather_fixed(d_src.data_ptr(), d_svalid.data_ptr(), 3, width, d_idx.data_ptr(), 4, n, dst.data_ptr(),
                            dvalid.data_ptr(), _stream(dev())))
    got = dst.cpu().numpy()
    assert (got[n * width:] == FILL).all()
    assert np.array_equal(unpack(dvalid, n), want_valid)
    assert (dvalid.cpu().numpy()[bitmap_bytes(n):] == FILL).all()
    want = np.where(want_valid[:, None], src[rows], 0)
    assert np.array_equal(np.where(want_valid[:, None], got[:n * width].reshape(n, width), 0), want)


@pytest.mark.parametrize("n", [VAR_COPY_GRID_ROWS + 65, FIXED_GRID_ROWS + 65])
def test_gather_var_past_the_grid(dfp, n):
    """Strings of 0 to 3 bytes: past the copy kernel's grid, and past the length kernel's."""
    from datafusion_parallelism_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(n)
    nsrc = 1001
    strs, ln, offs, _keep, d_offs, values, d_values = make_var_source(rng, nsrc, [0, 1, 2, 3, 3, 1], 4)
    svalid, d_svalid = make_validity(rng, nsrc, 13)
    rows, null, d_idx = make_indices(rng, n, nsrc, 4, True)
    want_valid = ~null & svalid[rows]
    out_lens = np.where(want_valid, ln[rows], 0).astype(np.int64)
    want_offs = np.concatenate([[0], np.cumsum(out_lens)])
    need = int(want_offs[-1])
    # byte k of output row i is values[offs[rows[i]] + k]
    src_pos = np.repeat(offs[rows] - want_offs[:-1], out_lens) + np.arange(need)
    want_vals = values[src_pos]
    res = run_gather_var(L, d_offs, 4, d_values, d_svalid, 13, d_idx, 4, n, need)
    check_gather_var(res, n, 4, need, want_offs, want_vals, want_valid, n)
    # and the same through pyarrow's take of the same column, for a sample of the rows
    arr = pa.Array.from_buffers(pa.binary(), nsrc, [pa.py_buffer(np.packbits(svalid, bitorder="little").tobytes()),
                                                    pa.py_buffer(offs.astype(np.int32).tobytes()),
                                                    pa.py_buffer(values.tobytes())])
    sample = np.concatenate([np.arange(0, 300), np.arange(n - 300, n)])
    taken = arr.take(pa.array(rows[sample], mask=null[sample])).to_pylist()
    got_offs = res[0][:(n + 1) * 4].view(np.int32)
    for i, t in zip(sample, taken):
        mine = res[1][got_offs[i]:got_offs[i + 1]].tobytes()
        assert (t is None) == (not want_valid[i]) and (t is None or t == mine), i


# ---- DeviceColumn round trips ---------------------------------------------------------

def pieces_of(arr: pa.Array, k: int) -> list[pa.Array]:
    """k slices at odd offsets that cover arr[3:], an empty piece among them from k = 2 on and
    an all-null piece (a bitmap of zeros from a non-zero bit) from k = 5 on."""
    n = len(arr)
    if k == 1:
        return [arr.slice(13, n - 20)]
    if k == 2:
        return [arr.slice(3, 0), arr.slice(3)]
    nulls = pa.array([None] * 29, arr.type).slice(5, 17)
    return [arr.slice(3, 18), arr.slice(21, 0), nulls, arr.slice(21, n // 2 - 21), arr.slice(n // 2)]


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_concat_matches_arrow(dfp, name, k):
    """DeviceColumn.concat of sliced pieces equals pa.concat_arrays, and is re-based as its
    docstring says: the bitmap starts at bit 0 and the offsets at 0 - a single piece whose
    bitmap starts elsewhere included (the early return is for voff == 0 only)."""
    from datafusion_parallelism_amd.columns import DeviceColumn

    pieces = pieces_of(COLUMNS[name], k)
    cols = [DeviceColumn.from_arrow(p, "cuda:0") for p in pieces]
    if k == 1 and pieces[0].null_count:
        assert cols[0].voff == 13
    if k == 5:
        assert cols[2].valid is not None and cols[2].voff == 5
    got = DeviceColumn.concat(cols)
    want = pa.concat_arrays(pieces)
    assert got.length == len(want) and got.type == want.type
    assert got.voff == 0
    if got.offsets is not None and got is not cols[0]:  # one piece with a bitmap from bit 0 is returned as it is
        assert int(got.offsets[0]) == 0
    assert got.to_arrow().equals(want)
    if got.valid is not None:
        want_bits = np.asarray(want.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        assert np.array_equal(got.valid_bools().cpu().numpy(), want_bits)
    # the concatenated column is what the joins gather from
    idx = torch.arange(len(want) - 1, -1, -1, dtype=torch.int64, device="cuda:0")
    assert got.take(idx).to_arrow().equals(want.take(pa.array(np.arange(len(want) - 1, -1, -1))))


def test_concat_mixes_null_free_and_null_bearing(dfp):
    """valid is None next to bitmaps: the null-free pieces' rows are all valid."""
    from datafusion_parallelism_amd.columns import DeviceColumn

    a = pa.array(["x", "yy", "zzz"] * 30, pa.string()).slice(7, 70)
    b = pa.array([None, "q", None, "rs"] * 20, pa.string()).slice(5, 61)
    cols = [DeviceColumn.from_arrow(p, "cuda:0") for p in (a, b, a, b)]
    assert cols[0].valid is None and cols[1].valid is not None and cols[1].voff == 5
    got = DeviceColumn.concat(cols)
    assert got.voff == 0 and got.to_arrow().equals(pa.concat_arrays([a, b, a, b]))
    # all pieces null-free: no bitmap at all
    assert DeviceColumn.concat([cols[0], cols[2]]).valid is None


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_from_arrow_round_trip_sliced(dfp, name):
    from datafusion_parallelism_amd.columns import DeviceColumn

    arr = COLUMNS[name]
    for off, ln in ((0, len(arr)), (1, 63), (3, 64), (13, 65), (13, len(arr) - 20), (len(arr) - 1, 1), (37, 0)):
        piece = arr.slice(off, ln)
        assert DeviceColumn.from_arrow(piece, "cuda:0").to_arrow().equals(piece), (name, off, ln)
