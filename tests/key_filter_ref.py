"""numpy restatement of the two key-filter layouts, written from the text of include/hj.h
("key filter"): plan (the AUTO rule), add, test and select. Shared by the CPU and GPU
tests; no GPU and no library call in here."""
import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1


def mix64(x: np.ndarray) -> np.ndarray:
    """murmur3 fmix64 on uint64 arrays (mod 2^64)."""
    x = x.astype(U64, copy=True)
    x ^= x >> U64(33)
    x *= U64(0xff51afd7ed558ccd)
    x ^= x >> U64(33)
    x *= U64(0xc4ceb9fe1a85ec53)
    x ^= x >> U64(33)
    return x


def plan(kind: str, key_lo: int, key_hi: int, expected_keys: int) -> tuple[str, int]:
    """-> (kind with "auto" resolved, nwords); ValueError where the header says
    HJ_ERR_INVALID. Python integers: nothing overflows."""
    if kind not in ("auto", "range", "bloom") or expected_keys < 0:
        raise ValueError("bad arguments")
    values = key_hi - key_lo + 1
    range_words = -(-values // 64) if values > 0 else 0
    if kind == "auto":
        kind = ("range" if key_lo <= key_hi and values <= 64 * max(expected_keys, 1) and range_words < 2**32
                else "bloom")
    if kind == "range":
        if key_lo > key_hi:
            raise ValueError("a range filter needs key_lo <= key_hi")
        nwords = range_words
    else:
        nwords = max(1, -(-expected_keys // 4))
    if nwords >= 2**32:
        raise ValueError("2^32 words or more")
    return kind, nwords


class RefFilter:
    def __init__(self, kind: str, key_lo: int, key_hi: int, expected_keys: int):
        self.kind, self.nwords = plan(kind, key_lo, key_hi, expected_keys)
        self.key_lo, self.key_hi = key_lo, key_hi
        self.words = np.zeros(self.nwords, dtype=U64)
        self.dropped_adds = 0

    def _locate(self, keys: np.ndarray):
        """-> (in domain, word index, mask) per key, keys widened to int64 first."""
        k = np.asarray(keys).astype(np.int64).view(U64)
        with np.errstate(over="ignore"):
            if self.kind == "range":
                d = k - U64(self.key_lo & MASK64)  # unsigned wrap-around subtraction
                inside = d < U64(self.key_hi - self.key_lo + 1)
                return inside, np.where(inside, d >> U64(6), U64(0)), U64(1) << (d & U64(63))
            h = mix64(k)
            # ((h >> 32) * nwords) >> 32 with both factors below 2^32: exact in uint64
            word = ((h >> U64(32)) * U64(self.nwords)) >> U64(32)
            mask = np.zeros(len(k), dtype=U64)
            for j in range(4):
                mask |= U64(1) << ((h >> U64(6 * j)) & U64(63))
            return np.ones(len(k), dtype=bool), word, mask

    def add(self, keys, valid=None) -> None:
        keys = np.asarray(keys)
        ok = np.ones(len(keys), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        inside, word, mask = self._locate(keys)
        self.dropped_adds += int((ok & ~inside).sum())
        sel = ok & inside
        np.bitwise_or.at(self.words, word[sel].astype(np.int64), mask[sel])

    def present(self, keys, valid=None) -> np.ndarray:
        """bool per row: valid and present."""
        keys = np.asarray(keys)
        ok = np.ones(len(keys), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        inside, word, mask = self._locate(keys)
        hit = (self.words[word.astype(np.int64)] & mask) == mask if self.nwords else np.zeros(len(keys), bool)
        return ok & inside & hit

    def test(self, keys, valid=None) -> tuple[np.ndarray, int]:
        """-> (Arrow LSB bitmap of ceil(n / 64) * 8 bytes, count)."""
        p = self.present(keys, valid)
        bits = np.zeros((len(p) + 63) // 64 * 64, dtype=bool)
        bits[: len(p)] = p
        return np.packbits(bits, bitorder="little"), int(p.sum())

    def select(self, keys, valid=None, probe_base: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """-> (passing keys in the keys' dtype, uint32 ids probe_base + row), row order."""
        keys = np.asarray(keys)
        rows = np.flatnonzero(self.present(keys, valid))
        return keys[rows], (rows + probe_base).astype(np.uint32)


def pack_validity(valid: np.ndarray, offset: int) -> np.ndarray:
    """An Arrow LSB bitmap whose bit `offset` is row 0 (the bits before it are set, to show
    that they are not read as rows)."""
    bits = np.concatenate([np.ones(offset, dtype=bool), np.asarray(valid, dtype=bool)])
    return np.packbits(bits, bitorder="little")
