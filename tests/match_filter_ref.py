"""numpy restatement of the filtered match probe's contract, written from the text of
include/hj.h ("Filtered match probe"): F = the inner pairs S of the probe that pass the pair
predicate (pair_filter_ref.pair_pass), and every output is the match probe's
(probe_match_ref.expected*) over F in place of S. Shared by the CPU and GPU tests; no GPU and
no library call in here."""
import numpy as np

import pair_filter_ref as pf
import probe_match_ref as pm


def filtered_pairs(ob, op, terms, build_cols, probe_cols, build_rows: int, probe_rows: int):
    """F: the pairs (ob = build ids, op = probe rows) of S that pass; order kept."""
    ob, op = np.asarray(ob).astype(np.uint64), np.asarray(op).astype(np.uint32)
    keep = pf.pair_pass(terms, build_cols, probe_cols, build_rows, probe_rows, ob, op)
    return ob[keep], op[keep]


def expected(ob, op, n: int, nflags: int, terms, build_cols, probe_cols, build_rows: int, probe_rows: int | None = None,
             before=None) -> dict:
    """bitmap / counts / flags / matched / pairs over F, candidates = |S|. The -1 rules of
    d_stats are stats()'s."""
    probe_rows = n if probe_rows is None else probe_rows
    assert probe_rows >= n, "pred->probe_rows < n is HJ_ERR_INVALID"
    fb, fp = filtered_pairs(ob, op, terms, build_cols, probe_cols, build_rows, probe_rows)
    e = pm.expected(fb, fp, n, nflags, before)
    e["candidates"] = int(len(np.asarray(op)))
    return e


def stats(e: dict, bitmap: bool, counts: bool) -> list[int]:
    """d_stats as the call leaves it: [0] = rows with a pair in F if a bitmap or counts were
    asked for, else -1; [1] = |F| if counts were asked for, else -1; [2] = |S|."""
    return [e["matched"] if (bitmap or counts) else -1, e["pairs"] if counts else -1, e["candidates"]]
