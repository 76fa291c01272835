"""`bench.py --dump-outputs DIR` writes what the timed path computed in its last step as
float64 .npy files, identical from run to run; `--full` is where everything past the
headline figure lives. CPU: the dry-run skeleton. GPU: the single-GPU job's dumped pairs
against the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dry_run_dumps_the_same_outputs_twice(tmp_path):
    dumps = []
    for name in ("a", "b"):
        d = _bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--dump-outputs",
                   str(tmp_path / name))
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["hit.npy", "matches.npy"]
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    for f, a in dumps[0].items():
        assert a.dtype == np.float64
        assert np.array_equal(a, dumps[1][f]), f
    assert dumps[0]["matches.npy"][0] == dumps[0]["hit.npy"].sum() > 0
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20


def test_full_is_an_option():
    d = _bench("--gpus", "1", "--dry-run", "--steps", "1", "--warmup", "0", "--full")
    assert d["steps"] == 1 and d["ms_per_step"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [1000, 1 << 21], ids=["sampled", "whole"])
def test_dumped_pairs_match_the_oracle(dfp, oracle_mod, tmp_path, monkeypatch, sample):
    """The single-GPU job's last step, dumped: every pair (or the seeded sample of them) and
    the checksums over all pairs equal the oracle's join of the same keys."""
    import torch

    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    rng = np.random.default_rng(11)
    bk = rng.permutation(20001).astype(np.int64)  # unique, as the benchmark's: at most one pair per probe row
    pk = rng.integers(0, 40000, 70001).astype(np.int64)  # above the sliced probe's 65536-row threshold
    ob, op = oracle_mod.inner_join(bk, pk)
    ob, op = ob.astype(np.int64), op.astype(np.int64)
    assert 1000 < len(ob) < len(pk)
    dev = torch.device("cuda", 0)
    job = bench.SingleGpuJoin(torch.from_numpy(bk).to(dev), torch.from_numpy(pk).to(dev), dev)
    for _ in range(2):
        job.step()
    torch.cuda.synchronize(dev)
    job.finish()
    assert job.matches == len(ob)
    bench.dump_pairs(str(tmp_path), *job.outputs())
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["build_row_idx", "checksums", "probe_row_idx", "sample_positions"]
    assert all(a.dtype == np.float64 for a in got.values())
    pos = got["sample_positions"].astype(np.int64)
    if sample < len(ob):
        assert len(pos) == sample and np.all(np.diff(pos) >= 0) and pos[0] >= 0 and pos[-1] < len(ob)
        assert np.array_equal(pos, np.sort(np.random.default_rng(0xD0).integers(0, len(ob), sample)))
    else:
        assert np.array_equal(pos, np.arange(len(ob)))
    assert np.array_equal(got["build_row_idx"], ob[pos].astype(np.float64))
    assert np.array_equal(got["probe_row_idx"], op[pos].astype(np.float64))
    weighted = int(((ob + op) * (np.arange(len(ob), dtype=np.int64) % 1021 + 1)).sum()) & ((1 << 52) - 1)
    assert got["checksums"].tolist() == [len(ob), ob.sum(), op.sum(), weighted]
