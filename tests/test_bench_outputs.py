"""bench.py's plain run and --dump-outputs (CPU: bench.run with the oracle as the engine, tests/test_distributed.py).

A plain run carries no CPU baseline (--full asks for it); --dump-outputs writes the last timed step's arrays, equal
from run to run and equal to a direct solve of that step's problem ids."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from test_distributed import OracleEngine  # noqa: E402

B, STEPS, WARMUP = 3, 2, 1


def _run(tmp_path, workload, name):
    d = str(tmp_path / name)
    argv = ["--gpus", "1", "--nq", "2", "--batch", str(B), "--steps", str(STEPS), "--warmup", str(WARMUP),
            "--workload", workload, "--dump-outputs", d]
    line = bench.run(bench.parse(argv), engine_factory=OracleEngine)
    return line, {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("workload", ["dg-loop", "first-solve"])
def test_dump_outputs_is_the_last_timed_step(tmp_path, workload):
    from vboc_amd.dist import shard_ids
    line, a = _run(tmp_path, workload, "a")
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    assert all(v.dtype == np.float64 for v in a.values())
    eng = OracleEngine(2, None, 0)
    ids = shard_ids(WARMUP + STEPS - 1, 1, 0, B)
    if workload == "dg-loop":
        assert sorted(a) == ["X_save", "problems", "row_cnt"]
        out = eng.dg(ids)
        X = bench.order_rows(out).numpy()
        np.testing.assert_array_equal(a["X_save"], X)
        np.testing.assert_array_equal(a["row_cnt"], out["row_cnt"].numpy())
        np.testing.assert_array_equal(a["problems"], np.arange(B))
    else:
        assert sorted(a) == ["qp_iter", "sqp_iter", "status", "x0"]
        out = eng.first_solve(eng.first_solve_batch(2, ids))
        np.testing.assert_array_equal(a["x0"], out["x0"].numpy())
        np.testing.assert_array_equal(a["status"], out["status"].numpy())
    _, b = _run(tmp_path, workload, "b")
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_dump_outputs_over_the_byte_bound_keeps_whole_problems(tmp_path, monkeypatch):
    """Past DUMP_BYTES the dump holds a subset of the problems fixed by their number alone, each with all its rows."""
    import torch
    cnt = np.array([2, -1, 0, 3, 1, 4], dtype=np.int32)
    n = np.maximum(cnt, 0)
    X = np.arange(int(n.sum()) * 4, dtype=np.float64).reshape(-1, 4)
    assert X.nbytes < bench.DUMP_BYTES
    last = dict(X_save=torch.as_tensor(X), row_cnt=torch.as_tensor(cnt))
    bench.dump_outputs(str(tmp_path / "all"), last)
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "X_save.npy"), X)
    # force the sampled branch: a bound below the array's size, sized for two problems
    monkeypatch.setattr(bench, "DG_ROWS_MAX", 2)
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 2 * 4 * 8)
    bench.dump_outputs(str(tmp_path / "some"), last)
    keep = np.load(tmp_path / "some" / "problems.npy").astype(int)
    assert len(keep) == 2 and np.all(np.diff(keep) > 0)
    np.testing.assert_array_equal(keep, np.sort(np.random.default_rng(0).permutation(len(cnt))[:2]))
    start = np.cumsum(n) - n
    want = np.concatenate([X[start[p]:start[p] + n[p]] for p in keep])
    np.testing.assert_array_equal(np.load(tmp_path / "some" / "X_save.npy"), want)
    np.testing.assert_array_equal(np.load(tmp_path / "some" / "row_cnt.npy"), cnt)
