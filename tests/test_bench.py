"""bench.py's command line: a plain run prints the headline alone, `--dump-outputs DIR` writes what the last timed step
returned (C = A @ B) as .npy files, the same in every run with the same arguments, and equal to the oracle's product."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_bounds_and_row_sums(tmp_path, monkeypatch):
    """Host tensors: the row sample stays within its byte budget, row sums beyond the cap are sums of consecutive runs
    of rows, every file is float32 or float64, and ranks of a distributed run write names of their own."""
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 100 * (16 * 4 + 8))
    monkeypatch.setattr(bench, "DUMP_SUMS_MAX", 300)
    c = torch.rand((1001, 16), generator=torch.Generator().manual_seed(3))
    bench.dump_outputs(str(tmp_path), c, 0, 1)
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert set(got) == {"c_rows_sample", "c_sample_rows", "c_row_sums", "c_col_sums"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    rows = got["c_sample_rows"].astype(np.int64)
    assert got["c_rows_sample"].shape == (100, 16) and np.array_equal(got["c_rows_sample"], c.numpy()[rows])
    want = c.double().sum(1).numpy()
    want = np.concatenate([want, np.zeros(3)]).reshape(-1, 4).sum(1)      # ceil(1001 / 300) = 4 rows per sum
    assert np.allclose(got["c_row_sums"], want, rtol=1e-12)
    assert np.allclose(got["c_col_sums"], c.double().sum(0).numpy(), rtol=1e-12)
    bench.dump_outputs(str(tmp_path / "r1"), c, 1, 2)
    assert sorted(os.listdir(tmp_path / "r1")) == ["c_col_sums_rank1.npy", "c_row_sums_rank1.npy", "c_rows_sample_rank1.npy",
                                                   "c_sample_rows_rank1.npy"]
    assert np.load(tmp_path / "r1" / "c_rows_sample_rank1.npy").shape == (50, 16)


SMALL = ["--rows", "20000", "--cols", "2000", "--n", "128", "--density", "0.01"]


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *SMALL,
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_product_the_same_in_every_run(tmp_path, orc):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert "roofline" not in line and "cpu_baseline" not in line
    _plain_run(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["c_col_sums.npy", "c_row_sums.npy", "c_rows_sample.npy", "c_sample_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n

    # the same inputs as bench.py builds them, multiplied by the oracle
    import torch

    import bench

    M, K, N = 20000, 2000, 128
    data, idx, ptr = bench.make_csr_device(M, K, 0.01, seed=1234, device=torch.device("cuda", 0))
    b = torch.rand((K, N), generator=torch.Generator(device="cuda").manual_seed(99), device="cuda", dtype=torch.float32)
    h = [t.cpu().numpy() for t in (data, idx, ptr, b)]
    want = orc.dot_csr_ndarray((M, N), *h)
    rows = np.load(tmp_path / "a" / "c_sample_rows.npy").astype(np.int64)
    assert len(rows) == M           # 20000 rows x 128 columns fit the sample budget whole
    assert np.allclose(np.load(tmp_path / "a" / "c_rows_sample.npy"), want[rows], rtol=1e-5, atol=0)
    assert np.allclose(np.load(tmp_path / "a" / "c_row_sums.npy"), want.astype(np.float64).sum(1), rtol=1e-5, atol=0)
