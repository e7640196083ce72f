"""bench.py --dump-outputs on the host: dump_outputs writes float64 .npy files, whole while they
fit its budget, and beyond it a fixed, seeded sample of the rows of the large arrays."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_whole_within_budget(tmp_path):
    B = torch.arange(3000 * 7, dtype=torch.float64).reshape(3000, 7)
    bench.dump_outputs(str(tmp_path / "d"), {"B": B, "loglik": -1.25, "beta": np.array([1.0, -0.5]),
                                             "i": torch.arange(5, dtype=torch.int32)}, "_rank1")
    assert sorted(os.listdir(tmp_path / "d")) == ["B_rank1.npy", "beta_rank1.npy", "i_rank1.npy", "loglik_rank1.npy"]
    got = {f: np.load(tmp_path / "d" / f, allow_pickle=False) for f in os.listdir(tmp_path / "d")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["B_rank1.npy"], B.numpy()) and float(got["loglik_rank1.npy"]) == -1.25
    assert got["beta_rank1.npy"].tolist() == [1.0, -0.5] and got["i_rank1.npy"].tolist() == [0, 1, 2, 3, 4]


def test_dump_outputs_samples_rows_beyond_budget(tmp_path):
    n, m = 500_001, 15  # B alone is 60 MB: over the budget; F (4 MB) fits its share and stays whole
    B = torch.arange(n, dtype=torch.float64)[:, None] + torch.arange(m, dtype=torch.float64) / 16
    F = torch.arange(n, dtype=torch.float64) + 0.5
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), {"B": B, "F": F, "partials": torch.ones(4, dtype=torch.float64)})
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == ["B.npy", "B_rows.npy", "F.npy", "partials.npy"]
    a = {f: np.load(tmp_path / "0" / f, allow_pickle=False) for f in files}
    assert all(x.dtype == np.float64 for x in a.values())
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= bench.DUMP_BUDGET + 4 * 128 < 64 * 10 ** 6
    rows = a["B_rows.npy"]
    assert 100_000 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(a["B.npy"], B.numpy()[rows.astype(np.int64)])  # the rows it names, in order
    assert np.array_equal(a["F.npy"], F.numpy())
    for f in files:  # the same sample every time
        assert np.array_equal(a[f], np.load(tmp_path / "1" / f, allow_pickle=False)), f
