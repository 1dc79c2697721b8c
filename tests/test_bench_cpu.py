"""bench.py --dump-outputs on the host: the files it writes, their dtypes, their size bound, and the fixed sample of a large weight
buffer (the same positions from run to run, so that two builds can be compared output for output)."""
import os
import types

import numpy as np
import torch

import bench


def _dump(tmp_path, n, tag):
    trainer = types.SimpleNamespace(master=torch.arange(n, dtype=torch.float32))
    terms = {"out": torch.tensor(2.5), "temporal_ae": torch.tensor(0.25, dtype=torch.bfloat16)}
    d = tmp_path / tag
    bench.dump_outputs(str(d), terms, trainer)
    return {f: np.load(d / f) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_loss_terms_and_small_weights_whole(tmp_path):
    got = _dump(tmp_path, 1000, "small")
    assert sorted(got) == ["loss_out.npy", "loss_temporal_ae.npy", "master_weights.npy"]
    assert got["loss_out.npy"].dtype == np.float64 and float(got["loss_out.npy"]) == 2.5
    assert float(got["loss_temporal_ae.npy"]) == 0.25
    w = got["master_weights.npy"]
    assert w.dtype == np.float32 and np.array_equal(w, np.arange(1000, dtype=np.float32))


def test_dump_outputs_stays_within_64_mb():
    assert bench.DUMP_WEIGHTS * 4 <= 48 << 20


def test_dump_outputs_samples_large_weights_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_WEIGHTS", 1000)
    n = 3 * bench.DUMP_WEIGHTS + 5
    a = _dump(tmp_path, n, "a")["master_weights.npy"]
    b = _dump(tmp_path, n, "b")["master_weights.npy"]
    assert a.shape == (bench.DUMP_WEIGHTS,) and np.array_equal(a, b)
    idx = a.astype(np.int64)                   # (the buffer holds its own indices)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.all(idx // 3 == np.arange(bench.DUMP_WEIGHTS))       # one element per stride of 3
