"""bench.py's run modes (CPU): a plain run keeps to the headline figure, ``--full`` adds the CPU
baseline leg, ``--dump-outputs DIR`` writes the last timed step's outputs as float32 ``.npy``."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup) == (7, 3)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def _step_out(n):
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(n, 23, generator=g)
    rew = torch.randn(n, generator=g)
    term = torch.rand(n, generator=g) < 0.3
    return {"policy": obs}, rew, term, ~term, {"log": {}}


def test_dump_outputs_writes_what_step_returned(tmp_path):
    out = _step_out(37)
    bench.dump_outputs(str(tmp_path / "d"), out)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["obs_policy", "reward", "terminated", "truncated"]
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["obs_policy"], out[0]["policy"].numpy())
    np.testing.assert_array_equal(got["reward"], out[1].numpy())
    np.testing.assert_array_equal(got["terminated"], out[2].numpy().astype(np.float32))
    np.testing.assert_array_equal(got["truncated"], 1.0 - got["terminated"])


def test_dump_outputs_samples_fixed_rows_past_the_cap(tmp_path, monkeypatch):
    out = _step_out(100)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * (23 + 3 + 2) * 4)   # room for 10 env rows and their indices
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out, rank=1, world=2)
    rows = np.load(tmp_path / "a" / "env_rows.npy").astype(int)
    assert len(rows) == 10 and len(set(rows)) == 10
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "env_rows_rank1.npy").astype(int))  # same draw
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obs_policy.npy"), out[0]["policy"].numpy()[rows])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 10 * (23 + 3 + 2) * 4 + 5 * 128 + 1
