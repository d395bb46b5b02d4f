"""bench.py's command line on the host: `--full` / `--dump-outputs` parse, and the dumped outputs are float32, stay under
64 MB at the bench's shapes and are the same bits for the same logits."""
import sys

import numpy as np
import torch

import bench

NAMES = ("logits_first_sample", "logits_last_sample", "logits_seeded_sample")


def test_plain_run_is_headline_only_unless_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out_dir"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out_dir"


def test_dump_outputs_float32_deterministic(tmp_path):
    out = torch.randn(3, 114, 4001, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(out, tmp_path / "a")
    bench.dump_outputs(out.clone(), tmp_path / "b")
    for n in NAMES:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y), n
    assert np.array_equal(np.load(tmp_path / "a" / "logits_first_sample.npy"), out[0].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "logits_last_sample.npy"), out[-1].numpy())
    s = np.load(tmp_path / "a" / "logits_seeded_sample.npy")
    assert s.shape == (min(bench.DUMP_SAMPLE, out.numel()),)
    assert np.isin(s, out.numpy()).all()


def test_dump_outputs_bounded_at_the_bench_shape(tmp_path):
    """B = 32 x 114 positions x 32002 logits (467 MB in float32) -> well under 64 MB; bf16 logits (the gather's wire
    format) are written as float32 too."""
    out = torch.zeros(32, 114, 32002, dtype=torch.bfloat16)
    bench.dump_outputs(out, tmp_path)
    total = sum((tmp_path / f"{n}.npy").stat().st_size for n in NAMES)
    assert total < 64 << 20, total
    assert np.load(tmp_path / "logits_first_sample.npy").shape == (114, 32002)
    assert all(np.load(tmp_path / f"{n}.npy").dtype == np.float32 for n in NAMES)


def test_dump_outputs_caps_long_sequences(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 10 * 1000 * 4)
    bench.dump_outputs(torch.ones(2, 50, 1000), tmp_path)
    assert np.load(tmp_path / "logits_first_sample.npy").shape == (10, 1000)
    assert np.load(tmp_path / "logits_last_sample.npy").shape == (10, 1000)
