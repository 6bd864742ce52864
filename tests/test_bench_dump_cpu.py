"""bench.py's command line and --dump-outputs, without a GPU: the sampled arrays are float32, deterministic, taken from the tensors the
step left behind, and small enough at the headline shape; --steps below 1 is refused before any device work."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _toy():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(96, 80), torch.nn.LayerNorm(80))           # 7680 > DUMP_PER_PARAM elements: sampled
    m(torch.randn(4, 96)).square().sum().backward()
    logits = torch.randn(2, 5, 7, dtype=torch.bfloat16)
    return m, logits, torch.tensor(3.25)


def _dump(tmp_path, name):
    m, logits, loss = _toy()
    d = tmp_path / name
    bench.dump_outputs(str(d), loss, logits, m)
    return {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}, m, logits


def test_dump_outputs_files_and_determinism(tmp_path):
    a, m, logits = _dump(tmp_path, "a")
    b, _, _ = _dump(tmp_path, "b")
    assert sorted(a) == ["grads_sample", "logits_sample", "loss", "params_sample"]
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    assert a["loss"].tolist() == [3.25]
    assert a["logits_sample"].shape == (bench.DUMP_LOGITS,)
    assert np.isin(a["logits_sample"], logits.float().numpy().ravel()).all()
    sizes = [min(p.numel(), bench.DUMP_PER_PARAM) for p in m.parameters()]
    assert a["params_sample"].shape == a["grads_sample"].shape == (sum(sizes),)
    # parameters no larger than the per-parameter sample are written whole, in order
    o = sizes[0]
    for p in list(m.parameters())[1:]:
        n = p.numel()
        assert np.array_equal(a["params_sample"][o:o + n], p.detach().numpy().ravel())
        assert np.array_equal(a["grads_sample"][o:o + n], p.grad.numpy().ravel())
        o += n
    w = m[0].weight
    assert np.isin(a["grads_sample"][:sizes[0]], w.grad.numpy().ravel()).all()


def test_dump_outputs_without_logits(tmp_path):
    m, _, loss = _toy()
    bench.dump_outputs(str(tmp_path), loss, None, m)
    assert sorted(os.listdir(tmp_path)) == ["grads_sample.npy", "loss.npy", "params_sample.npy"]


def test_dump_size_at_the_headline_shape():
    tensors = 3 + bench.L * 12 + 2                                   # embeddings + LayerNorm, 12 per block, final LayerNorm
    total = 4 * (1 + bench.DUMP_LOGITS + 2 * tensors * bench.DUMP_PER_PARAM)
    assert total <= 64 * 2 ** 20, total


def test_command_line(capsys):
    with pytest.raises(SystemExit) as e:
        bench.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--full" in out and "--dump-outputs" in out
    with pytest.raises(SystemExit) as e:
        bench.main(["--steps", "0"])
    assert e.value.code == 2
