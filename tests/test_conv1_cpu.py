"""ops.conv1 without its kernels: the fallback is the torch composition itself, the fused MNIST models start from the
bits and keys of the plain ones, and a job runs with --fused-stem."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tony_amd.models.mnist import mnist_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k,p", [(3, 0), (5, 2)])
def test_cpu_fallback_is_the_composition(k, p):
    from tony_amd.ops.conv1 import conv1_bias_relu

    g = torch.Generator().manual_seed(k)
    x = torch.randn(3, 1, 9, 11, generator=g, requires_grad=True)
    w, b = torch.randn(32, 1, k, k, generator=g, requires_grad=True), torch.randn(32, generator=g, requires_grad=True)
    y, yr = conv1_bias_relu(x, w, b, p), F.relu(F.conv2d(x, w, b, padding=p))
    assert torch.equal(y, yr)
    dy = torch.randn(y.shape, generator=g)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), dy), torch.autograd.grad(yr, (x, w, b), dy)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["deepnn", "keras_cnn", "hvd_cnn"])
def test_fused_model_starts_from_the_same_state(name):
    from tony_amd.ops.conv1 import Conv1BiasReLU

    plain, fused = mnist_model(name, seed=3), mnist_model(name, seed=3, fused=True)
    assert isinstance(fused[0], Conv1BiasReLU) and isinstance(fused[1], torch.nn.Identity)
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) and all(torch.equal(sp[k], sf[k]) for k in sp)
    plain.load_state_dict(sf)  # a checkpoint of either form loads in the other
    x = torch.rand(2, 1, 28, 28)
    assert torch.equal(plain(x), fused(x))


def test_allreduce_job_runs_with_fused_stem():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tony_amd", "jobs", "mnist_tf_allreduce.py"), "--fused-stem",
                        "--steps", "2", "--per-worker-batch", "8"], capture_output=True, text=True, timeout=240,
                       env={k: v for k, v in os.environ.items() if k not in ("TF_CONFIG", "CLUSTER_SPEC")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fused stem: Conv1BiasReLU" in r.stdout + r.stderr
