"""ops.conv1 with pool=True without its kernels: the fallback is the torch composition itself, deepnn with fused_pool
starts from the bits and keys of the plain one, the other models ignore the flag, and a job runs with
--fused-stem-pool."""
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
    y, yr = conv1_bias_relu(x, w, b, p, pool=True), F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=p)), 2)
    assert torch.equal(y, yr)
    dy = torch.randn(y.shape, generator=g)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), dy), torch.autograd.grad(yr, (x, w, b), dy)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("others", [False, True])
def test_deepnn_with_fused_pool_starts_from_the_same_state(others):
    from tony_amd.ops.conv1 import Conv1BiasReLU

    plain = mnist_model("deepnn", seed=3)
    fused = mnist_model("deepnn", seed=3, fused_pool=True, fused_conv2=others, fused_dense=others)
    assert isinstance(fused[0], Conv1BiasReLU) and fused[0].pool and "pool=True" in repr(fused[0])
    assert isinstance(fused[1], torch.nn.Identity) and isinstance(fused[2], torch.nn.Identity)
    assert isinstance(mnist_model("deepnn", fused=True)[2], torch.nn.MaxPool2d)  # fused alone keeps the pool apart
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) and all(torch.equal(sp[k], sf[k]) for k in sp)
    fused.load_state_dict(sp)  # a checkpoint of either form loads in the other
    x = torch.rand(2, 1, 28, 28)
    assert torch.equal(plain(x), fused(x))


@pytest.mark.parametrize("name", ["hvd_cnn", "keras_cnn"])
def test_models_without_that_pool_take_the_flag_as_fused(name):
    a, b = mnist_model(name, seed=3, fused=True), mnist_model(name, seed=3, fused_pool=True)
    assert [repr(m) for m in a] == [repr(m) for m in b] and "pool" not in repr(b[0])
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))


def test_ddp_job_runs_with_fused_stem_pool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tony_amd", "jobs", "mnist_pytorch_ddp.py"), "--model",
                        "deepnn", "--fused-stem-pool", "--steps-per-epoch", "2", "--batch-size", "8"],
                       capture_output=True, text=True, timeout=240,
                       env={k: v for k, v in os.environ.items() if k not in ("TF_CONFIG", "CLUSTER_SPEC")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fused stem: Conv1BiasReLU" in r.stdout + r.stderr and "pool=True" in r.stdout + r.stderr
