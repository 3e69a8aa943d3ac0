"""ops.conv2 without its kernels: the fallback is the torch composition itself, the fused MNIST models start from the
bits and keys of the plain ones, and a job runs with --fused-conv2."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tony_amd.models.mnist import mnist_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the form's own shape, a padded plane 65 wide and 16 input channels: on CPU tensors all are the composition
@pytest.mark.parametrize("k,p,cin,hw", [(3, 0, 32, (9, 11)), (5, 2, 32, (9, 11)), (3, 1, 32, (4, 63)), (3, 0, 16, (9, 11))])
def test_cpu_fallback_is_the_composition(k, p, cin, hw):
    from tony_amd.ops.conv2 import conv2_bias_relu_pool

    g = torch.Generator().manual_seed(k)
    x = torch.randn(3, cin, *hw, generator=g, requires_grad=True)
    w, b = torch.randn(64, cin, k, k, generator=g, requires_grad=True), torch.randn(64, generator=g, requires_grad=True)
    y, yr = conv2_bias_relu_pool(x, w, b, p), F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=p)), 2)
    assert torch.equal(y, yr)
    dy = torch.randn(y.shape, generator=g)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), dy), torch.autograd.grad(yr, (x, w, b), dy)):
        assert torch.equal(got, want)


def test_module_takes_only_its_conv():
    from tony_amd.ops.conv2 import Conv2BiasReLUPool

    conv = torch.nn.Conv2d(32, 64, 5, padding=2)
    m = Conv2BiasReLUPool(conv=conv)
    assert m.weight is conv.weight and m.bias is conv.bias and (m.kernel_size, m.padding) == (5, 2)
    for bad in (torch.nn.Conv2d(16, 64, 3), torch.nn.Conv2d(32, 64, 3, stride=2), torch.nn.Conv2d(32, 64, 3, bias=False)):
        with pytest.raises(ValueError):
            Conv2BiasReLUPool(conv=bad)


@pytest.mark.parametrize("name,at", [("deepnn", 3), ("hvd_cnn", 2)])
@pytest.mark.parametrize("stem", [False, True])
def test_fused_model_starts_from_the_same_state(name, at, stem):
    from tony_amd.ops.conv2 import Conv2BiasReLUPool

    plain, fused = mnist_model(name, seed=3), mnist_model(name, seed=3, fused=stem, fused_conv2=True)
    assert isinstance(fused[at], Conv2BiasReLUPool)
    assert isinstance(fused[at + 1], torch.nn.Identity) and isinstance(fused[at + 2], torch.nn.Identity)
    assert isinstance(fused[0], torch.nn.Conv2d) != stem
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) and all(torch.equal(sp[k], sf[k]) for k in sp)
    fused.load_state_dict(sp)  # a checkpoint of either form loads in the other
    x = torch.rand(2, 1, 28, 28)
    assert torch.equal(plain(x), fused(x))


def test_keras_cnn_is_unchanged():
    plain, flagged = mnist_model("keras_cnn", seed=3), mnist_model("keras_cnn", seed=3, fused_conv2=True)
    assert [type(m) for m in plain] == [type(m) for m in flagged]
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), flagged.state_dict().values()))


def test_ddp_job_runs_with_fused_conv2():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tony_amd", "jobs", "mnist_pytorch_ddp.py"), "--model", "deepnn",
                        "--fused-conv2", "--steps-per-epoch", "2", "--batch-size", "8"], capture_output=True, text=True,
                       timeout=240, env={k: v for k, v in os.environ.items() if k not in ("TF_CONFIG", "CLUSTER_SPEC")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fused conv2: Conv2BiasReLUPool" in r.stdout + r.stderr
