"""ops.dense_xent without its kernels: the fallback is the torch composition to the bit, ``mnist_loss(fused_head=True)``
is the jobs' loss line on every model, and a job runs with --fused-head."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tony_amd.models.mnist import MODELS, mnist_loss, mnist_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grads(loss, params):
    return torch.autograd.grad(loss, [p for p in params if p is not None])


# the form's own shape on CPU tensors, then K % 4 != 0, N > 32, float64, no bias and a non-contiguous x
@pytest.mark.parametrize("case", ["form", "k7", "n33", "f64", "nobias", "strided"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_fallback_is_the_composition(case, reduction):
    from tony_amd.ops.dense_xent import dense_xent

    k, n = 7 if case == "k7" else 8, 33 if case == "n33" else 10
    g = torch.Generator().manual_seed(k + n)
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64 if case == "f64" else torch.float32).requires_grad_()
               for s in ((6, 2 * k if case == "strided" else k), (n, k), (n,)))
    b = None if case == "nobias" else b
    xs = x[:, ::2] if case == "strided" else x
    y = torch.randint(0, n, (6,), generator=g)
    loss, logits = dense_xent(xs, w, b, y, reduction=reduction, return_logits=True)
    want = F.cross_entropy(F.linear(xs, w, b).float(), y, reduction="none")  # the losses are fp32 whatever the dtype
    want = want.mean() if reduction == "mean" else want.sum() if reduction == "sum" else want
    assert torch.equal(loss, want) and torch.equal(logits, F.linear(xs, w, b)) and not logits.requires_grad
    go = torch.randn(loss.shape, generator=g)
    for got, ref in zip(_grads((loss * go).sum(), (x, w, b)), _grads((want * go).sum(), (x, w, b))):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("fused_dense", [False, True])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_fused_head_is_the_loss_line(name, fused_dense):
    model = mnist_model(name, seed=3, fused_dense=fused_dense)
    keys = list(model.state_dict())
    x, y = torch.rand(4, 1, 28, 28), torch.tensor([3, 0, 9, 3])
    fused, plain = mnist_loss(model, x, y, fused_head=True), F.cross_entropy(model(x), y)
    assert torch.equal(mnist_loss(model, x, y), plain) and list(model.state_dict()) == keys
    # the value is the mean of the same four fp32 losses summed by another torch kernel: three additions and a division
    # of positive terms, 4 * 2^-24 relative at the most each way; every row's gradient is 1/4 both ways
    torch.testing.assert_close(fused, plain, rtol=2.0 ** -21, atol=0)
    params = list(model.parameters())
    assert all(torch.equal(got, ref) for got, ref in zip(_grads(fused, params), _grads(plain, params)))


def test_fused_head_refuses_a_model_without_a_linear_head():
    with pytest.raises(TypeError):
        mnist_loss(torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.ReLU()), torch.rand(2, 4), torch.tensor([0, 1]),
                   fused_head=True)


def test_estimator_job_runs_with_fused_head(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cluster = {"chief": [f"127.0.0.1:{port}"], "ps": ["127.0.0.1:0"]}
    env = {k: v for k, v in os.environ.items() if k != "CLUSTER_SPEC"}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", TONY_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "tony_amd", "jobs", "mnist_estimator.py"), "--fused-head", "--steps", "3",
           "--batch-size", "8"]
    procs = [subprocess.Popen(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(env, TF_CONFIG=json.dumps({"cluster": cluster, "task": {"type": t, "index": 0}})))
             for t in ("chief", "ps")]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-2000:] for o in outs)
    assert "fused head: Linear(in_features=128, out_features=10, bias=True) + cross-entropy" in outs[0]
    assert "step 3: loss " in outs[0]
