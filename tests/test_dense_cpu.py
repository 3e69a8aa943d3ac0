"""ops.dense without its kernels: the fallback is the torch composition itself, the fused MNIST models start from the
bits and keys of the plain ones, and a job runs with --fused-dense."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tony_amd.models.mnist import MODELS, mnist_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the form's own shape on CPU tensors, K % 4 != 0, and float64: all are the composition
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("k,dtype", [(8, torch.float32), (7, torch.float32), (8, torch.float64)])
def test_fallback_is_the_composition(relu, k, dtype):
    from tony_amd.ops.dense import dense

    g = torch.Generator().manual_seed(k)
    x, w, b = (torch.randn(s, generator=g, dtype=dtype).requires_grad_() for s in ((5, k), (3, k), (3,)))
    y, yr = dense(x, w, b, relu), F.linear(x, w, b)
    yr = F.relu(yr) if relu else yr
    assert torch.equal(y, yr)
    dy = torch.randn(y.shape, generator=g, dtype=dtype)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), dy), torch.autograd.grad(yr, (x, w, b), dy)):
        assert torch.equal(got, want)


def test_module_takes_only_a_linear_with_a_bias():
    from tony_amd.ops.dense import Dense

    lin = torch.nn.Linear(4, 3)
    m = Dense(linear=lin, relu=True)
    assert m.weight is lin.weight and m.bias is lin.bias and (m.in_features, m.out_features, m.relu) == (4, 3, True)
    assert list(Dense(4, 3).state_dict()) == list(lin.state_dict())
    with pytest.raises(ValueError):
        Dense(linear=torch.nn.Linear(4, 3, bias=False))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_fused_model_starts_from_the_same_state(name):
    from tony_amd.ops.dense import Dense

    plain, fused = mnist_model(name, seed=3), mnist_model(name, seed=3, fused_dense=True)
    for i, m in enumerate(plain):
        if isinstance(m, torch.nn.Linear):
            relu = i + 1 < len(plain) and isinstance(plain[i + 1], torch.nn.ReLU)
            assert isinstance(fused[i], Dense) and fused[i].relu == relu
            assert not relu or isinstance(fused[i + 1], torch.nn.Identity)
    assert not any(isinstance(m, torch.nn.Linear) for m in fused)
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) and all(torch.equal(sp[k], sf[k]) for k in sp)
    fused.load_state_dict(sp)  # a checkpoint of either form loads in the other
    x = torch.rand(2, 1, 28, 28)
    assert torch.equal(plain(x), fused(x))


def test_estimator_job_runs_with_fused_dense(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cluster = {"chief": [f"127.0.0.1:{port}"], "ps": ["127.0.0.1:0"]}
    env = {k: v for k, v in os.environ.items() if k != "CLUSTER_SPEC"}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", TONY_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "tony_amd", "jobs", "mnist_estimator.py"), "--fused-dense", "--steps", "3",
           "--batch-size", "8"]
    procs = [subprocess.Popen(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(env, TF_CONFIG=json.dumps({"cluster": cluster, "task": {"type": t, "index": 0}})))
             for t in ("chief", "ps")]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-2000:] for o in outs)
    assert "fused dense: ['Dense(784, 256, relu=True)', 'Dense(256, 128, relu=True)', 'Dense(128, 10, relu=False)']" \
        in outs[0]
    assert "step 3: loss " in outs[0]
