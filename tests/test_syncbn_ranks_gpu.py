"""Synchronised BatchNorm over 2 and 3 ranks on the GPU, ranks as processes placed by tests/gpu_ranks.py
(tests/syncbn_worker.py is the rank body, shared with the gloo test of tests/test_syncbn_cpu.py, which also holds the
checks and the derivation of the stack's bound).

Each rank holds a different slice of the batch of a small converted stack -- one ``ConvBNAct``, one ``Bottleneck``
with downsample, 8 to 32 channels, 4 x 4, in bf16 and in fp32 -- and of the rows of two kernel-test cases.  After
forward and backward the
outputs and dx are inside the bound of the float64 full-batch reference and far outside it from per-rank BatchNorm (a
fall-back to local statistics cannot pass); running_mean, running_var and the saved statistics are bit-identical
across ranks; the sum of the ranks' BN parameter gradients is the full-batch gradient.  ``hvd.SyncBatchNorm`` runs
on the same ranks, and under ``tape.recording()`` the op raises."""
import multiprocessing as mp
import socket

import pytest
import torch

from gpu_ranks import placement
from test_syncbn_cpu import check_hvd, check_model, check_ops, check_recording

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=200) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    errors = {r: out[r]["error"] for r in range(world) if "error" in out[r]}
    assert not errors, "\n".join(f"rank {r}: {e}" for r, e in errors.items())
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]  # each rank ends normally
    return [out[r] for r in range(world)]


@pytest.mark.parametrize("world", [2, 3], ids=[placement(2), placement(3)])
def test_ranks_normalise_with_the_statistics_of_all_batches(world):
    import syncbn_worker as W

    outs = _spawn(W.gpu_rank, world)
    check_ops(outs, world)
    check_model([o["model"]["bf16"] for o in outs], world, torch.bfloat16)
    check_model([o["model"]["fp32"] for o in outs], world, torch.float32)
    check_hvd(outs, world)
    check_recording(outs)
