"""Adagrad and TF-style RMSProp on the PS data plane (csrc/ps_plane.hip tony_ps_apply, opt 2 and 3): 1 ps + 2
workers, synchronous, plane="xgmi", as processes placed like tests/test_ps_plane_gpu.py's.

The workers push that file's exactly-representable gradient schedule for 4 steps; the ps's fp32 masters must
follow the CPU class replaying it (sum of the workers' gradients in worker order, grad_scale 1/2) and every
worker's landed parameters the rounded reference.

Asynchronous applies of these optimizers depend on the order in which the workers' pushes arrive once there
is more than one worker (the updates do not commute, unlike momentum-free SGD's), so they are not asserted
here.
"""
import multiprocessing as mp
import socket

import pytest

from gpu_ranks import placement

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
    return out


@pytest.mark.parametrize("kind,wire", [("adagrad", None), ("rmsprop_tf", "fp32")],
                         ids=[f"adagrad-bf16wire-{placement(3)}", f"rmsprop_tf-fp32wire-{placement(3)}"])
def test_ps_plane_applies_the_new_optimizers(kind, wire, monkeypatch):
    import torch

    import optim_plane_worker as W

    monkeypatch.setenv("TONY_PS_SPIN_S", "60")
    world = 3
    out = _spawn(W.run, world, kind, torch.float32 if wire == "fp32" else None)
    print({r: {k: v for k, v in out[r].items() if k.endswith("_err")} for r in range(world)})
    for r in range(world):
        bad = [k for k, v in out[r].items() if v is False]
        assert not bad, (r, bad, out[r])
    assert "master_match" in out[0]
    assert out[0]["pushed"] == 0 and all(out[r]["pushed"] > 0 for r in range(1, world))
