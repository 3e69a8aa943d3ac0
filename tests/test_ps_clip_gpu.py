"""The colocated parameter server with ``clip_norm`` and an EMA over two ranks on the GPU: bf16 variables, more
than 3 buckets, each rank owning half of every bucket, ranks as processes placed like
tests/test_optim_plane_gpu.py's (tests/clip_ema_worker.py is the rank body, shared with the gloo test of
tests/test_optim_clip_ema_cpu.py).

Both ranks must end with bit-identical variables and have computed the same norm to the bit; their fp32 masters
must follow the CPU class that clips by the norm of the WHOLE averaged gradient, and must NOT follow a reference
that clips each shard by its own norm.
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


@pytest.mark.parametrize("world", [2], ids=[placement(2)])
def test_two_ranks_clip_by_one_global_norm(world):
    import torch

    import clip_ema_worker as W

    out = _spawn(W.gpu_rank, world)
    for r in range(world):
        print(r, {k: v for k, v in out[r].items() if k.endswith("_err") or k.endswith("norms")})
    assert torch.equal(out[0]["flat"], out[1]["flat"])
    assert torch.equal(out[0]["ema_flat"], out[1]["ema_flat"])
    for r in range(world):
        o = out[r]
        assert o["norms"] == out[0]["norms"]  # every rank computed the same norm, to the bit
        assert o["norms"] == pytest.approx(o["ref_norms"], rel=1e-6)
        assert any(o["clipped"]) and not all(o["clipped"])
        bad = [k for k, v in o.items() if v is False]
        assert not bad, (r, bad, {k: v for k, v in o.items() if not torch.is_tensor(v)})
