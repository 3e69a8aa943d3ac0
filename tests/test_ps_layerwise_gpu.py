"""The colocated parameter server with ``optimizer="lars"`` / ``"lamb"`` over two ranks on the GPU: bf16 variables,
more than 3 buckets, each rank owning half of every bucket so that piece boundaries cut parameter tensors, ranks as
processes placed like tests/test_ps_clip_gpu.py's (tests/layerwise_worker.py is the rank body, shared with the gloo
test of tests/test_layerwise_cpu.py).

Both ranks must end with bit-identical variables and identical ratio tables; their fp32 masters must follow the
float64 loop that takes norms over WHOLE tensors and must NOT follow the loop that takes each rank's piece as a tensor
of its own.
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
def test_two_ranks_take_whole_tensor_ratios(world):
    import layerwise_worker as W

    out = _spawn(W.gpu_rank, world)
    for name in W.CONFIGS:
        a, b = out[0][name], out[1][name]
        for o in (a, b):
            print(name, {k: v for k, v in o.items() if not isinstance(v, bytes)})
        assert a["flat"] == b["flat"] and len(a["flat"]) > 2 * 54000     # the bf16 variables, bit for bit
        assert a["table"] == b["table"] and len(a["table"]) == 8 * 7     # the same (ratio_t, wd_t), to the bit
        for r, o in enumerate((a, b)):
            bad = [k for k, v in o.items() if v is False]
            assert not bad, (name, r, bad, {k: v for k, v in o.items() if not isinstance(v, bytes)})
            assert o["refs_err"] > 100 * (1e-5 + 1e-4 * 16)  # the two references are far apart
