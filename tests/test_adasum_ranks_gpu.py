"""``hvd.DistributedOptimizer(op=hvd.Adasum)`` over 2 and 4 ranks on the GPU, ranks as processes placed like
tests/test_ps_layerwise_gpu.py's (tests/adasum_worker.py is the rank body, shared with the gloo test of
tests/test_adasum_cpu.py): a model of parameters of 4, 7, 4096, 4100 and 3 * 4096 + 8 elements over four buckets, fp32
gradients under a fused SGD and bf16 wire gradients under ``Compression.bf16``.

After every backward the ranks' gradient buffers must be bit-identical, inside the derived bound
(tests/adasum_ref.py) against the float64 tree of the local gradients the ranks return, and far outside it from both
the plain sum and the average: a fall-back to an all-reduce cannot pass.  After three steps the variables must be
bit-identical too.  The ``hvd.allreduce`` / ``grouped_allreduce`` forms run on the same ranks."""
import multiprocessing as mp
import socket

import pytest

from gpu_ranks import placement
from test_adasum_cpu import check_api, check_opt

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


@pytest.mark.parametrize("world", [2, 4], ids=[placement(2), placement(4)])
def test_ranks_hold_the_adasum_of_their_gradients(world):
    import adasum_worker as W

    outs = _spawn(W.gpu_rank, world)
    check_opt(outs, world, "fp32", bf16=False, want_fused=True)
    check_opt(outs, world, "bf16", bf16=True, want_fused=True)
    check_api(outs, world)
