"""Rank bodies of the Adasum tests: tests/test_adasum_cpu.py (a pool task per rank, gloo, CPU tensors) and
tests/test_adasum_ranks_gpu.py (a process per rank, placed by tests/gpu_ranks.py, the result on a queue).

``api_body`` calls ``hvd.allreduce`` / ``grouped_allreduce`` / the async forms with ``op=hvd.Adasum`` on this rank's
gradients of ``adasum_ref.make_grads``; ``opt_body`` trains a model of parameters of ``adasum_ref.LENGTHS`` through
``hvd.DistributedOptimizer(op=hvd.Adasum)`` over more than three buckets.  The loss of a step is ``sum_t p_t . g_t``
with ``g`` this rank's gradient of that step, so the local gradient is known to the bit; it is still read back from the
gradient buffer of a backward pass without reduction, and returned.  Everything goes back as bytes: the parent holds
the references and does the comparing."""
import os

import numpy as np
import torch
import torch.distributed as dist

import adasum_ref as R
from ps_plane_worker import _Net

STEPS = 3
BUCKET_MB = 0.001  # 262 fp32 elements: every large tensor its own bucket, the two tiny ones together -- 4 buckets
CONFIGS = {"fp32": None, "bf16": "bf16"}  # name -> wire compression


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    return _np(t).tobytes()


def api_body(rank, world, dev, hvd):
    grads, segs = R.make_grads(world, seed=11)
    offs = [lo for lo, _ in segs]
    mine = [torch.from_numpy(grads[rank][o:o + n].copy()).to(dev) for o, n in zip(offs, R.LENGTHS)]
    res = {}
    for k in (1, 4):  # 7 elements: not a multiple of anything; 3 * 4096 + 8: several work items
        keep = mine[k].clone()
        res[f"single{k}"] = _bits(hvd.allreduce(mine[k], op=hvd.Adasum))
        res[f"single{k}_input_kept"] = bool(torch.equal(keep, mine[k]))
    res["grouped"] = [_bits(t) for t in hvd.grouped_allreduce(mine, op=hvd.Adasum)]
    # Adasum commutes with a power of two: x 0.5 before and x 2 after must give the same bits
    res["scaled"] = [_bits(t) for t in hvd.grouped_allreduce(mine, op=hvd.Adasum, prescale_factor=0.5,
                                                              postscale_factor=2.0)]
    t = mine[3].clone()
    h = hvd.allreduce_async_(t, op=hvd.Adasum)
    res["async_complete_at_issue"] = bool(hvd.poll(h))
    res["async_inplace"] = hvd.synchronize(h) is t
    res["async"] = _bits(t)
    h = hvd.allreduce_async(mine[3], op=hvd.Adasum)
    res["async_copy"] = _bits(hvd.synchronize(h))
    inplace = mine[2].clone()
    res["inplace_returns_argument"] = hvd.allreduce_(inplace, op=hvd.Adasum) is inplace
    res["inplace"] = _bits(inplace)
    for name, call in (("int_single", lambda: hvd.allreduce(torch.arange(8, device=dev), op=hvd.Adasum)),
                       ("int_grouped", lambda: hvd.grouped_allreduce([mine[0], torch.arange(8, device=dev)],
                                                                     op=hvd.Adasum))):
        try:
            call()
            res[f"{name}_raises_type_error"] = False
        except TypeError:
            res[f"{name}_raises_type_error"] = True
    return res


def opt_body(rank, world, dev, hvd, compression=None, steps=STEPS):
    torch.manual_seed(100 + rank)  # every rank its own start: the wrapper must broadcast rank 0's
    net = _Net(R.LENGTHS).to(dev)
    with torch.no_grad():
        for p in net.ps:
            p.copy_(torch.randn(p.shape))
    opt = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
    comp = hvd.Compression.bf16 if compression == "bf16" else hvd.Compression.none
    dopt = hvd.DistributedOptimizer(opt, named_parameters=net.named_parameters(), op=hvd.Adasum,
                                    bucket_mb=BUCKET_MB, compression=comp)
    (flat, red), = dopt.groups
    offs, segs, n = R.layout()
    res = {"buckets": len(red.buckets), "fused": bool(dopt._fused), "reduce": red.reduce,
           "layout_matches": [s.offset for s in flat.slots] == offs and flat.numel == n,
           "local": [], "grad": []}
    for s in range(steps):
        grads, _ = R.make_grads(world, seed=1000 + s)
        target = torch.from_numpy(grads[rank]).to(dev)

        def loss():
            return sum((p * target[o:o + p.numel()]).sum() for p, o in zip(net.ps, offs))

        red.enabled = False  # this rank's own gradient, as backward leaves it in the buffer
        dopt.zero_grad()
        loss().backward()
        res["local"].append(_bits(flat.grad))
        red.enabled = True
        dopt.zero_grad()
        loss().backward()
        res["grad"].append(_bits(flat.grad))
        dopt.step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    res["vars"] = _bits(flat.data)
    res["launches"] = red.launches
    return res


def _refusals(hvd):
    """Three ranks: the operator raises ValueError where it is requested, before anything is sent."""
    res = {}
    net = _Net([8, 8])
    calls = {"allreduce": lambda: hvd.allreduce(torch.ones(8), op=hvd.Adasum),
             "grouped": lambda: hvd.grouped_allreduce([torch.ones(8)], op=hvd.Adasum),
             "optimizer": lambda: hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1),
                                                           op=hvd.Adasum)}
    for name, call in calls.items():
        try:
            call()
            res[name] = "no error"
        except ValueError as e:
            res[name] = f"ValueError: {e}"
    hvd.barrier()
    return res


def cpu_rank(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TONY_DIST_BACKEND="gloo")
    torch.set_num_threads(1)
    import tony_amd.hvd as hvd

    hvd.init()
    try:
        if world & (world - 1):
            return {"refusals": _refusals(hvd)}
        dev = torch.device("cpu")
        return {"api": api_body(rank, world, dev, hvd), "opt": opt_body(rank, world, dev, hvd)}
    finally:
        hvd.shutdown()


def gpu_rank(rank, world, port, q):
    import gpu_ranks

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dev, _ = gpu_ranks.init(rank, world)
        import tony_amd.hvd as hvd

        hvd.init()  # takes the process group that is up (tests/gpu_ranks.py chose its backend) as it is
        assert hvd.size() == world and hvd.rank() == rank and hvd.device() == dev
        out = {name: opt_body(rank, world, dev, hvd, comp) for name, comp in CONFIGS.items()}
        out["api"] = api_body(rank, world, dev, hvd)
        q.put((rank, out))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, {"error": f"{e!r}\n{traceback.format_exc()}"}))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
