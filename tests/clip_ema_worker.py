"""Rank body for tests/test_optim_clip_ema_cpu.py (gloo, CPU tensors) and tests/test_ps_clip_gpu.py (one process
per rank, placed by tests/gpu_ranks.py): the parameter server (colocated, or dedicated with several ps tasks) with
``clip_norm`` and an EMA over several buckets.  The gradient schedule is tests/optim_plane_worker.py's (multiples of 1/8: exact in bf16, and so is
their sum over the workers), so the pushed sums carry no rounding of their own."""
import os

import torch
import torch.distributed as dist

from optim_plane_worker import _grad
from ps_plane_worker import _Net

KIND, LR, MOMENTUM, EMA = "rmsprop_tf", 0.1, 0.9, 0.9
# the averaged gradient's norm is about 135, 220 and 305 at step % 3 = 0, 1, 2 (54208 elements): steps 0 and 3
# pass unclipped, steps 1 and 2 clip.  A rank's own shard (half of every bucket) has norm / sqrt(2): about 95,
# 155 and 215, so a per-shard norm would clip step 2 alone, and by another factor
CLIP = 200.0
MASTER_TOL = dict(rtol=1e-5, atol=1e-4)   # tests/optim_plane_worker.py: fp32 masters vs the CPU class
PARAMS_TOL = dict(rtol=1e-2, atol=2e-2)   # ... and the landed bf16 variables vs the rounded reference


def _shard_index(ps):
    """Flat positions of the elements this rank owns, in its master shard's order (colocated: its piece of every
    bucket; dedicated: the whole of the buckets placed on it)."""
    idx = torch.empty(ps.optimizers[ps.rank].w.numel(), dtype=torch.long)
    for b in ps.buckets:
        if ps._master_range[b.index] is None:
            continue
        m, p = ps._master_range[b.index]
        lo = b.lo + ps.rank * p if ps.mode == "colocated" else b.lo
        idx[m:m + p] = torch.arange(lo, lo + p)
    return idx


def body(rank, world, dev, dtype, steps=4, mode="colocated", ps_ranks=(0,)):
    from tony_amd.parallel.ps import ParameterServer, make_optimizer

    torch.manual_seed(0)
    net = _Net([11000, 12000, 4136, 13000, 3000, 11008, 64])
    with torch.no_grad():
        for p in net.ps:
            p.copy_(torch.randn(p.shape).mul_(0.5))
    ps = ParameterServer(net, optimizer=KIND, lr=LR, momentum=MOMENTUM, mode=mode, ps_ranks=ps_ranks, dtype=dtype,
                         device=dev, bucket_mb=0.02, clip_norm=CLIP, ema_decay=EMA, plane="rccl")
    assert len(ps.buckets) > 3 and not ps.single and ps.plane is None
    n = ps.flat.numel
    w0 = ps.flat.data.float().cpu().clone()
    idx = torch.arange(n, dtype=torch.float32)
    norms = []
    opt = ps.optimizers.get(rank)
    nw = len(ps.worker_ranks)
    for s in range(steps):
        ps.begin_step(overlap=False)
        if ps.is_worker:
            ps.flat.grad.copy_(_grad(s, ps.worker_ranks.index(rank), idx).to(dev))
        ps.step()
        if opt is not None:
            norms.append(opt.last_norm())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    # the same schedule on the CPU class: the workers' gradients summed in worker order, x 1 / workers, the norm
    # taken over the WHOLE averaged gradient
    ref = make_optimizer(KIND, w0.clone(), LR, MOMENTUM, clip_norm=CLIP, ema_decay=EMA)
    ref.grad_scale = 1.0 / nw
    ref_norms = []
    for s in range(steps):
        tot = torch.zeros(n)
        for w in range(nw):
            tot += _grad(s, w, idx)
        ref.step(tot)
        ref_norms.append(ref.last_norm())
    got = ps.flat.data.float().cpu()
    exp = ref.w.to(dtype).float()
    vtol = MASTER_TOL if dtype == torch.float32 else PARAMS_TOL
    res = {"flat": ps.flat.data.cpu().clone(), "norms": norms, "ref_norms": ref_norms,
           "clipped": [x > CLIP for x in ref_norms],
           "params_err": (got - exp).abs().max().item(),
           "params_match": bool(torch.allclose(got, exp, **vtol)),
           "params_moved": bool((ref.w - w0).abs().min() > 0.05)}
    if opt is not None:
        res.update(_shard_checks(ps, opt, ref, w0, idx, steps, nw))
    # evaluation on the EMA: every rank sees the whole EMA, then exactly the variables it had
    before = ps.flat.data.clone()
    with ps.ema_weights():
        inside = ps.flat.data.float().cpu()
        res["ema_flat"] = ps.flat.data.cpu().clone()
        res["ema_weights_match"] = bool(torch.allclose(inside, ref.ema.to(dtype).float(), **vtol))
        res["ema_weights_differ_from_params"] = not torch.equal(ps.flat.data, before)
    res["restored"] = bool(torch.equal(ps.flat.data, before))
    return res


def _shard_checks(ps, opt, ref, w0, idx, steps, nw):
    """An owner's fp32 masters and EMA against the reference, and against the deliberately wrong one."""
    from tony_amd.parallel.ps import make_optimizer

    n = ps.flat.numel
    mine = _shard_index(ps)
    # the deliberately wrong one: this rank's shard alone, clipped by the norm of the shard
    wrong = make_optimizer(KIND, w0[mine].clone(), LR, MOMENTUM, clip_norm=CLIP)
    wrong.grad_scale = 1.0 / nw
    for s in range(steps):
        tot = torch.zeros(n)
        for w in range(nw):
            tot += _grad(s, w, idx)
        wrong.step(tot[mine])
    master = opt.w.float().cpu()
    return {"master_err": (master - ref.w[mine]).abs().max().item(),
            "master_match": bool(torch.allclose(master, ref.w[mine], **MASTER_TOL)),
            "ema_match": bool(torch.allclose(opt.ema.float().cpu(), ref.ema[mine], **MASTER_TOL)),
            "wrong_err": (master - wrong.w).abs().max().item(),
            "per_shard_norm_differs": not torch.allclose(master, wrong.w, **MASTER_TOL)}


def cpu_rank(rank, world, port, mode="colocated", ps_ranks=(0,)):
    """tests/test_dist_cpu.py's pattern: a pool task per rank, fp32 variables over gloo."""
    from dist_workers import _init

    _init(rank, world, port)
    try:
        return body(rank, world, torch.device("cpu"), torch.float32, mode=mode, ps_ranks=ps_ranks)
    finally:
        dist.destroy_process_group()


def gpu_rank(rank, world, port, q):
    """tests/test_optim_plane_gpu.py's pattern: a process per rank, bf16 variables, the result on a queue."""
    import gpu_ranks

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dev, _ = gpu_ranks.init(rank, world)
        q.put((rank, body(rank, world, dev, torch.bfloat16)))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, {"error": f"{e!r}\n{traceback.format_exc()}"}))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
