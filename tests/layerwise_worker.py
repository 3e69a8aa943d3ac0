"""Rank body for tests/test_layerwise_cpu.py (gloo, CPU tensors) and tests/test_ps_layerwise_gpu.py (one process per
rank, placed by tests/gpu_ranks.py): the colocated parameter server with ``optimizer="lars"`` / ``"lamb"`` over
several buckets, each rank owning half of every bucket, so that parameter tensors are cut by piece boundaries.

The first 30 % of every tensor has its weights scaled by 8 and its gradients by 4: wherever a piece boundary cuts a
tensor, the two pieces' own norms give other trust ratios than the whole tensor's.  Gradients are multiples of 1/8
below 16 (exact in bf16, and so is their sum over two workers), so the pushed sums carry no rounding of their own."""
import os

import torch
import torch.distributed as dist

from layerwise_ref import RefLAMB, RefLARS
from ps_plane_worker import _Net

SIZES = [11000, 12000, 4136, 13000, 3000, 11008, 64]
VS_TORCH = dict(rtol=1e-4, atol=1e-5)
FAR = dict(rtol=100 * 1e-4, atol=100 * 1e-5)  # "differs by more than 100 times the tolerance"
CONFIGS = {
    "lars": dict(optimizer="lars", lr=0.5, momentum=0.9, weight_decay=1e-3, trust_coef=0.02),
    "lamb": dict(optimizer="lamb", lr=0.02, weight_decay=1e-2),
    "lamb-clip": dict(optimizer="lamb", lr=0.02, weight_decay=1e-2, clip_norm=150.0, skip_nonfinite=True),
}


def _adapt(name, p):
    return p.numel() != 64  # the 1-D test tensors are adapted (the default rule would skip them), the last is not


def _pattern(flat):
    """1 on every tensor, 2 on its first 30 % (there the weights are x 8 and the gradients x 4), 0 on the padding
    between tensors (no gradient is ever written there)."""
    e = torch.zeros(flat.numel)
    for s in flat.slots:
        e[s.offset:s.offset + s.numel] = 1.0
        e[s.offset:s.offset + (3 * s.numel) // 10] = 2.0
    return e


def _grad(step, widx, n, e):
    g = torch.Generator().manual_seed(1000 * step + widx)
    base = (torch.randn(n, generator=g) * 8).round().clamp_(-16, 16) / 8  # multiples of 1/8 in [-2, 2]
    return base * torch.where(e == 2.0, 4.0, e) * (0.25 if step % 2 else 1.0)  # the norm: about 390, 97, 390, ...


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()


def _flat_segments(ps, rank):
    """(flat_lo, flat_hi, tensor) of the segments of ``rank``'s master shard, in flat coordinates."""
    from tony_amd.parallel.flat import build_segments

    out = []
    for b in sorted(ps.buckets, key=lambda b: b.lo):
        p = b.numel // ps.world
        lo = b.lo + rank * p
        seg = build_segments(ps.flat, [(lo, lo + p)], _adapt)
        out += [(lo + a, lo + c, t) for a, c, t in zip(seg.starts, seg.starts[1:], seg.tensor)]
    return out


def _reference(cfg, w0, segs, adapt, nw):
    kw = {k: v for k, v in cfg.items() if k not in ("optimizer", "skip_nonfinite")}
    return (RefLARS if cfg["optimizer"] == "lars" else RefLAMB)(w0, segs, adapt, grad_scale=1.0 / nw, **kw)


def one(name, rank, world, dev, dtype, steps=4):
    from tony_amd.parallel.ps import ParameterServer

    cfg = CONFIGS[name]
    torch.manual_seed(0)
    net = _Net(SIZES)
    ps = ParameterServer(net, mode="colocated", dtype=dtype, device=dev, bucket_mb=0.02, plane="rccl",
                         adapt_filter=_adapt, **cfg)
    assert len(ps.buckets) > 3 and not ps.single and ps.plane is None and ps._norm_deferred
    f, opt = ps.flat, ps.optimizers[rank]
    n, nw = f.numel, len(ps.worker_ranks)
    e = _pattern(f)
    # the variables: multiples of 1/16 below 2 (exact in bf16), x 8 on the pattern; padding stays zero
    g0 = torch.Generator().manual_seed(7)
    w0 = torch.zeros(n)
    for s in f.slots:
        w0[s.offset:s.offset + s.numel] = ((torch.rand(s.numel, generator=g0) * 30).round() + 1) / 16
    w0 *= torch.where(e == 2.0, 8.0, 1.0)
    f.data.copy_(w0.to(dev))
    mine = torch.cat([torch.arange(lo, hi) for lo, hi, _ in _flat_segments(ps, rank)])
    assert mine.numel() == opt.w.numel()
    opt.w.copy_(w0[mine].to(dev))
    for s in range(steps):
        ps.begin_step(overlap=False)
        f.grad.copy_(_grad(s, rank, n, e).to(dev))
        ps.step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    # whole tensors: the flat buffer's slots (padding with the slot before it); pieces: every rank's segments as
    # tensors of their own
    whole_segs = [(s.offset, nxt, i) for i, (s, nxt) in
                  enumerate(zip(f.slots, [t.offset for t in f.slots[1:]] + [n]))]
    adapt = [_adapt(s.name, p) for s, p in zip(f.slots, f.params)]
    piece_segs, piece_adapt = [], []
    for r in range(world):
        for lo, hi, t in _flat_segments(ps, r):
            piece_segs.append((lo, hi, len(piece_adapt)))
            piece_adapt.append(adapt[t])
    cut = len(piece_segs) - len(whole_segs)  # tensors cut by a piece boundary
    ref, wrong = _reference(cfg, w0, whole_segs, adapt, nw), _reference(cfg, w0, piece_segs, piece_adapt, nw)
    norms = []
    for s in range(steps):
        tot = sum(_grad(s, w, n, e) for w in range(nw))
        ref.step(tot)
        wrong.step(tot)
        norms.append(ref.norm)
    master = opt.w.double().cpu()
    ratios, ref_ratios = opt.ratios().double().cpu(), torch.tensor(ref.ratios, dtype=torch.float64)
    # the variables and the ratio table go back as their bits (bytes pickle by value: a tensor on a queue is handed
    # over through a descriptor that the sending process must outlive)
    res = {"flat": _bits(f.data), "table": _bits(opt.table), "cut_tensors": cut, "ref_norms": norms,
           "has_cut_tensor": cut >= 3,
           "master_err": (master - ref.w[mine]).abs().max().item(),
           "master_match": bool(torch.allclose(master, ref.w[mine], **VS_TORCH)),
           "ratio_err": (ratios - ref_ratios).abs().max().item(),
           "ratios_match": bool(torch.allclose(ratios, ref_ratios, **VS_TORCH)),
           "wrong_err": (master - wrong.w[mine]).abs().max().item(),
           "refs_err": (ref.w - wrong.w).abs().max().item(),
           "piece_reference_differs": not torch.allclose(master, wrong.w[mine], **FAR),
           "moved": bool((ref.w - w0.double()).abs().max() > 0.05),
           "variables_are_the_rounded_masters": bool(torch.equal(f.data[mine.to(dev)].cpu(), opt.w.to(dtype).cpu())),
           "padding_stays_zero": bool(all((f.data[s.offset + s.numel:nxt] == 0).all() for s, nxt in zip(
               f.slots, [t.offset for t in f.slots[1:]] + [n])))}
    if "clip_norm" in cfg:
        res["clipped_some_steps"] = any(x > cfg["clip_norm"] for x in norms) and \
            not all(x > cfg["clip_norm"] for x in norms)
        res["skipped_none"] = opt.skipped_steps() == 0
    return res


def body(rank, world, dev, dtype, names=("lars", "lamb", "lamb-clip")):
    return {name: one(name, rank, world, dev, dtype) for name in names}


def cpu_rank(rank, world, port, names=("lars", "lamb", "lamb-clip")):
    """tests/test_dist_cpu.py's pattern: a pool task per rank, fp32 variables over gloo."""
    from dist_workers import _init

    _init(rank, world, port)
    try:
        return body(rank, world, torch.device("cpu"), torch.float32, names)
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
