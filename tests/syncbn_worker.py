"""Rank bodies of the synchronised-BatchNorm tests: tests/test_syncbn_cpu.py (a pool task per rank, gloo, CPU tensors)
and tests/test_syncbn_ranks_gpu.py (a process per rank, placed by tests/gpu_ranks.py, the result on a queue).

``op_body`` runs ``sync_bn_act`` forward and backward on this rank's rows of a ``syncbn_cases.case``; ``model_body``
trains one step of a small converted stack (one ``ConvBNAct``, one ``Bottleneck`` with downsample) on this rank's
slice of a batch; ``hvd_body`` runs ``hvd.SyncBatchNorm``.  Everything goes back as numpy arrays: the parent holds the
references and does the comparing."""
import os

import numpy as np
import torch
import torch.distributed as dist

import syncbn_cases as K

OP_CASES = {2: [(8, (5, 3)), (24, (343, 90))], 3: [(8, (5, 3, 9)), (24, (300, 1, 343))]}
# the model: rank r holds BATCH[world][r] images of 8 channels, 4 x 4
BATCH = {1: (6,), 2: (4, 2), 3: (3, 2, 1)}
CIN, WIDTH, HW = 8, 8, 4


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def op_body(rank, dev, C, slices, res, relu, dtype):
    from tony_amd.ops.syncbn import sync_bn_act

    c = K.case(C, slices, res, relu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)  # noqa: E731
    x = t(c["xs"][rank]).requires_grad_(True)
    r = t(c["ress"][rank]).requires_grad_(True) if res else None
    g = torch.nn.Parameter(torch.from_numpy(c["g"]).float().to(dev))
    b = torch.nn.Parameter(torch.from_numpy(c["b"]).float().to(dev))
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = sync_bn_act(x, g, b, rm, rv, True, K.MOM, K.EPS, relu, r, None)
    saved = [s for s in y.grad_fn.saved_tensors[3:5]]  # save_mean, save_invstd
    y.backward(t(c["dys"][rank]))
    return dict(y=_np(y), dx=_np(x.grad), dres=_np(r.grad) if res else None, dgamma=_np(g.grad), dbeta=_np(b.grad),
                rm=_np(rm), rv=_np(rv), save_mean=_np(saved[0]), save_invstd=_np(saved[1]))


def make_model(dtype, dev, seed=3):
    """The stack, unconverted: ConvBNAct(8 -> 16, 3x3) + Bottleneck(16 -> 8 x 4 = 32, downsample)."""
    from tony_amd.models.layers import ConvBNAct, cast_model
    from tony_amd.models.resnet import Bottleneck

    torch.manual_seed(seed)
    m = torch.nn.Sequential(ConvBNAct(CIN, 16, 3, padding=1, eps=1e-5), Bottleneck(16, WIDTH))
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):  # bf16-representable, away from the trivial 1 / 0
                mod.weight.copy_(torch.randint(4, 13, mod.weight.shape) / 8.0)
                mod.bias.copy_(torch.randint(-8, 9, mod.bias.shape) / 16.0)
    return cast_model(m, dtype, dev).to(memory_format=torch.channels_last).train()


def model_inputs(world):
    """The full batch: images of rank r offset by 2 r (clearly different statistics per rank), and the loss weights."""
    n = sum(BATCH[world])
    rng = np.random.default_rng(17)
    x = rng.integers(-2, 3, (n, CIN, HW, HW)).astype(np.float64)
    x += np.repeat(2.0 * np.arange(world), BATCH[world])[:, None, None, None]
    t = rng.integers(-2, 3, (n, 4 * WIDTH, HW, HW)).astype(np.float64) / 4
    return x, t


def bn_layers(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def model_body(rank, world, dev, dtype):
    """One forward + backward of the converted stack on this rank's slice: loss = sum(out * t)."""
    from tony_amd.models.syncbn import SyncBottleneck, SyncConvBNAct, convert_sync_batchnorm
    from tony_amd.ops.syncbn import SyncBatchNormAct2d

    model = convert_sync_batchnorm(make_model(dtype, dev))
    assert isinstance(model[0], SyncConvBNAct) and isinstance(model[1], SyncBottleneck)
    assert all(isinstance(m, SyncBatchNormAct2d) for m in bn_layers(model))
    x, t = model_inputs(world)
    lo = sum(BATCH[world][:rank])
    hi = lo + BATCH[world][rank]
    cl = lambda a: torch.from_numpy(a).to(dtype).to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    xr = cl(x[lo:hi]).requires_grad_(True)
    out = model(xr)
    (out.double() * cl(t[lo:hi]).double()).sum().backward()
    bns = bn_layers(model)
    return dict(out=_np(out), dx=_np(xr.grad), dgamma=[_np(m.weight.grad) for m in bns],
                dbeta=[_np(m.bias.grad) for m in bns], rm=[m.running_mean.cpu().numpy().tobytes() for m in bns],
                rv=[m.running_var.cpu().numpy().tobytes() for m in bns])


def hvd_body(rank, world, dev, hvd):
    """``hvd.SyncBatchNorm`` (affine and not) on this rank's rows of a case; the saved statistics as bytes."""
    C, slices = OP_CASES[world][0]
    c = K.case(C, slices, False, False)
    res = {}
    for affine in (True, False):
        bn = hvd.SyncBatchNorm(C, eps=K.EPS, momentum=K.MOM, affine=affine).to(dev)
        x = torch.from_numpy(c["xs"][rank]).float().to(dev).view(-1, C, 1, 1).requires_grad_(True)
        y = bn(x)
        saved = y.grad_fn.saved_tensors[3:5]
        y.backward(torch.from_numpy(c["dys"][rank]).float().to(dev).view(-1, C, 1, 1))
        res[affine] = dict(y=_np(y).reshape(-1, C), dx=_np(x.grad).reshape(-1, C),
                           stats=b"".join(s.cpu().numpy().tobytes() for s in saved)
                           + bn.running_mean.cpu().numpy().tobytes() + bn.running_var.cpu().numpy().tobytes(),
                           has_params=bn.weight is not None, relu=bn.relu)
    return res


def recording_raises(dev):
    """Inside ``tape.recording()`` with more than one rank the op must raise, naming eager mode."""
    from tony_amd.ops import tape
    from tony_amd.ops.syncbn import sync_bn_act

    x = torch.zeros(4, 8, device=dev)
    prev = tape._active[0]
    tape._active[0] = tape.Tape(x, ())
    try:
        sync_bn_act(x, None, None, None, None, True, 0.1, 1e-5, False)
        return "no error"
    except RuntimeError as e:
        return f"RuntimeError: {e}"
    finally:
        tape._active[0] = prev


def cpu_rank(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TONY_DIST_BACKEND="gloo")
    torch.set_num_threads(1)
    import tony_amd.hvd as hvd

    hvd.init()
    try:
        dev = torch.device("cpu")
        out = {"op": {}}
        for C, slices in OP_CASES[world]:
            for res, relu in ((False, True), (True, True), (False, False)):
                for dt in (torch.float32, torch.bfloat16):
                    key = (C, slices, res, relu, dt == torch.bfloat16)
                    out["op"][key] = op_body(rank, dev, C, slices, res, relu, dt)
        out["model"] = model_body(rank, world, dev, torch.float32)
        out["hvd"] = hvd_body(rank, world, dev, hvd)
        out["recording"] = recording_raises(dev)
        return out
    finally:
        hvd.shutdown()


def gpu_rank(rank, world, port, q):
    import gpu_ranks

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dev, _ = gpu_ranks.init(rank, world)
        import tony_amd.hvd as hvd

        hvd.init()
        out = {"op": {}}
        C, slices = OP_CASES[world][1]
        for res in (False, True):
            for dt in (torch.float32, torch.bfloat16):
                out["op"][(C, slices, res, True, dt == torch.bfloat16)] = op_body(rank, dev, C, slices, res, True, dt)
        out["model"] = {"bf16": model_body(rank, world, dev, torch.bfloat16),
                        "fp32": model_body(rank, world, dev, torch.float32)}
        out["hvd"] = hvd_body(rank, world, dev, hvd)
        out["recording"] = recording_raises(dev)
        torch.cuda.synchronize()
        q.put((rank, out))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, {"error": f"{e!r}\n{traceback.format_exc()}"}))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
