"""Rank body for tests/test_optim_plane_gpu.py: the dedicated synchronous PS over the xGMI data plane
(csrc/ps_plane.hip) applying Adagrad / TF-style RMSProp, every rank a process as in tests/ps_plane_worker.py."""
import os

import torch
import torch.distributed as dist

import gpu_ranks
from ps_plane_worker import _Net, _master_flat


def _grad(step, widx, idx):
    """ps_plane_worker.run's schedule: multiples of 1/8 (exact in bf16, and so is their fp32 sum over workers)."""
    return float((widx + 1) * (step % 3 + 1)) * 0.25 + idx.remainder(4) * 0.125


def run(rank, world, port, q, kind, wire=None, steps=4):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dev, _ = gpu_ranks.init(rank, world)
        from tony_amd.parallel.ps import ParameterServer, make_optimizer

        torch.manual_seed(0)
        net = _Net([11000, 12000, 4136, 13000, 3000, 11008, 64])
        with torch.no_grad():
            for p in net.ps:
                p.copy_(torch.randn(p.shape).mul_(0.5))
        lr, momentum = 0.1, 0.9
        ps = ParameterServer(net, optimizer=kind, lr=lr, momentum=momentum, mode="dedicated", sync=True,
                             ps_ranks=(0,), dtype=torch.bfloat16, device=dev, bucket_mb=0.02, wire_dtype=wire,
                             plane="xgmi")
        assert ps.plane is not None and len(ps.buckets) > 3
        n = ps.flat.numel
        w0 = ps.flat.data.float().cpu().clone()
        idx = torch.arange(n, dtype=torch.float32)
        nw = len(ps.worker_ranks)
        for s in range(steps):
            if ps.is_worker:
                ps.begin_step(overlap=False)
                ps.flat.grad.copy_(_grad(s, ps.worker_ranks.index(rank), idx).to(dev))
            ps.step()
        torch.cuda.synchronize()
        ps.plane.check_error()
        # the same schedule on the CPU class: each step the workers' gradients summed in worker order, x 1/nw
        ref = make_optimizer(kind, w0.clone(), lr, momentum)
        ref.grad_scale = 1.0 / nw
        for s in range(steps):
            tot = torch.zeros(n)
            for w in range(nw):
                tot += _grad(s, w, idx)
            ref.step(tot)
        res = {}
        got = ps.flat.data.float().cpu()
        exp = ref.w.to(torch.bfloat16).float()
        res["params_err"] = (got - exp).abs().max().item()
        res["params_match"] = bool(torch.allclose(got, exp, rtol=1e-2, atol=2e-2))
        res["params_moved"] = bool((ref.w - w0).abs().min() > 0.05)
        if ps.is_ps:
            master = _master_flat(ps)
            res["master_err"] = (master - ref.w).abs().max().item()
            res["master_match"] = bool(torch.allclose(master, ref.w, rtol=1e-5, atol=1e-4))
        res["pushed"] = ps.plane.pushed
        ps.plane.close()
        q.put((rank, res))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, {"error": f"{e!r}\n{traceback.format_exc()}"}))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
