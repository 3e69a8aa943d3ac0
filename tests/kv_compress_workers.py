"""Rank bodies of the kvstore gradient-compression tests (test_kv_compress_cpu.py, test_kv_compress_gpu.py):
importable by spawned processes, each returns a picklable result."""
import os

import numpy as np
import torch

import kv_compress_ref as ref

LR, HALF_N = 0.5, 5  # sgd lr (a power of two, like rescale 1/2: the update is exact whether or not it is fused)


def grad_of(rank, step, key_index, n, thr, extra=False):
    """The gradient worker ``rank`` pushes for a key at a step (``extra``: its second push of that step)."""
    return ref.gradient(n, thr, seed=10000 * rank + 100 * step + 10 * key_index + int(extra), with_specials=False)


def kv_gc_rank(role, index, num_servers, num_workers, port, kind, steps, device, thr, big_n, extra_step=None):
    """A scheduler / server / worker of a dist_sync or dist_async store with 2-bit compression: fp32 keys "a"
    (3 elements) and "big" (``big_n``) and the bf16 key "h".  At ``extra_step`` a worker pushes "big" twice
    before pulling it (the second push finds the key's window row possibly unread).  That step's order --
    push big, push a, pull a, push big -- keeps dist_sync's rounds well defined: the reply to the pull of "a"
    follows both workers' pushes of "a", each of which follows that worker's first push of "big" on its
    connection, so the round of the first pushes has closed before either second push arrives."""
    os.environ.update(DMLC_ROLE=role, DMLC_NUM_SERVER=str(num_servers), DMLC_NUM_WORKER=str(num_workers),
                      DMLC_PS_ROOT_URI="127.0.0.1", DMLC_PS_ROOT_PORT=str(port), TASK_INDEX=str(index))
    if device == "cpu":
        os.environ["TONY_KV_PLANE"] = "gloo"
    import tony_amd.kv as kv

    if kv.run_role():
        return {"role": role}
    store = kv.create(kind)
    a = torch.zeros(3, device=device)
    big = torch.zeros(big_n, device=device)
    h = torch.zeros(HALF_N, dtype=torch.bfloat16, device=device)
    store.init("a", a)
    store.init("big", big)
    store.init("h", h)
    store.set_optimizer(kv.create_optimizer("sgd", learning_rate=LR, rescale_grad=1.0 / num_workers))
    store.set_gradient_compression({"type": "2bit", "threshold": thr})
    rank = store.rank

    def g(step, key_index, n, extra=False):
        return torch.from_numpy(grad_of(rank, step, key_index, n, thr, extra)).to(device)

    seen = []
    for s in range(steps):
        if s == extra_step:
            store.push("big", g(s, 1, big_n))
            store.push("a", g(s, 0, 3))
            store.pull("a", out=a)
            store.push("big", g(s, 1, big_n, extra=True))
        else:
            store.push("a", g(s, 0, 3))
            store.push("big", g(s, 1, big_n))
            store.pull("a", out=a)
        store.push("h", torch.full((HALF_N,), float(rank + 1), dtype=torch.bfloat16, device=device))
        store.pull("big", out=big)
        store.pull("h", out=h)
        seen.append({"a": a.cpu().numpy().copy(), "big": big.cpu().numpy().copy(), "h": h.float().cpu().tolist()})
    try:
        store.set_gradient_compression({"type": "none"})
        late = None
    except Exception as e:  # noqa: BLE001 - the test names the type it expects
        late = type(e).__name__
    res = {"role": role, "rank": rank, "seen": seen, "late": late, "compressed_ops": list(store.compressed_ops),
           "plane_ops": list(store.plane_ops)}
    store.close()
    return res


def device_sync_rank(rank, world, port, q, thr, n, steps):
    """A rank of a ``dist_device_sync`` store with 2-bit compression on the GPU (tests/gpu_ranks.py)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        import gpu_ranks

        dev, _ = gpu_ranks.init(rank, world)
        import torch.distributed as dist

        import tony_amd.kv as kv

        store = kv.create("dist_device_sync")
        w = torch.zeros(n, device=dev)
        store.init("w", w)
        store.set_optimizer(kv.create_optimizer("sgd", learning_rate=LR, rescale_grad=1.0 / world))
        store.set_gradient_compression({"type": "2bit", "threshold": thr})
        seen = []
        for s in range(steps):
            store.push("w", torch.from_numpy(grad_of(rank, s, 0, n, thr)).to(dev))
            store.pull("w", out=w)
            seen.append(w.cpu().numpy().copy())
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, {"seen": seen}))
    except Exception as e:  # noqa: BLE001 - reported to the parent, which fails the test
        import traceback

        q.put((rank, {"error": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))


def predict(steps, num_workers, thr, sizes, extra_step=None):
    """What every worker pulls after each step of ``kv_gc_rank`` under dist_sync, per fp32 key, from the
    reference: ``{key: [value after step 0, ...]}``; and the final values of dist_async (the same sums)."""
    out = {}
    for key_index, (key, n) in enumerate(sizes):
        w = np.zeros(n, np.float32)
        res = [np.zeros(n, np.float32) for _ in range(num_workers)]
        vals = []
        for s in range(steps):
            for extra in ([False, True] if (s == extra_step and key == "big") else [False]):
                words = []
                for r in range(num_workers):
                    wd, res[r] = ref.quantise(grad_of(r, s, key_index, n, thr, extra), res[r], thr)
                    words.append(wd)
                w = ref.sgd_update(w, ref.merge(words, n, thr), LR, 1.0 / num_workers)
            vals.append(w)
        out[key] = vals
    return out
