"""Rank body of the multi-precision kvstore's server test (test_kv_mp_gpu.py): one dist_sync round of a dense bf16 key
on the GPU plane; the server reports its optimizer's launch counters."""
import os

import numpy as np
import torch

N = 2053


def push_of(rank):
    """Worker ``rank``'s pushed gradient, fp32 values exactly representable in bf16."""
    g = np.random.default_rng(50 + rank).standard_normal(N).astype(np.float32)
    return (g.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def key0():
    return (np.random.default_rng(49).standard_normal(N).astype(np.float32).view(np.uint32)
            & np.uint32(0xFFFF0000)).view(np.float32)


def kv_mp_rank(role, index, num_workers, port, name, cfg):
    os.environ.update(DMLC_ROLE=role, DMLC_NUM_SERVER="1", DMLC_NUM_WORKER=str(num_workers),
                      DMLC_PS_ROOT_URI="127.0.0.1", DMLC_PS_ROOT_PORT=str(port), TASK_INDEX=str(index))
    import tony_amd.kv as kv

    if role == "server":
        stats = {}
        kv.run_server(stats=stats)
        return {"role": role, **stats}
    if kv.run_role():
        return {"role": role}
    dev = torch.device("cuda", 0)
    store = kv.create("dist_sync")
    store.init("d", torch.from_numpy(key0()).to(dev).bfloat16())
    store.set_optimizer(kv.create_optimizer(name, multi_precision=True, **cfg))
    store.push("d", torch.from_numpy(push_of(store.rank)).to(dev).bfloat16())
    out = torch.zeros(N, dtype=torch.bfloat16, device=dev)
    store.pull("d", out=out)
    res = {"role": role, "rank": store.rank, "plane_ops": list(store.plane_ops),
           "pulled": out.view(torch.int16).cpu().numpy().view(np.uint16)}
    store.close()
    return res
