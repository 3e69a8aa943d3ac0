"""Rank bodies of the kvstore fused-optimizer tests (test_kv_optim_cpu.py, test_kv_optim_gpu.py): a dist_sync store
with one dense and one row-sparse key under one of the fused kinds, and the prediction of what its workers see from
the numpy contract (kv_optim_ref.py).  The sparse pushes and pulls are those of kv_sparse_workers.py."""
import os

import numpy as np
import torch

import kv_optim_ref as ref
import kv_sparse_ref as sref
import kv_sparse_workers as SW

NW = SW.NW


def dense0(N):
    return np.random.default_rng(4321).standard_normal(N).astype(np.float32)


def dense_grad(rank, step, N):
    return np.random.default_rng(77 + 10 * step + rank).standard_normal(N).astype(np.float32)


def predict(name, cfg, steps, R, D, N):
    """``(seen, dense, table)``: ``seen[step]`` the (dense value, table) every worker pulls from after the round of
    ``step`` -- the workers' pushes merged in worker order (one fp32 add each), then the update -- and the finals."""
    table, dense = SW.table0(R, D, False), dense0(N)
    ts, ds, seen = {}, {}, []
    for s in range(steps):
        g = dense_grad(0, s, N)
        for r in range(1, NW):
            g = (g + dense_grad(r, s, N)).astype(np.float32)
        dense, ds, _ = ref.step(name, dense, ds, None, g, **cfg)
        ids, rows = sref.merge([sref.merge(SW.pushes_of(r, s, R, D, False)) for r in range(NW)])
        table, ts, _ = ref.step(name, table, ts, ids, rows, **cfg)
        seen.append((dense.copy(), table.copy()))
    return seen, dense, table


def kv_opt_rank(role, index, num_servers, num_workers, port, kind, device, name, cfg, steps, R, D, N):
    """A scheduler / server / worker of a ``kind`` store with the sparse key "emb" [R, D] and the dense key "d" [N]
    under optimizer ``name``: every step push both, pull the dense value and row_sparse_pull the step's ids."""
    os.environ.update(DMLC_ROLE=role, DMLC_NUM_SERVER=str(num_servers), DMLC_NUM_WORKER=str(num_workers),
                      DMLC_PS_ROOT_URI="127.0.0.1", DMLC_PS_ROOT_PORT=str(port), TASK_INDEX=str(index))
    if device == "cpu":
        os.environ["TONY_KV_PLANE"] = "gloo"
    import tony_amd.kv as kv

    if kv.run_role():
        return {"role": role}
    store = kv.create(kind)
    shape = (R, D)
    store.init("emb", SW._rsp(kv, (np.arange(R, dtype=np.int64), SW.table0(R, D, False)), shape, device))
    store.init("d", torch.from_numpy(dense0(N)).to(device))
    store.set_optimizer(kv.create_optimizer(name, **cfg))
    rank = store.rank
    out = kv.RowSparse(torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, D, device=device), shape)
    d = torch.zeros(N, device=device)
    seen = []
    for s in range(steps):
        store.push("d", torch.from_numpy(dense_grad(rank, s, N)).to(device))
        store.push("emb", [SW._rsp(kv, p, shape, device) for p in SW.pushes_of(rank, s, R, D, False)])
        store.pull("d", out=d)
        store.row_sparse_pull("emb", out=out, row_ids=torch.from_numpy(SW.pull_ids(rank, s, R)).to(device))
        seen.append((d.cpu().numpy().copy(), out.indices.cpu().numpy().copy(), out.data.cpu().numpy().copy()))
    store.barrier()
    final = torch.zeros(R, D, device=device)
    store.pull("emb", out=final, ignore_sparse=False)
    store.pull("d", out=d)
    res = {"role": role, "rank": rank, "seen": seen, "table": final.cpu().numpy(), "dense": d.cpu().numpy(),
           "sparse_ops": list(store.sparse_ops), "plane_ops": list(store.plane_ops)}
    store.close()
    return res
