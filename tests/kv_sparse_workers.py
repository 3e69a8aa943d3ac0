"""Rank bodies of the kvstore row-sparse tests (test_kv_sparse_cpu.py, test_kv_sparse_gpu.py): importable by
spawned processes, each returns a picklable result; and the prediction of what they see from the numpy reference."""
import os

import numpy as np
import torch

import kv_sparse_ref as ref

NW = 2  # workers of every dist case here


def table0(R, D, exact):
    """The sparse key's initial value (every worker passes the same)."""
    rng = np.random.default_rng(1234)
    if exact:
        return rng.integers(-4, 5, (R, D)).astype(np.float32)
    return rng.standard_normal((R, D)).astype(np.float32)


def _rows(seed, n, D, exact):
    rng = np.random.default_rng(seed)
    if exact:  # small integers: with power-of-two hyper-parameters every operation of the update is exact
        return rng.integers(-8, 9, (n, D)).astype(np.float32)
    return (rng.standard_normal((n, D)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)


def pushes_of(rank, step, R, D, exact):
    """The list of (ids, rows) worker ``rank`` pushes at ``step``: step 0 overlapping row sets (worker 0's own list
    overlaps too), step 1 disjoint ones, step 2 an empty push from worker 1, step 3 every row from worker 1 (more
    than its window row holds beside the ids)."""
    sets = [
        [[[0, 3, 5, R - 1], [3, 4]], [[3, 5, 7]]],
        [[[1, 2]], [[8, 9, R - 1]]],
        [[[0, 4, R - 1]], [[]]],
        [[[2]], [list(range(R))]],
    ][step][rank]
    return [(np.asarray(ids, np.int64), _rows(1000 * step + 100 * rank + j, len(ids), D, exact))
            for j, ids in enumerate(sets)]


def pull_ids(rank, step, R):
    """Unsorted row ids with duplicates, rows 0 and R - 1 among them."""
    return np.asarray([R - 1, 3, 0, 3, (5 + rank + step) % R, R - 1], np.int64).reshape(2, 3)


def _apply(w, m, opt, ids, rows, tol):
    if opt is None:
        return ref.assign(w.shape, ids, rows), m
    w, m, bw, _ = ref.sgd(w, m, ids, rows, lr=opt["learning_rate"], momentum=opt.get("momentum", 0.0),
                          wd=opt.get("wd", 0.0), rescale=opt.get("rescale_grad", 1.0),
                          clip=opt.get("clip_gradient"))
    tol[ids] += bw
    return w, m


def predict(kind, opt, steps, exact, R, D):
    """``(seen, final, tol)``: ``seen[step][rank]`` the table worker ``rank`` pulls rows of at ``step``, the final
    table and the summed per-step bounds of the reference's SGD (kv_sparse_ref.py).  dist_async runs its workers one
    after the other (``kv_rsp_rank``): each push is applied on its own, in rank order."""
    w = table0(R, D, exact)
    m = np.zeros_like(w) if opt and opt.get("momentum") else None
    tol = np.zeros((R, D), np.float64)
    seen = []
    for s in range(steps):
        per_worker = [ref.merge(pushes_of(r, s, R, D, exact)) for r in range(NW)]
        if kind == "dist_async":
            now = []
            for ids, rows in per_worker:
                w, m = _apply(w, m, opt, ids, rows, tol)
                now.append(w.copy())
        else:
            ids, rows = ref.merge(per_worker)
            w, m = _apply(w, m, opt, ids, rows, tol)
            now = [w.copy()] * NW
        seen.append(now)
    return seen, w, tol


def _rsp(kv, pair, shape, device):
    ids, rows = pair
    return kv.RowSparse(torch.from_numpy(ids).to(device), torch.from_numpy(rows).to(device), shape)


def kv_rsp_rank(role, index, num_servers, num_workers, port, kind, device, opt, steps, exact, R, D):
    """A scheduler / server / worker of a dist_sync or dist_async store with the sparse key "emb" [R, D] and the
    dense key "d".  Every step: push the step's list, row_sparse_pull unsorted duplicate ids.  Under dist_async the
    workers take turns (push, pull, barrier), so that the order the server applies their pushes in is known."""
    os.environ.update(DMLC_ROLE=role, DMLC_NUM_SERVER=str(num_servers), DMLC_NUM_WORKER=str(num_workers),
                      DMLC_PS_ROOT_URI="127.0.0.1", DMLC_PS_ROOT_PORT=str(port), TASK_INDEX=str(index))
    if device == "cpu":
        os.environ["TONY_KV_PLANE"] = "gloo"
    import tony_amd.kv as kv

    if kv.run_role():
        return {"role": role}
    store = kv.create(kind)
    shape = (R, D)
    store.init("emb", _rsp(kv, (np.arange(R, dtype=np.int64), table0(R, D, exact)), shape, device))
    store.init("d", torch.zeros(3, device=device))
    if opt is not None:
        store.set_optimizer(kv.create_optimizer("sgd", **opt))
    rank = store.rank
    out = kv.RowSparse(torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, D, device=device), shape)
    seen = []

    def step_of(s):
        store.push("emb", [_rsp(kv, p, shape, device) for p in pushes_of(rank, s, R, D, exact)])
        store.row_sparse_pull("emb", out=out, row_ids=torch.from_numpy(pull_ids(rank, s, R)).to(device))
        seen.append((out.indices.cpu().numpy().copy(), out.data.cpu().numpy().copy()))

    for s in range(steps):
        if kind == "dist_async":
            for turn in range(num_workers):
                if turn == rank:
                    step_of(s)
                store.barrier()
        else:
            step_of(s)
    errors = {}
    for name, call in (("dense_to_sparse", lambda: store.push("emb", torch.zeros(R, D, device=device))),
                       ("sparse_to_dense", lambda: store.push("d", _rsp(kv, pushes_of(0, 1, R, D, exact)[0], shape,
                                                                        device))),
                       ("out_of_range", lambda: store.row_sparse_pull(
                           "emb", out=out, row_ids=torch.tensor([0, R], device=device)))):
        try:
            call()
            errors[name] = None
        except Exception as e:  # noqa: BLE001 - the test names the type it expects
            errors[name] = type(e).__name__
    store.barrier()  # every worker's last pull is answered: the value is final
    skipped = torch.full((R, D), 7.0, device=device)
    store.pull("emb", out=skipped)  # ignore_sparse defaults to True: untouched
    final = torch.full((R, D), 7.0, device=device)
    store.pull("emb", out=final, ignore_sparse=False)
    dense = torch.full((3,), 7.0, device=device)
    store.pull("d", out=dense, ignore_sparse=True)
    res = {"role": role, "rank": rank, "seen": seen, "errors": errors, "final": final.cpu().numpy(),
           "skipped": skipped.cpu().numpy(), "dense": dense.cpu().tolist(), "sparse_ops": list(store.sparse_ops),
           "plane_ops": list(store.plane_ops)}
    store.close()
    return res


def device_sync_rank(rank, world, port, q, device, opt, steps, exact, R, D):
    """A rank of a ``dist_device_sync`` store pushing the same lists as ``kv_rsp_rank``: gloo on the CPU, the test
    box's placement (tests/gpu_ranks.py) on the GPU."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        import torch.distributed as dist

        if device == "cpu":
            dist.init_process_group("gloo", rank=rank, world_size=world)
            dev = torch.device("cpu")
        else:
            import gpu_ranks

            dev, _ = gpu_ranks.init(rank, world)
        import tony_amd.kv as kv

        store = kv.create("dist_device_sync")
        shape = (R, D)
        store.init("emb", _rsp(kv, (np.arange(R, dtype=np.int64), table0(R, D, exact)), shape, dev))
        if opt is not None:
            store.set_optimizer(kv.create_optimizer("sgd", **opt))
        out = kv.RowSparse(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, D, device=dev), shape)
        seen = []
        for s in range(steps):
            store.push("emb", [_rsp(kv, p, shape, dev) for p in pushes_of(rank, s, R, D, exact)])
            store.row_sparse_pull("emb", out=out, row_ids=torch.from_numpy(pull_ids(rank, s, R)).to(dev))
            seen.append((out.indices.cpu().numpy().copy(), out.data.cpu().numpy().copy()))
        final = torch.zeros(R, D, device=dev)
        store.pull("emb", out=final, ignore_sparse=False)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, {"seen": seen, "final": final.cpu().numpy()}))
    except Exception as e:  # noqa: BLE001 - reported to the parent, which fails the test
        import traceback

        q.put((rank, {"error": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))
