"""Sparse logistic regression through the kvstore's row-sparse keys under TonY's mxnet runtime (the shape of
MXNet's ``sparse/linear_classification`` example: a wide table, a few active features per sample).

The model is one ``[F, D]`` table held by the servers as a sparse key.  A sample has ``--active`` feature ids; its
logit is the sum of their rows projected on a fixed vector.  Every step a worker pulls only the rows its batch
touches (``row_sparse_pull``), runs forward and backward on them in torch, and pushes only their gradients
(``RowSparse.from_rows`` sums the rows of a feature that occurs more than once); the servers update only those rows.
Roles follow DMLC_ROLE as in mxnet_linreg.py.

  tony --src_dir tony_amd/jobs --executes mxnet_sparse_linear.py --conf tony.application.framework=mxnet \
       --conf tony.scheduler.instances=1 --conf tony.server.instances=1 --conf tony.worker.instances=2 \
       [--task_params "--kvstore dist_sync"]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import tony_amd.kv as kv  # noqa: E402
from tony_amd.jobs.common import Throughput, log, metric  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kvstore", default="dist_async")
    ap.add_argument("--features", type=int, default=100000, help="F: rows of the table")
    ap.add_argument("--dim", type=int, default=16, help="D: elements of a row")
    ap.add_argument("--active", type=int, default=8, help="active features of a sample")
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--optimizer", choices=["sgd", "adam", "adagrad", "ftrl"], default="sgd",
                    help="the servers' (lazy) update of the touched rows")
    ap.add_argument("--device", choices=["auto", "cpu", "cuda"], default="auto")
    a = ap.parse_args(argv)
    if kv.run_role():  # scheduler / server: serve until the workers are done
        return 0
    dev = torch.device("cuda" if a.device == "cuda" or (a.device == "auto" and torch.cuda.is_available()) else "cpu")
    store = kv.create(a.kvstore)
    rank, nw = store.rank, store.num_workers
    F, D = a.features, a.dim
    g = torch.Generator().manual_seed(0)
    feats = torch.randint(0, F, (a.samples, a.active), generator=g)
    truth = torch.randn(F, generator=g)                      # the hidden per-feature weight the labels come from
    labels = (truth[feats].sum(1) > 0).float()
    proj = torch.randn(D, generator=g) / D ** 0.5            # fixed: every column of a row takes part
    shard = slice(rank * a.samples // nw, (rank + 1) * a.samples // nw)
    feats, labels, proj = feats[shard].to(dev), labels[shard].to(dev), proj.to(dev)
    shape = (F, D)
    store.init("table", kv.RowSparse(torch.zeros(0, dtype=torch.int64), torch.zeros(0, D), shape))  # all zero
    store.set_optimizer(kv.create_optimizer(a.optimizer, learning_rate=a.lr, rescale_grad=1.0 / nw))
    extra = {} if a.optimizer == "sgd" else {"optimizer": a.optimizer}  # (the default's output stays as it was)
    if extra:
        log(f"worker {rank}/{nw}: optimizer {a.optimizer}, lr {a.lr}")
    rows = kv.RowSparse(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, D, device=dev), shape)
    rate = Throughput(dev)
    first = last = None
    for epoch in range(a.epochs):
        rate.start()
        total, seen = 0.0, 0
        for lo in range(0, feats.shape[0], a.batch_size):
            fb, yb = feats[lo:lo + a.batch_size], labels[lo:lo + a.batch_size]
            store.row_sparse_pull("table", out=rows, row_ids=fb)
            pos = torch.searchsorted(rows.indices, fb.reshape(-1))         # each occurrence's pulled row
            occ = rows.data.index_select(0, pos).requires_grad_()
            logit = occ.view(fb.shape[0], a.active, D).sum(1) @ proj
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, yb, reduction="sum")
            loss.backward()
            store.push("table", kv.RowSparse.from_rows(fb.reshape(-1), occ.grad, shape))
            total += float(loss)
            seen += fb.shape[0]
            rate.add(fb.shape[0])
        last = total / max(1, seen)
        first = last if first is None else first
        metric(epoch=epoch, loss=last, samples_per_s=rate.rate(), rank=rank, **extra)
    store.barrier()  # every worker's last push is applied (its round closed, or its pull answered) before the read
    store.row_sparse_pull("table", out=rows, row_ids=feats[:1])
    table = torch.empty(shape, device=dev)
    store.pull("table", out=table, ignore_sparse=False)
    digest = hashlib.sha256(table.cpu().numpy().tobytes()).hexdigest()
    metric(final=1, table_sha256=digest, first_loss=first, loss=last, rank=rank, **extra)
    log(f"worker {rank}/{nw}: loss {first:.4f} -> {last:.4f}, table {digest[:12]}")
    store.close()
    return 0 if last < first else 1


if __name__ == "__main__":
    sys.exit(main())
