"""Shared plumbing of the reference jobs: device choice, synthetic data, metric lines, checkpoint dir."""
from __future__ import annotations

import json
import os
import sys
import time

import torch


def log(msg: str) -> None:
    print(f"[{os.environ.get('JOB_NAME', 'job')}:{os.environ.get('TASK_INDEX', '0')}] {msg}", flush=True)


def metric(**kv) -> None:
    """One machine-readable line per report (the training-metrics side channel)."""
    print("TONY_METRIC " + json.dumps(kv, sort_keys=True), flush=True)


def working_dir(default: str = "model") -> str:
    """Where checkpoints go: $TONY_WORKING_DIR, else <job dir>/<default> (shared by every task and
    by every session of a retried job, so a relaunched gang resumes), else ./<default>."""
    if os.environ.get("TONY_WORKING_DIR"):
        return os.environ["TONY_WORKING_DIR"]
    return os.path.join(os.environ.get("TONY_JOB_DIR", os.getcwd()), default)


class Throughput:
    def __init__(self, device: torch.device):
        self.device = device
        self.t0 = None
        self.n = 0

    def start(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.t0 = time.perf_counter()
        self.n = 0

    def add(self, items: int):
        self.n += items

    def rate(self) -> float:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - self.t0
        return self.n / dt if dt > 0 else 0.0


def synthetic_images(n: int, res: int, classes: int, device, dtype=torch.bfloat16, seed: int = 0):
    """Device-side RNG fill of an NHWC ImageNet-shaped batch."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, 3, res, res, device=device, generator=g).to(dtype).contiguous(
        memory_format=torch.channels_last)
    y = torch.randint(0, classes, (n,), device=device, generator=g)
    return x, y


def evaluate(model, eval_dir: str, batch: int, size: int, kind: str, device, dtype, rank: int, world: int):
    """Top-1 / top-5 counters ``[hit@1, hit@5, images]`` (int64, on ``device``) of ``model`` in eval mode over
    this rank's share of the shards in ``eval_dir`` (central crop, file order); the caller all-reduces them."""
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.metrics import TopK

    top = TopK(5, device)
    was_training = model.training
    model.eval()
    try:
        with ImageBatches(eval_dir, batch, size, train=False, model=kind, device=device, dtype=dtype, rank=rank,
                          world=world) as batches, torch.no_grad():
            for x, y in batches:
                out = model(x)
                top.update(out[0] if isinstance(out, tuple) else out, y)
    finally:
        model.train(was_training)
    return top.counters


def exit_code(ok: bool) -> None:
    sys.exit(0 if ok else 1)


def poly_warmup_lr(step: int, base_lr: float, warmup_steps: int, total_steps: int, power: float = 2.0,
                   end_lr: float = 0.0) -> float:
    """The LARS schedule: a linear warm-up to ``base_lr`` over ``warmup_steps`` steps (step 0 gets
    ``base_lr / warmup_steps``), then polynomial decay to ``end_lr`` at ``total_steps``, where it stays."""
    if warmup_steps < 0 or total_steps < warmup_steps:
        raise ValueError(f"need 0 <= warmup_steps <= total_steps, got {warmup_steps} and {total_steps}")
    if step < warmup_steps:
        return base_lr * (step + 1) / warmup_steps
    if step >= total_steps:
        return end_lr
    left = 1.0 - (step - warmup_steps) / (total_steps - warmup_steps)
    return end_lr + (base_lr - end_lr) * left ** power
