"""Top-1 / top-k evaluation counters (HIP kernel in csrc/metrics.hip).

``tf.math.in_top_k``'s semantics: a row is a top-k hit iff its target logit is finite and fewer than ``k``
classes have a strictly greater logit (ties that straddle the boundary all count).  The three int64 counters
``[hit@1, hit@k, rows]`` live on the device and are only read by ``result()``: ``update`` never synchronises.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib


def topk_count(logits: torch.Tensor, targets: torch.Tensor, k: int, counters: torch.Tensor) -> None:
    """``counters += [hit@1, hit@k, rows]`` for the ``[rows, classes]`` bf16 / fp32 ``logits`` (unit column
    stride, any row stride) and the integer ``targets``."""
    if logits.dim() != 2 or targets.dim() != 1 or targets.numel() != logits.shape[0]:
        raise ValueError(f"logits [rows, classes] and targets [rows], got {tuple(logits.shape)} / "
                         f"{tuple(targets.shape)}")
    if counters.dtype != torch.int64 or counters.numel() != 3 or not counters.is_contiguous() \
            or counters.device != logits.device:
        raise ValueError("counters must be 3 contiguous int64 on the logits' device")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"top-k takes bf16 / fp32 logits, got {logits.dtype}")
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    rows, classes = logits.shape
    if rows == 0:
        return
    if logits.stride(1) != 1 or logits.stride(0) < classes:
        logits = logits.contiguous()
    targets = targets.to(device=logits.device, dtype=torch.int64).contiguous()
    if not logits.is_cuda:
        x = logits.float()
        valid = (targets >= 0) & (targets < classes)
        xt = x.gather(1, targets.clamp(0, classes - 1)[:, None])
        greater = (x > xt).sum(1)
        ok = valid & torch.isfinite(xt[:, 0])
        counters += torch.stack([(ok & (greater < 1)).sum(), (ok & (greater < k)).sum(), torch.tensor(rows)])
        return
    rc = _lib.lib().tony_topk_count(logits.data_ptr(), int(logits.dtype == torch.bfloat16), rows, classes,
                                    logits.stride(0), targets.data_ptr(), int(k), counters.data_ptr(),
                                    _lib.stream_ptr(logits.device))
    _lib.check(rc, "tony_topk_count")


class TopK:
    """Running top-1 / top-k accuracy: ``update(logits, targets)`` per batch, ``result()`` once at the end."""

    def __init__(self, k: int = 5, device="cpu"):
        self.k = int(k)
        self.counters = torch.zeros(3, dtype=torch.int64, device=device)  # [hit@1, hit@k, rows]: all-reduce these

    def update(self, logits: torch.Tensor, targets: torch.Tensor) -> None:
        topk_count(logits, targets, self.k, self.counters)

    def result(self) -> Tuple[float, float, int]:
        """(top-1 accuracy, top-k accuracy, rows seen); the one host synchronisation."""
        h1, hk, seen = (int(v) for v in self.counters.tolist())
        return (h1 / seen if seen else 0.0, hk / seen if seen else 0.0, seen)

    def reset(self) -> None:
        self.counters.zero_()
