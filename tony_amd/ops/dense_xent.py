"""The MNIST networks' classifier head as one op: ``cross_entropy(linear(x, weight, bias), labels)`` in one forward and
one backward launch (HIP kernels in csrc/dense_xent.hip).

``dense_xent(x, weight, bias, labels, reduction="mean", return_logits=False)`` means exactly
``ops.cross_entropy(ops.dense.dense(x, weight, bias), labels, reduction=reduction)``: per-row fp32 losses, a label
outside ``[0, N)`` marks an ignored row (loss 0, zero gradient row), and ``"mean"`` divides by all ``M`` rows.  The
kernels take this form::

    x [M, K], weight [N, K], bias [N]: contiguous fp32 on one GPU, x and weight 16-byte aligned
    labels [M]: contiguous int64 on that GPU
    1 <= N <= 32, K >= 4 and K % 4 == 0, M >= 1, M * K < 2^31

Anything else -- CPU tensors, another dtype, ``N > 32``, ``K % 4 != 0``, no bias, a non-contiguous or misaligned
tensor, an active autocast -- is served by that composition itself.  On a GPU a call of the form above never takes it:
a missing kernel library is an error (``_lib.lib``).

Forward is ``tony_dense_xent_fwd``: it stores the logits, their row log-sum-exp and the per-row losses, and saves
``(x, weight, labels, logits, lse)``.  Backward is ``tony_dense_xent_bwd``: it rebuilds the logit gradient from the
saved logits and ``lse`` on its way into LDS and forms ``dx`` (only if ``x`` requires grad), ``dw`` and ``db`` from it in
the same launch; first order only (``once_differentiable``).  The logits are returned (``return_logits=True``) as a
non-differentiable output, for accuracy counters.  No atomics: the same inputs give the same bits.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .dense import _native as _dense_native
from .dense import dense
from .loss import cross_entropy

MAX_CLASSES = 32  # csrc/dense_xent.hip kTile: the classes are the columns of one accumulator tile


def _native(x, weight, bias, labels) -> bool:
    if not _dense_native(x, weight, bias) or weight.shape[0] > MAX_CLASSES:
        return False
    return (labels.dtype == torch.int64 and labels.device == x.device and labels.dim() == 1
            and labels.shape[0] == x.shape[0] and labels.is_contiguous())


class _DenseXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels):
        (m, k), n = x.shape, weight.shape[0]
        L = _lib.lib()
        logits = torch.empty((m, n), dtype=torch.float32, device=x.device)
        lse, loss = (torch.empty(m, dtype=torch.float32, device=x.device) for _ in range(2))
        with torch.cuda.device(x.device):
            _lib.check(L.tony_dense_xent_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), labels.data_ptr(),
                                             logits.data_ptr(), lse.data_ptr(), loss.data_ptr(), m, n, k,
                                             _lib.stream_ptr(x.device)), "tony_dense_xent_fwd")
        ctx.save_for_backward(x, weight, labels, logits, lse)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, _dlogits):
        x, weight, labels, logits, lse = ctx.saved_tensors
        (m, k), n = x.shape, weight.shape[0]
        # the gradient of a sum or a mean is one value expanded over the rows: the kernel reads it with stride 0
        gs = gout.stride(0) if m > 1 else 1
        if gout.dtype != torch.float32 or gs not in (0, 1):
            gout, gs = gout.float().contiguous(), 1
        L = _lib.lib()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight)
        db = torch.empty(n, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.tony_dense_xent_bwd(gout.data_ptr(), gs, logits.data_ptr(), lse.data_ptr(), labels.data_ptr(),
                                             x.data_ptr(), weight.data_ptr(), None if dx is None else dx.data_ptr(),
                                             dw.data_ptr(), db.data_ptr(), m, n, k, _lib.stream_ptr(x.device)),
                       "tony_dense_xent_bwd")
        return dx, dw, db, None


def dense_xent(x, weight, bias, labels, reduction: str = "mean", return_logits: bool = False):
    """``ops.cross_entropy(ops.dense.dense(x, weight, bias), labels, reduction=reduction)``: one HIP launch each way
    for the form in the module docstring, that composition itself for everything else.  With ``return_logits`` the
    result is ``(loss, logits)``, the logits detached."""
    if _native(x, weight, bias, labels):
        per_row, logits = _DenseXent.apply(x, weight, bias, labels)
        loss = per_row.mean() if reduction == "mean" else per_row.sum() if reduction == "sum" else per_row
    else:
        logits = dense(x, weight, bias)
        loss = cross_entropy(logits, labels, reduction=reduction)
        logits = logits.detach()
    return (loss, logits) if return_logits else loss
