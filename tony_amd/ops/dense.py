"""fp32 Linear + bias (+ ReLU) of the MNIST dense layers (HIP kernels in csrc/dense.hip).

``dense(x, weight, bias, relu=False)`` is ``F.linear(x, weight, bias)``, wrapped in ``F.relu`` when ``relu`` is set.
The kernels take this form::

    x [M, K], weight [N, K], bias [N]: contiguous fp32 on one GPU, x and weight 16-byte aligned
    M, N >= 1, K >= 4 and K % 4 == 0, M * K, N * K, M * N < 2^31
    x may or may not require grad (dx is computed only when it does)

Anything else -- a CPU tensor, another dtype, a non-contiguous or misaligned tensor, ``K % 4 != 0``, no bias,
``x.dim() != 2``, an active autocast (under which ``F.linear`` computes in the autocast dtype) -- is served by exactly
that torch composition, the calls the models made before this op existed.  On a GPU a tensor of the form above never
takes that path: a missing kernel library is an error (``_lib.lib``).  The kernels' backward is first order only
(``once_differentiable``): a double backward through the native path raises, where the composition supports it.

Forward is ``tony_dense_fwd``; where the shape's long K is cut into ``S = tony_dense_splits(M, N, K) > 1`` slices it
writes ``S`` partial products and ``tony_dense_fold`` adds them in index order, adds the bias and applies ReLU.  The
forward saves ``(x, weight, y)``: ``not y <= 0`` is ReLU's backward mask, applied in ``tony_dense_dgrad`` (only if ``x``
requires grad) and ``tony_dense_wgrad`` (``dw`` and ``db``) while ``dy`` is staged.  No atomics: the same inputs give
the same bits.  ``ops.linear`` (bf16, with its fp32 vendor path for the image models' heads) is a different op and is
untouched.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib


def _native(x, weight, bias) -> bool:
    if bias is None or torch.is_autocast_enabled():
        return False
    if not (x.is_cuda and x.dim() == 2 and weight.dim() == 2 and bias.dim() == 1):
        return False
    if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device for t in (x, weight, bias)):
        return False
    (m, k), n = x.shape, weight.shape[0]
    if weight.shape[1] != k or bias.shape[0] != n or m < 1 or n < 1 or k < 4 or k % 4:
        return False
    if x.data_ptr() % 16 or weight.data_ptr() % 16:
        return False
    return max(m * k, n * k, m * n) < 2 ** 31


def _forward(x, weight, bias, relu):
    """``y`` from ``tony_dense_fwd`` (and ``tony_dense_fold`` when K is split) for tensors of the native form."""
    (m, k), n = x.shape, weight.shape[0]
    L = _lib.lib()
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    splits = L.tony_dense_splits(m, n, k)
    partials = torch.empty(splits * m * n, dtype=torch.float32, device=x.device) if splits > 1 else None
    with torch.cuda.device(x.device):
        stream = _lib.stream_ptr(x.device)
        _lib.check(L.tony_dense_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                    partials.data_ptr() if splits > 1 else None, m, n, k, int(relu), stream),
                   "tony_dense_fwd")
        if splits > 1:
            _lib.check(L.tony_dense_fold(partials.data_ptr(), bias.data_ptr(), y.data_ptr(), splits, m, n, int(relu),
                                         stream), "tony_dense_fold")
    return y


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        y = _forward(x, weight, bias, relu)
        ctx.save_for_backward(x, weight, y)
        ctx.relu = relu
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        (m, k), n, relu = x.shape, weight.shape[0], int(ctx.relu)
        dy = dy.contiguous()
        L = _lib.lib()
        dx = dw = db = None
        with torch.cuda.device(x.device):
            stream = _lib.stream_ptr(x.device)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(L.tony_dense_dgrad(dy.data_ptr(), y.data_ptr(), weight.data_ptr(), dx.data_ptr(), m, n, k,
                                              relu, stream), "tony_dense_dgrad")
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                dw = torch.empty_like(weight)
                db = torch.empty(n, dtype=torch.float32, device=x.device)
                _lib.check(L.tony_dense_wgrad(dy.data_ptr(), y.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                              m, n, k, relu, stream), "tony_dense_wgrad")
        return dx, dw, db, None


def dense(x, weight, bias, relu: bool = False):
    """``F.linear(x, weight, bias)``, in ``F.relu`` when ``relu``: the HIP kernels for the form in the module docstring,
    the torch composition itself for everything else."""
    if _native(x, weight, bias):
        return _Dense.apply(x, weight, bias, bool(relu))
    y = F.linear(x, weight, bias)
    return F.relu(y) if relu else y


class Dense(nn.Module):
    """``nn.Linear(in_features, out_features)`` and, with ``relu``, the ``nn.ReLU`` after it as one op; ``weight`` and
    ``bias`` have ``nn.Linear``'s names, shapes and initial values (they ARE those of an ``nn.Linear`` built here, or
    of ``linear``)."""

    def __init__(self, in_features: int = None, out_features: int = None, relu: bool = False, linear: nn.Linear = None):
        super().__init__()
        if linear is None:
            linear = nn.Linear(in_features, out_features)
        if not isinstance(linear, nn.Linear) or linear.bias is None:
            raise ValueError(f"Dense replaces an nn.Linear with a bias, got {linear}")
        self.in_features, self.out_features, self.relu = linear.in_features, linear.out_features, bool(relu)
        self.weight, self.bias = linear.weight, linear.bias

    def forward(self, x):
        return dense(x, self.weight, self.bias, self.relu)

    def extra_repr(self) -> str:
        return f"{self.in_features}, {self.out_features}, relu={self.relu}"
