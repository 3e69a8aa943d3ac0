"""Single-channel first-layer conv + bias + ReLU (+ 2x2 max-pool) of the MNIST CNNs (HIP kernels in csrc/conv1.hip and
csrc/conv1_pool.hip).

``conv1_bias_relu(x, weight, bias, padding)`` is ``relu(conv2d(x, weight, bias, padding=padding))`` for the layer
``deepnn``, ``keras_cnn`` and ``hvd_cnn`` open with.  The kernels take this form::

    x [N, 1, H, W], weight [32, 1, k, k], bias [32]: contiguous fp32 on one GPU, N >= 1
    k in {3, 5}, stride 1, dilation 1, padding 0 or (k - 1) / 2, H >= k, W >= k, N * OH * OW < 2^31
    x does not require grad (it is the image: the layer has no data gradient)

Anything else -- a CPU tensor, another dtype, layout, shape or padding, an ``x`` that requires grad -- is served by
exactly ``F.relu(F.conv2d(x, weight, bias, padding=padding))``, the calls the models made before this op existed.
On a GPU a tensor of the form above never takes that path: a missing kernel library is an error (``_lib.lib``).

Forward is one launch (``tony_conv1_fwd``); backward is two (``tony_conv1_bwd`` stores one 32x32 partial of
``[dW | db]`` per workgroup, ``tony_conv1_fold`` adds them in index order).  The gradient at ``y == 0`` is 0, torch's
convention.  No atomics: the same inputs give the same bits.

``pool=True`` is ``max_pool2d(relu(conv2d(...)), 2)``, ``deepnn``'s opening: the same form with ``OH, OW >= 2``, and
anything else is exactly that torch composition.  Forward is one launch (``tony_conv1_pool_fwd``) that writes the
pooled ``y`` and a uint8 ``idx``, the window position 0..3 of each maximum (the first one in row-major order, torch's
rule); an odd ``OH`` or ``OW`` is pooled with floor and the last conv row or column is never computed.  Backward is
``tony_conv1_pool_bwd`` over ``(dy, y, idx, x)`` and the same ``tony_conv1_fold``.  Neither the full-resolution
activation nor its gradient is ever written.  With ``pool=False`` nothing differs from what is described above.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

COUT = 32
KERNEL_SIZES = (3, 5)


def _native(x, weight, bias, padding) -> bool:
    if not (x.is_cuda and x.dim() == 4 and weight.dim() == 4 and bias.dim() == 1) or x.requires_grad:
        return False
    k = weight.shape[-1]
    if (x.shape[1] != 1 or tuple(weight.shape) != (COUT, 1, k, k) or k not in KERNEL_SIZES or bias.shape[0] != COUT
            or not isinstance(padding, int) or padding not in (0, (k - 1) // 2)):
        return False
    if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device for t in (x, weight, bias)):
        return False
    n, _, h, w = x.shape
    return n >= 1 and h >= k and w >= k and n * (h + 2 * padding - k + 1) * (w + 2 * padding - k + 1) < 2 ** 31


class _Conv1BiasReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, padding):
        n, _, h, w = x.shape
        k = weight.shape[-1]
        y = torch.empty(n, COUT, h + 2 * padding - k + 1, w + 2 * padding - k + 1, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = _lib.lib().tony_conv1_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, k,
                                           padding, _lib.stream_ptr(x.device))
        _lib.check(rc, "tony_conv1_fwd")
        ctx.save_for_backward(x, y)
        ctx.geom = (k, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        k, padding = ctx.geom
        n, _, h, w = x.shape
        dy = dy.contiguous()
        L = _lib.lib()
        grid = L.tony_conv1_bwd_grid(n)
        partials = torch.empty(grid * COUT * 32, dtype=torch.float32, device=x.device)
        dw = torch.empty(COUT, 1, k, k, dtype=torch.float32, device=x.device)
        db = torch.empty(COUT, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            stream = _lib.stream_ptr(x.device)
            _lib.check(L.tony_conv1_bwd(dy.data_ptr(), y.data_ptr(), x.data_ptr(), partials.data_ptr(), n, h, w, k,
                                        padding, stream), "tony_conv1_bwd")
            _lib.check(L.tony_conv1_fold(partials.data_ptr(), grid, k, dw.data_ptr(), db.data_ptr(), stream),
                       "tony_conv1_fold")
        return None, dw, db, None


def _native_pool(x, weight, bias, padding) -> bool:
    if not _native(x, weight, bias, padding):
        return False
    k = weight.shape[-1]
    return x.shape[2] + 2 * padding - k + 1 >= 2 and x.shape[3] + 2 * padding - k + 1 >= 2


def _forward_pool(x, weight, bias, padding):
    """The pooled ``y`` and its ``idx`` from ``tony_conv1_pool_fwd`` (``x`` of the native form)."""
    n, _, h, w = x.shape
    k = weight.shape[-1]
    shape = (n, COUT, (h + 2 * padding - k + 1) // 2, (w + 2 * padding - k + 1) // 2)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    idx = torch.empty(shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().tony_conv1_pool_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                            idx.data_ptr(), n, h, w, k, padding, _lib.stream_ptr(x.device))
    _lib.check(rc, "tony_conv1_pool_fwd")
    return y, idx


class _Conv1BiasReLUPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, padding):
        y, idx = _forward_pool(x, weight, bias, padding)
        ctx.save_for_backward(x, y, idx)
        ctx.geom = (weight.shape[-1], padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, idx = ctx.saved_tensors
        k, padding = ctx.geom
        n, _, h, w = x.shape
        dy = dy.contiguous()
        L = _lib.lib()
        grid = L.tony_conv1_pool_bwd_grid(n)
        partials = torch.empty(grid * COUT * 32, dtype=torch.float32, device=x.device)
        dw = torch.empty(COUT, 1, k, k, dtype=torch.float32, device=x.device)
        db = torch.empty(COUT, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            stream = _lib.stream_ptr(x.device)
            _lib.check(L.tony_conv1_pool_bwd(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), x.data_ptr(),
                                             partials.data_ptr(), n, h, w, k, padding, stream), "tony_conv1_pool_bwd")
            _lib.check(L.tony_conv1_fold(partials.data_ptr(), grid, k, dw.data_ptr(), db.data_ptr(), stream),
                       "tony_conv1_fold")
        return None, dw, db, None


def conv1_bias_relu(x, weight, bias, padding: int = 0, pool: bool = False):
    """``relu(conv2d(x, weight, bias, padding=padding))``, under ``max_pool2d(., 2)`` with ``pool``: the HIP kernels for
    the form in the module docstring, the torch composition itself for everything else."""
    if pool:
        if _native_pool(x, weight, bias, padding):
            return _Conv1BiasReLUPool.apply(x, weight, bias, padding)
        return F.max_pool2d(F.relu(F.conv2d(x, weight, bias, padding=padding)), 2)
    if _native(x, weight, bias, padding):
        return _Conv1BiasReLU.apply(x, weight, bias, padding)
    return F.relu(F.conv2d(x, weight, bias, padding=padding))


class Conv1BiasReLU(nn.Module):
    """``nn.Conv2d(1, 32, kernel_size, padding=padding)`` followed by ReLU (and by ``nn.MaxPool2d(2)`` with ``pool``) as
    one op; ``weight`` and ``bias`` have ``nn.Conv2d``'s names, shapes and initial values (they ARE those of an
    ``nn.Conv2d`` built here, or of ``conv``)."""

    def __init__(self, kernel_size: int = 3, padding: int = 0, conv: nn.Conv2d = None, pool: bool = False):
        super().__init__()
        if conv is None:
            conv = nn.Conv2d(1, COUT, kernel_size, padding=padding)
        if (conv.in_channels, conv.out_channels, conv.stride, conv.dilation, conv.groups) != (1, COUT, (1, 1), (1, 1), 1) \
                or conv.bias is None or conv.kernel_size[0] != conv.kernel_size[1] or conv.padding[0] != conv.padding[1] \
                or not isinstance(conv.padding[0], int) or conv.padding_mode != "zeros":
            raise ValueError(f"Conv1BiasReLU replaces Conv2d(1, {COUT}, k, padding=p) with a bias, got {conv}")
        self.kernel_size, self.padding, self.pool = conv.kernel_size[0], conv.padding[0], pool
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x):
        return conv1_bias_relu(x, self.weight, self.bias, self.padding, self.pool)

    def extra_repr(self) -> str:
        s = f"1, {COUT}, kernel_size={self.kernel_size}, padding={self.padding}"
        return s + ", pool=True" if self.pool else s
