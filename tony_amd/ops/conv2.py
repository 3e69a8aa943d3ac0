"""32 -> 64 conv + bias + ReLU + 2x2 max-pool of the MNIST CNNs (HIP kernels in csrc/conv2.hip).

``conv2_bias_relu_pool(x, weight, bias, padding)`` is
``max_pool2d(relu(conv2d(x, weight, bias, padding=padding)), 2)``, the second layer of ``deepnn`` and ``hvd_cnn``.
The kernels take this form::

    x [N, 32, H, W], weight [64, 32, k, k], bias [64]: contiguous fp32 on one GPU, N >= 1
    k in {3, 5}, stride 1, dilation 1, padding 0 or (k - 1) / 2
    OH = H + 2p - k + 1 >= 2, OW = W + 2p - k + 1 >= 2, W + 2p <= 64, N * 64 * OH * OW < 2^31
    x may or may not require grad (dX is computed only when it does)

Anything else -- a CPU tensor, another dtype, layout, channel count, padding, a wider plane -- is served by exactly
that torch composition, the calls the models made before this op existed.  On a GPU a tensor of the form above never
takes that path: a missing kernel library is an error (``_lib.lib``).

Forward is one launch (``tony_conv2_fwd``) that writes the pooled ``y`` and a uint8 ``idx``, the window position 0..3
of each maximum (the first one in row-major order, torch's rule); an odd ``OH`` or ``OW`` is pooled with floor and
the last conv row or column is never computed.  The full-resolution activation is never written.  Backward expands
``(dy, y, idx)`` in LDS -- ``dy`` at position ``idx`` unless ``y <= 0``, zero elsewhere, so the gradient at
``relu == 0`` is 0 -- in ``tony_conv2_dgrad`` (only if ``x`` requires grad) and ``tony_conv2_wgrad``, whose partials
``tony_conv2_fold`` adds in index order.  No atomics: the same inputs give the same bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

CIN, COUT = 32, 64
KERNEL_SIZES = (3, 5)
MAX_PLANE_W = 64


def _native(x, weight, bias, padding) -> bool:
    if not (x.is_cuda and x.dim() == 4 and weight.dim() == 4 and bias.dim() == 1):
        return False
    k = weight.shape[-1]
    if (x.shape[1] != CIN or tuple(weight.shape) != (COUT, CIN, k, k) or k not in KERNEL_SIZES
            or bias.shape[0] != COUT or not isinstance(padding, int) or padding not in (0, (k - 1) // 2)):
        return False
    if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device for t in (x, weight, bias)):
        return False
    n, _, h, w = x.shape
    oh, ow = h + 2 * padding - k + 1, w + 2 * padding - k + 1
    return n >= 1 and oh >= 2 and ow >= 2 and w + 2 * padding <= MAX_PLANE_W and n * COUT * oh * ow < 2 ** 31


def _forward(x, weight, bias, padding):
    """The pooled ``y`` and its ``idx`` from ``tony_conv2_fwd`` (``x`` of the native form)."""
    n, _, h, w = x.shape
    k = weight.shape[-1]
    shape = (n, COUT, (h + 2 * padding - k + 1) // 2, (w + 2 * padding - k + 1) // 2)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    idx = torch.empty(shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().tony_conv2_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), idx.data_ptr(),
                                       n, h, w, k, padding, _lib.stream_ptr(x.device))
    _lib.check(rc, "tony_conv2_fwd")
    return y, idx


class _Conv2BiasReLUPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, padding):
        y, idx = _forward(x, weight, bias, padding)
        ctx.save_for_backward(x, weight, y, idx)
        ctx.padding = padding
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y, idx = ctx.saved_tensors
        k, padding = weight.shape[-1], ctx.padding
        n, _, h, w = x.shape
        dy = dy.contiguous()
        L = _lib.lib()
        dx = dw = db = None
        with torch.cuda.device(x.device):
            stream = _lib.stream_ptr(x.device)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(L.tony_conv2_dgrad(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), weight.data_ptr(),
                                              dx.data_ptr(), n, h, w, k, padding, stream), "tony_conv2_dgrad")
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                grid = L.tony_conv2_wgrad_grid(n)
                partials = torch.empty(grid * (k * k * COUT * CIN + COUT), dtype=torch.float32, device=x.device)
                dw = torch.empty_like(weight)
                db = torch.empty(COUT, dtype=torch.float32, device=x.device)
                _lib.check(L.tony_conv2_wgrad(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), x.data_ptr(),
                                              partials.data_ptr(), n, h, w, k, padding, stream), "tony_conv2_wgrad")
                _lib.check(L.tony_conv2_fold(partials.data_ptr(), grid, k, dw.data_ptr(), db.data_ptr(), stream),
                           "tony_conv2_fold")
        return dx, dw, db, None


def conv2_bias_relu_pool(x, weight, bias, padding: int = 0):
    """``max_pool2d(relu(conv2d(x, weight, bias, padding=padding)), 2)``: the HIP kernels for the form in the module
    docstring, the torch composition itself for everything else."""
    if _native(x, weight, bias, padding):
        return _Conv2BiasReLUPool.apply(x, weight, bias, padding)
    return F.max_pool2d(F.relu(F.conv2d(x, weight, bias, padding=padding)), 2)


class Conv2BiasReLUPool(nn.Module):
    """``nn.Conv2d(32, 64, kernel_size, padding=padding)``, ReLU and ``nn.MaxPool2d(2)`` as one op; ``weight`` and
    ``bias`` have ``nn.Conv2d``'s names, shapes and initial values (they ARE those of an ``nn.Conv2d`` built here, or
    of ``conv``)."""

    def __init__(self, kernel_size: int = 3, padding: int = 0, conv: nn.Conv2d = None):
        super().__init__()
        if conv is None:
            conv = nn.Conv2d(CIN, COUT, kernel_size, padding=padding)
        if not isinstance(conv, nn.Conv2d) or (conv.in_channels, conv.out_channels, conv.stride, conv.dilation,
                                                conv.groups) != (CIN, COUT, (1, 1), (1, 1), 1) or conv.bias is None or conv.kernel_size[0] != conv.kernel_size[1] \
                or conv.padding[0] != conv.padding[1] or not isinstance(conv.padding[0], int) \
                or conv.padding_mode != "zeros":
            raise ValueError(f"Conv2BiasReLUPool replaces Conv2d({CIN}, {COUT}, k, padding=p) with a bias, got {conv}")
        self.kernel_size, self.padding = conv.kernel_size[0], conv.padding[0]
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x):
        return conv2_bias_relu_pool(x, self.weight, self.bias, self.padding)

    def extra_repr(self) -> str:
        return f"{CIN}, {COUT}, kernel_size={self.kernel_size}, padding={self.padding}"
