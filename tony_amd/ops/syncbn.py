"""Synchronised BatchNorm (+ReLU, + residual add): the statistics of ALL ranks' batches (csrc/syncbn.hip).

``sync_bn_act(x, weight, bias, running_mean, running_var, training, momentum, eps, relu, res=None, group=None)``
is ``bn_act`` (``res``: the bottleneck tail ``relu(bn(x) + res)``) whose batch statistics are taken over the
batches of every rank of ``group``.  tests/syncbn_ref.py is this contract in numpy.

Activations are NHWC rows ``[M_r, C]`` on rank ``r`` of ``W`` with row stride ``ld``; ``C % 8 == 0``, ``C <= 2048``;
bf16 and fp32; ``M_r >= 1`` may differ between ranks; ``N = sum_r M_r``.

Forward, training
  * Rank ``r`` builds a float64 packet ``[M_r | S_r[C] | Q_r[C]]``, ``S = sum x``, ``Q = sum x * x``: every element is
    converted exactly to double and accumulated in double (a bf16 or fp32 square is exact there, so the sums are
    good to ``n * 2^-53`` and carry no fp32 cancellation).  No float atomics: the grid is a function of ``(M, C)``
    only, each workgroup stores its partial, and the partials are folded in ascending workgroup order -- two runs
    give the same bits.
  * The ranks all-gather the packets: ``[W, 1 + 2C]`` float64, at most 32 KB per rank
    (parallel/collectives.py ``all_gather_packets``).
  * Every rank computes in double, summing ranks in ascending order: ``mean = S / N``,
    ``var = max(Q / N - mean^2, 0)``, ``invstd = 1 / sqrt(var + eps)``.  ``save_mean`` / ``save_invstd`` are these
    rounded once to fp32; the running statistics are updated in fp32 as ``bn_fwd_apply_kernel`` does, with the
    unbiased ``var * N / (N - 1)`` for ``N > 1``.  Every rank reads the same gathered bytes, so ``save_*`` and
    ``running_*`` are bit-identical on all ranks.
  * The row pass is ``y = act(fma(x, g * invstd, b - mean * g * invstd) [+ res])`` with fp32 coefficients, rounded
    once to the output type.

Backward
  * ``dy'`` is ``dy`` masked by the ReLU: the plain form recomputes the mask from ``x`` with the forward's fp32
    coefficients, the ``res`` form takes it from the saved ``y <= 0``.  ``xhat = fma(x, invstd, -mean * invstd)`` in
    fp32.
  * Rank ``r`` folds ``A_r = sum dy'`` and ``B_r = sum dy' * xhat`` in double, by the same stored-partials scheme.
    ``dbeta = A_r`` and ``dgamma = B_r`` are the LOCAL sums, as in torch's SyncBatchNorm (the gradient all-reduce
    that follows averages them); they are written, or accumulated into the parameter's gradient slot
    (``_lib.grad_slot``), fp32 or bf16, rounded once.
  * The ranks all-gather ``[A_r | B_r]``; ``dx = g * invstd * (dy' - A / N - xhat * B / N)`` with the sums over the
    ranks, folded into three fp32 coefficients per channel as ``bn_bwd_apply_kernel`` does.  The ``res`` form also
    returns ``dres = dy'``.

Evaluation uses the running statistics and is exactly ``bn_act`` / ``bn_add_relu``.  One rank, or no process group,
runs the same kernels with no exchange.  With more than one rank inside ``tape.recording()`` or a stream capture
the call raises ``RuntimeError``: the statistics exchange cannot be part of a captured step, use eager mode.
``momentum=None`` (cumulative averaging) raises ``ValueError``.

CUDA bf16 / fp32 tensors whose layout the kernels take run on the HIP kernels; CPU tensors and any other dtype or
layout take a torch composition of the same contract (float64 packets, the same gather).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib, tape
from .bn import BatchNormAct2d, _as_rows, _empty_like_rows, _rows_view, bn_act

_KERNEL_DTYPES = (torch.bfloat16, torch.float32)
MAX_C = 2048


def _world(group) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _gather(packet, group):
    from ..parallel.collectives import all_gather_packets

    return all_gather_packets(packet, group)


def _f64(n, dev):
    return torch.empty(n, dtype=torch.float64, device=dev)


def _f32(n, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


class _SyncBNActFn(torch.autograd.Function):
    """Training forward / backward on the HIP kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, res, group):
        L = _lib.lib()
        _lib.check_f32_stats(running_mean, running_var)
        x, (M, C, ldx) = _as_rows(x)
        dev = x.device
        f32 = int(x.dtype == torch.float32)
        y = _empty_like_rows(x)
        _, _, ldy = _rows_view(y)
        ldr = 0
        if res is not None:
            res, (_, _, ldr) = _as_rows(res)
        pb = int(weight is not None and weight.dtype == torch.bfloat16)
        stream = _lib.stream_ptr(dev)
        G = L.tony_syncbn_grid(M, C)
        if G < 1:
            raise _lib.KernelError(f"tony_syncbn_grid({M}, {C}) = {G}")
        partials, packet = _f64(G * 2 * C, dev), _f64(1 + 2 * C, dev)
        _lib.check(L.tony_syncbn_stats(x.data_ptr(), M, C, ldx, f32, partials.data_ptr(), stream), "tony_syncbn_stats")
        _lib.check(L.tony_syncbn_fold(partials.data_ptr(), G, C, packet.data_ptr(), M, stream), "tony_syncbn_fold")
        gathered = _gather(packet, group)
        mean, invstd, coef, count = _f32(C, dev), _f32(C, dev), _f32(2 * C, dev), _f64(1, dev)
        rc = L.tony_syncbn_merge(gathered.data_ptr(), gathered.shape[0], C, _lib.ptr(weight), _lib.ptr(bias), pb,
                                 float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                                 _lib.ptr(running_mean), _lib.ptr(running_var), coef.data_ptr(), count.data_ptr(),
                                 stream)
        _lib.check(rc, "tony_syncbn_merge")
        rc = L.tony_syncbn_apply(x.data_ptr(), M, C, ldx, _lib.ptr(res), ldr, y.data_ptr(), ldy, f32, coef.data_ptr(),
                                 int(relu), stream)
        _lib.check(rc, "tony_syncbn_apply")
        ctx.save_for_backward(x, weight, bias, mean, invstd, count, y if res is not None else None)
        ctx.params = (weight, bias)
        ctx.relu, ctx.pb, ctx.f32, ctx.group, ctx.grid = relu, pb, f32, group, G
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, weight, bias, mean, invstd, count, y = ctx.saved_tensors
        M, C, ldx = _rows_view(x)
        dev = x.device
        stream = _lib.stream_ptr(dev)
        dy, (_, _, lddy) = _as_rows(dy)
        dx = _empty_like_rows(x)
        _, _, lddx = _rows_view(dx)
        ldy = _rows_view(y)[2] if y is not None else 0
        dres, lddr = None, 0
        if y is not None and ctx.needs_input_grad[8]:
            dres = _empty_like_rows(x)
            lddr = _rows_view(dres)[2]
        gw, gb = _lib.grad_slot(ctx.params[0]), _lib.grad_slot(ctx.params[1])
        inplace = gw is not None and gb is not None
        if inplace:
            dw, db = gw, gb
        else:
            dw = torch.empty_like(weight) if weight is not None else None
            db = torch.empty_like(bias) if bias is not None else None
        partials, ab = _f64(ctx.grid * 2 * C, dev), _f64(2 * C, dev)  # (the forward's grid: a function of M, C)
        rc = L.tony_syncbn_bwd_reduce(x.data_ptr(), ldx, dy.data_ptr(), lddy, _lib.ptr(y), ldy, M, C, ctx.f32,
                                      mean.data_ptr(), invstd.data_ptr(), _lib.ptr(weight), _lib.ptr(bias), ctx.pb,
                                      int(ctx.relu), partials.data_ptr(), ab.data_ptr(), _lib.ptr(dw), _lib.ptr(db),
                                      int(inplace), stream)
        _lib.check(rc, "tony_syncbn_bwd_reduce")
        gathered = _gather(ab, ctx.group)
        tab = _f32(5 * C, dev)
        rc = L.tony_syncbn_bwd_merge(gathered.data_ptr(), gathered.shape[0], C, count.data_ptr(), mean.data_ptr(),
                                     invstd.data_ptr(), _lib.ptr(weight), _lib.ptr(bias), ctx.pb, tab.data_ptr(),
                                     stream)
        _lib.check(rc, "tony_syncbn_bwd_merge")
        rc = L.tony_syncbn_bwd_apply(x.data_ptr(), ldx, dy.data_ptr(), lddy, _lib.ptr(y), ldy, _lib.ptr(dres), lddr,
                                     dx.data_ptr(), lddx, M, C, ctx.f32, tab.data_ptr(), int(ctx.relu), stream)
        _lib.check(rc, "tony_syncbn_bwd_apply")
        if inplace:
            dw = db = None  # already added into param.grad
        _lib.report_inplace(ctx.params, (dw, db))
        return dx, dw, db, None, None, None, None, None, dres, None


def _channel_rows(t):
    """[N, C, *] -> float64 rows [M, C] (any layout)."""
    return t.detach().movedim(1, -1).reshape(-1, t.shape[1]).double()


def _from_rows(rows, like):
    shape = (like.shape[0],) + tuple(like.shape[2:]) + (like.shape[1],)
    out = _empty_like_rows(like) if like.dim() in (2, 4) else torch.empty_like(like)
    return out.copy_(rows.view(shape).movedim(-1, 1))  # (a tensor of its own: a ReLU may run in place on it)


class _SyncBNActTorchFn(torch.autograd.Function):
    """The same contract as a torch composition (CPU tensors, other dtypes and layouts)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, res, group):
        C = x.shape[1]
        X = _channel_rows(x)
        M = X.shape[0]
        packet = torch.cat([torch.tensor([float(M)], dtype=torch.float64, device=x.device), X.sum(0), (X * X).sum(0)])
        g = _gather(packet, group)
        N, S, Q = g[:, 0].sum(), g[:, 1:1 + C].sum(0), g[:, 1 + C:].sum(0)
        mean = S / N
        var = (Q / N - mean * mean).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
        mu, is_ = mean.float(), invstd.float()
        if running_mean is not None:
            n = N.float()
            unbiased = var.float() * (n / (n - 1)) if float(N) > 1 else var.float()
            running_mean.mul_(1 - momentum).add_(momentum * mu)
            running_var.mul_(1 - momentum).add_(momentum * unbiased)
        gm = weight.detach().float() if weight is not None else torch.ones_like(mu)
        bt = bias.detach().float() if bias is not None else torch.zeros_like(mu)
        k = gm * is_
        sh = bt - mu * k
        pre = X * k.double() + sh.double()
        if res is not None:
            pre = pre + _channel_rows(res)
        y = _from_rows(pre.clamp_min(0) if relu else pre, x)
        ctx.save_for_backward(x, weight, bias, mu, is_, k, sh, y if res is not None else None)
        ctx.relu, ctx.group, ctx.count = relu, group, N
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mu, is_, k, sh, y = ctx.saved_tensors
        X, D = _channel_rows(x), _channel_rows(dy)
        if y is not None and ctx.relu:
            D = D * (_channel_rows(y) > 0)
        elif ctx.relu:
            D = D * ((X * k.double() + sh.double()).float() > 0)
        xhat = (X * is_.double() - (mu * is_).double()).float().double()
        ab = torch.cat([D.sum(0), (D * xhat).sum(0)])
        C = x.shape[1]
        g = _gather(ab, ctx.group)
        A, B = g[:, :C].sum(0), g[:, C:].sum(0)
        N = ctx.count
        dx = k.double() * (D - A / N - xhat * (B / N))
        dw = ab[C:].to(weight.dtype) if weight is not None else None
        db = ab[:C].to(bias.dtype) if bias is not None else None
        dres = _from_rows(D, x) if y is not None and ctx.needs_input_grad[8] else None
        return _from_rows(dx, x), dw, db, None, None, None, None, None, dres, None


def _kernel_ok(x, res) -> bool:
    if not x.is_cuda or x.dtype not in _KERNEL_DTYPES or x.dim() not in (2, 4):
        return False
    c = x.shape[1]
    if c % 8 or c > MAX_C:
        return False
    return res is None or (res.is_cuda and res.dtype == x.dtype and res.shape == x.shape)


def sync_bn_act(x, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=1e-5, relu=True,
                res=None, group=None):
    """``relu?(batch_norm(x) [+ res])`` with the batch statistics of every rank of ``group`` (module docstring)."""
    if momentum is None:
        raise ValueError("sync_bn_act: momentum=None (cumulative moving average) is not supported; pass a float")
    if not training:  # the running statistics: exactly the unsynchronised path
        if res is not None:
            from .residual import bn_add_relu

            if relu and x.is_cuda and x.dtype == torch.bfloat16:
                return bn_add_relu(x, res, weight, bias, running_mean, running_var, False, momentum, eps)
            y = torch.nn.functional.batch_norm(x, running_mean, running_var, weight, bias, False, momentum, eps) + res
            return torch.relu(y) if relu else y
        if x.is_cuda and x.dtype != torch.bfloat16:
            y = torch.nn.functional.batch_norm(x, running_mean, running_var, weight, bias, False, momentum, eps)
            return torch.relu(y) if relu else y
        return bn_act(x, weight, bias, running_mean, running_var, False, momentum, eps, relu)
    if _world(group) > 1 and (tape.recording() or (x.is_cuda and torch.cuda.is_current_stream_capturing())):
        raise RuntimeError("sync_bn_act: the statistics exchange between ranks cannot be part of a tape segment or a "
                           "captured graph; run synchronised BatchNorm in eager mode")
    fn = _SyncBNActFn if _kernel_ok(x, res) else _SyncBNActTorchFn
    return tape.apply(fn, x, weight, bias, running_mean, running_var, momentum, eps, relu, res, group)


class SyncBatchNormAct2d(BatchNormAct2d):
    """``BatchNormAct2d`` whose training statistics are those of every rank of ``process_group`` (None: the default
    group)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=True, process_group=None, **kw):
        if momentum is None:
            raise ValueError("SyncBatchNormAct2d: momentum=None (cumulative moving average) is not supported")
        super().__init__(num_features, eps=eps, momentum=momentum, relu=relu, **kw)
        self.process_group = process_group

    def forward(self, x, res=None):
        training = self.training or not self.track_running_stats
        return sync_bn_act(x, self.weight, self.bias, self.running_mean if self.track_running_stats else None,
                           self.running_var if self.track_running_stats else None, training, self.momentum, self.eps,
                           self.relu, res, self.process_group)

    def extra_repr(self):
        return super().extra_repr() + f", relu={self.relu}, sync=True"


class SyncBatchNorm(SyncBatchNormAct2d):
    """``hvd.SyncBatchNorm``: Horovod's signature, no activation, over the default (Horovod's) process group.
    ``affine=False`` passes null parameters to the kernels."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__(num_features, eps=eps, momentum=momentum, relu=False, process_group=None, affine=affine,
                         track_running_stats=track_running_stats)
