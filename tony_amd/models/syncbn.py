"""``convert_sync_batchnorm``: a model's BatchNorm layers take their training statistics over all ranks' batches
(ops/syncbn.py), like ``torch.nn.SyncBatchNorm.convert_sync_batchnorm``.

``nn.BatchNorm2d`` and ``BatchNormAct2d`` modules are replaced by ``SyncBatchNormAct2d`` modules that SHARE their
parameters and buffers (an optimizer or a flat buffer built before the conversion keeps working).  The fused
containers read BN parameters directly and feed them to kernels that fold the local statistics into a conv
epilogue, so they are re-classed, keeping every parameter and submodule:

* ``ConvBNAct``  -> ``SyncConvBNAct``: the training forward is ``conv_ops.conv2d`` followed by ``sync_bn_act``;
* ``Bottleneck`` -> ``SyncBottleneck``: the tail is the 1x1 conv followed by ``sync_bn_act(res=identity)``;
* ``ResNet``     -> ``SyncResNet``: the stem's BN + ReLU + max pool are the synchronised BN and the tony max pool.

Evaluation goes through the parent classes: the running statistics need no exchange.  A fused or x3 ``InceptionV3``
is refused with a ``TypeError``: its multi-split heads normalise several layers in one launch from local statistics.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops import conv as conv_ops
from ..ops.pool import global_avg_pool, max_pool
from ..ops.syncbn import SyncBatchNormAct2d, sync_bn_act
from .inception_v3 import InceptionV3
from .layers import ConvBNAct
from .resnet import Bottleneck, ResNet


def _bn_args(bn):
    return (bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
            bn.running_var if bn.track_running_stats else None)


class SyncConvBNAct(ConvBNAct):
    def forward(self, x, slot=None):
        if not self.training:
            return super().forward(x, slot)
        c = self.conv
        y = self.bn(conv_ops.conv2d(x, c.weight, c.stride, c.padding))  # a SyncBatchNormAct2d (with the ReLU if fused)
        return y if self.fused else self.act(y)


class SyncBottleneck(Bottleneck):
    def forward(self, x):
        if not self.training:
            return super().forward(x)
        if self.downsample is None:
            identity = x
        else:
            c, bn = self.downsample[0], self.downsample[1]
            identity = bn(conv_ops.conv2d(x, c.weight, c.stride, c.padding))
        out = self.conv2(self.conv1(x))
        bn = self.bn3
        z = conv_ops.conv2d(out, self.conv3.weight)
        return sync_bn_act(z, *_bn_args(bn), True, bn.momentum, bn.eps, True, identity, bn.process_group)


class SyncResNet(ResNet):
    def forward(self, x):
        if not self.training:
            return super().forward(x)
        y = self.stem(x)
        x = max_pool(y, 3, 2, padding=1) if self.fused else nn.functional.max_pool2d(y, 3, 2, 1)
        x = self.blocks(x)
        x = global_avg_pool(x) if self.fused else x.mean((2, 3))
        return self.fc(x)


_RECLASS = {ConvBNAct: SyncConvBNAct, Bottleneck: SyncBottleneck, ResNet: SyncResNet}


def _sync_bn(bn: nn.BatchNorm2d, process_group) -> SyncBatchNormAct2d:
    if bn.momentum is None:
        raise ValueError("convert_sync_batchnorm: momentum=None (cumulative moving average) is not supported")
    with torch.device("meta"):  # no storage of its own: every parameter and buffer below is the original's
        new = SyncBatchNormAct2d(bn.num_features, eps=bn.eps, momentum=bn.momentum, relu=getattr(bn, "relu", False),
                                 process_group=process_group, affine=bn.affine,
                                 track_running_stats=bn.track_running_stats)
    for name in ("weight", "bias"):
        new._parameters[name] = bn._parameters[name]
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        new._buffers[name] = bn._buffers[name]
    new.training = bn.training
    return new


def convert_sync_batchnorm(module: nn.Module, process_group=None) -> nn.Module:
    """Replace every ``nn.BatchNorm2d`` / ``BatchNormAct2d`` under ``module`` by a ``SyncBatchNormAct2d`` over
    ``process_group`` sharing its parameters and buffers, and re-class the fused containers (module docstring).
    Returns the converted module (``module`` itself unless it is a BatchNorm layer)."""
    for m in module.modules():
        if isinstance(m, InceptionV3) and (m.fused or m.x3):
            raise TypeError(f"convert_sync_batchnorm: a fused or x3 {type(m).__name__} normalises the splits of its "
                            "fused heads from local statistics in one launch and cannot be synchronised; build it "
                            "with fused=False")
    if isinstance(module, nn.BatchNorm2d) and not isinstance(module, SyncBatchNormAct2d):
        return _sync_bn(module, process_group)
    for name, child in list(module.named_children()):
        new = convert_sync_batchnorm(child, process_group)
        if new is not child:
            module._modules[name] = new
    cls = _RECLASS.get(type(module))
    if cls is not None:
        module.__class__ = cls
        module.__dict__.pop("_routes", None)
    return module


__all__ = ["SyncBatchNormAct2d", "SyncBottleneck", "SyncConvBNAct", "SyncResNet", "convert_sync_batchnorm"]
