"""MI355X (gfx950) compute kernels of tony_amd.

Hand-written HIP kernels (``csrc/*.hip``) built in-tree into
``_tony_kernels.so`` and bound with ctypes:

* ``bn``     -- NHWC BatchNorm(+ReLU) training/inference fwd+bwd (H3/H4)
* ``loss``   -- fused softmax cross-entropy fwd+bwd (H9)
* ``optim``  -- flat-shard fused SGD-momentum / Adam(W) apply, grad stats (H10-H12)
* ``gemm``   -- MFMA bf16 GEMM (LDS-tiled, XCD-aware) for 1x1 convs / FC (H1/H8)
* ``image``  -- uint8 batch + per-sample crop boxes -> the model's input in one launch (H17's real-data side)
* ``metrics`` -- top-1 / top-k evaluation counters

(``image`` and ``metrics`` are imported by their users -- ``tony_amd.data.images``, the jobs -- not from here.)
"""
from ._lib import KernelError, available, lib  # noqa: F401
from .bn import BatchNormAct2d, bn_act  # noqa: F401
from .loss import cross_entropy  # noqa: F401
from .optim import (FlatAdagrad, FlatAdam, FlatLAMB, FlatLARS, FlatRMSProp, FlatSGD, Segments,  # noqa: F401
                    grad_stats)
