"""The MNIST networks of the reference example jobs (parameter counts in SURVEY.md §2.7 K1-K9).

linear       EX/mnist-pytorch/mnist_distributed.py:129-136      Linear(784, 10)
deepnn       EX/mnist-tensorflow/mnist_distributed.py:64-124    conv5x5(32) pool conv5x5(64) pool fc1024 fc10
                                                                  (3,274,634 params)
keras_cnn    EX/mnist-tensorflow/mnist_keras_distributed.py     Conv2D(32,3) Dense(128) Dense(10) (2,770,634)
hvd_cnn      EX/horovod-on-tony/tensorflow2_mnist.py            Conv(32,3) Conv(64,3) pool Dense(128) Dense(10)
                                                                  (1,199,882)
dnn          EX/mnist-tensorflow/mnist_estimator_distributed.py DNNClassifier([256, 128]) (235,146)

``mnist_model``'s flags move layers onto this project's fp32 HIP kernels without changing a state-dict key or an
initial bit: ``fused`` (the CNNs' first conv + ReLU, ``ops.conv1``), ``fused_pool`` (``fused`` with the
``nn.MaxPool2d(2)`` that follows it in ``deepnn`` taken into the same op), ``fused_conv2`` (the 32 -> 64 conv + ReLU +
pool, ``ops.conv2``) and ``fused_dense`` (every ``nn.Linear`` with the ``nn.ReLU`` after it, ``ops.dense``).  With
``fused``, ``fused_conv2`` and ``fused_dense``, ``hvd_cnn`` and ``keras_cnn`` hold no vendor kernel, as ``dnn`` and
``linear`` do with ``fused_dense`` alone; with all four flags ``deepnn`` holds none either.  ``mnist_loss`` is the jobs'
loss line; its ``fused_head`` takes the last layer and the cross-entropy after it into one op (``ops.dense_xent``).
"""
from __future__ import annotations

import torch
from torch import nn


class _Flatten(nn.Module):
    def forward(self, x):
        return x.reshape(x.shape[0], -1)


def linear() -> nn.Module:
    return nn.Sequential(_Flatten(), nn.Linear(784, 10))


def deepnn() -> nn.Module:
    return nn.Sequential(
        nn.Conv2d(1, 32, 5, padding=2), nn.ReLU(), nn.MaxPool2d(2),
        nn.Conv2d(32, 64, 5, padding=2), nn.ReLU(), nn.MaxPool2d(2),
        _Flatten(), nn.Linear(7 * 7 * 64, 1024), nn.ReLU(), nn.Linear(1024, 10))


def keras_cnn() -> nn.Module:
    return nn.Sequential(nn.Conv2d(1, 32, 3), nn.ReLU(), _Flatten(), nn.Linear(26 * 26 * 32, 128), nn.ReLU(),
                         nn.Linear(128, 10))


def hvd_cnn() -> nn.Module:
    return nn.Sequential(nn.Conv2d(1, 32, 3), nn.ReLU(), nn.Conv2d(32, 64, 3), nn.ReLU(), nn.MaxPool2d(2),
                         _Flatten(), nn.Linear(12 * 12 * 64, 128), nn.ReLU(), nn.Linear(128, 10))


def dnn() -> nn.Module:
    return nn.Sequential(_Flatten(), nn.Linear(784, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                         nn.Linear(128, 10))


MODELS = {"linear": linear, "deepnn": deepnn, "keras_cnn": keras_cnn, "hvd_cnn": hvd_cnn, "dnn": dnn}


CONV2_AT = {"deepnn": 3, "hvd_cnn": 2}  # index of the Conv2d(32, 64, k); its ReLU and MaxPool2d(2) follow


def mnist_model(name: str = "deepnn", seed: int = 0, fused: bool = False, fused_conv2: bool = False,
                fused_dense: bool = False, fused_pool: bool = False) -> nn.Module:
    """``fused``: the CNNs' opening ``Conv2d(1, 32, k)`` + ReLU as one ``ops.conv1.Conv1BiasReLU`` (HIP on a GPU).  It
    adopts the parameters of the ``nn.Conv2d`` built here, so the initial bits and the state-dict keys are those of
    ``fused=False`` (index 1 becomes an ``nn.Identity``); the models without that layer are unchanged.

    ``fused_conv2``: likewise ``deepnn``'s and ``hvd_cnn``'s ``Conv2d(32, 64, k)`` + ReLU + ``MaxPool2d(2)`` as one
    ``ops.conv2.Conv2BiasReLUPool`` at the convolution's index, an ``nn.Identity`` at the two after it.

    ``fused_dense``: every ``nn.Linear`` as an ``ops.dense.Dense`` over that layer's parameters, with ``relu`` set and
    an ``nn.Identity`` in the ``nn.ReLU``'s place where one follows it.  Independent of the other two flags.

    ``fused_pool``: implies ``fused``; where an ``nn.MaxPool2d(2)`` follows the first conv's ReLU (``deepnn``) the
    ``Conv1BiasReLU`` takes it in (``pool=True``) and index 2 becomes an ``nn.Identity`` too.  Independent of
    ``fused_conv2`` and ``fused_dense``."""
    torch.manual_seed(seed)
    model = MODELS[name]()
    if (fused or fused_pool) and name in ("deepnn", "keras_cnn", "hvd_cnn"):
        from ..ops.conv1 import Conv1BiasReLU

        pool = fused_pool and isinstance(model[2], nn.MaxPool2d) and model[2].kernel_size == 2
        model[0], model[1] = Conv1BiasReLU(conv=model[0], pool=pool), nn.Identity()
        if pool:
            model[2] = nn.Identity()
    if fused_conv2 and name in CONV2_AT:
        from ..ops.conv2 import Conv2BiasReLUPool

        i = CONV2_AT[name]
        model[i], model[i + 1], model[i + 2] = Conv2BiasReLUPool(conv=model[i]), nn.Identity(), nn.Identity()
    if fused_dense:
        from ..ops.dense import Dense

        for i in dense_layers(model):
            relu = i + 1 < len(model) and isinstance(model[i + 1], nn.ReLU)
            model[i] = Dense(linear=model[i], relu=relu)
            if relu:
                model[i + 1] = nn.Identity()
    return model


def dense_layers(model: nn.Sequential) -> list:
    """Indices of the model's ``nn.Linear`` layers, or of the ``ops.dense.Dense`` modules ``fused_dense`` put there."""
    from ..ops.dense import Dense

    return [i for i, m in enumerate(model) if isinstance(m, (nn.Linear, Dense))]


def mnist_loss(model: nn.Sequential, x, y, fused_head: bool = False):
    """The jobs' training loss, ``F.cross_entropy(model(x), y)``.  ``fused_head``: the layers before the last one run
    as they are and the closing ``Linear(K, 10)`` and the loss become one ``ops.dense_xent.dense_xent`` over that
    layer's ``weight`` and ``bias`` (one HIP launch each way on a GPU).  No module is replaced, so the state-dict keys
    and the initial bits are those of the model as built."""
    if not fused_head:
        return torch.nn.functional.cross_entropy(model(x), y)
    from ..ops.dense import Dense
    from ..ops.dense_xent import dense_xent

    *body, head = model  # what model[:-1](x) runs, without building that nn.Sequential every step
    if not (isinstance(head, nn.Linear) or (isinstance(head, Dense) and not head.relu)) or head.bias is None:
        raise TypeError(f"fused_head takes a model that ends in a Linear with a bias and no ReLU, got {head}")
    for layer in body:
        x = layer(x)
    return dense_xent(x, head.weight, head.bias, y)


def synthetic_mnist(n: int, seed: int = 0, device="cpu"):
    """Deterministic MNIST-shaped batch (no dataset download): images in [0,1], labels from a fixed
    random linear teacher so the task is learnable (loss decreases)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 1, 28, 28, generator=g)
    teacher = torch.randn(784, 10, generator=torch.Generator().manual_seed(1234))
    y = (x.reshape(n, -1) @ teacher).argmax(1)
    return x.to(device), y.to(device)
