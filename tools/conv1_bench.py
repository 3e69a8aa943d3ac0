#!/usr/bin/env python3
"""Device-event timing of the MNIST CNNs' first layer (csrc/conv1.hip, ops/conv1.py) beside the torch composition it
replaces and beside plain copies of the bytes it must move: 100 launches per window, the arms taking turns window by
window so drift hits all of them alike.

    python tools/conv1_bench.py [--launches 100] [--rounds 5]

The three layer forms (keras_cnn and hvd_cnn: k = 3, pad 0; deepnn: k = 5, pad 2; 28x28 images) at batch 64, the jobs'
per-worker batch, and 128.  Forward: ``tony_conv1_fwd`` against ``F.relu(F.conv2d(x, w, b))``.  Backward: autograd's
backward of either graph (``x`` not requiring grad), which for the kernels is ``tony_conv1_bwd`` + ``tony_conv1_fold``.
Bytes: the forward reads x and writes y, the backward reads dy, y and x; a ``tony_kv_copy`` moves each count, half read
and half written.  These tensors fit in the caches, so the copy is a latency yardstick more than a bandwidth one.
After them the deepnn form with its 2x2 max-pool at both batches ("pooled"): ``conv1_bias_relu(..., pool=True)``, i.e.
``tony_conv1_pool_fwd`` and ``tony_conv1_pool_bwd`` + ``tony_conv1_fold``, against ``F.max_pool2d`` over the composition.
Prints per arm the median / min / max us per launch over the rounds, then whether each kernel arm's slowest round is
below the composition's fastest.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FORMS = [("keras_cnn / hvd_cnn k3 p0", 3, 0), ("deepnn k5 p2", 5, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.ops.conv1 import _Conv1BiasReLU, _Conv1BiasReLUPool, conv1_bias_relu

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.empty(2, 64 << 20, dtype=torch.uint8, device=dev)
    arms = []  # (case, arm, callable)
    for label, k, p in FORMS:
        for n in (64, 128):
            case = f"{label} batch {n}"
            x = torch.rand(n, 1, 28, 28, device=dev, generator=gen)
            w = (torch.randn(32, 1, k, k, device=dev, generator=gen) * 0.2).requires_grad_()
            b = torch.zeros(32, device=dev).requires_grad_()
            y_k, y_t = conv1_bias_relu(x, w, b, p), F.relu(F.conv2d(x, w, b, padding=p))
            assert isinstance(y_k.grad_fn, _Conv1BiasReLU._backward_cls)
            dy = torch.randn(y_k.shape, device=dev, generator=gen)
            fwd_bytes, bwd_bytes = 4 * (x.numel() + y_k.numel()), 4 * (x.numel() + 2 * y_k.numel())

            def copy(nbytes):
                half = nbytes // 2 // 16 * 16
                return lambda: _lib.check(L.tony_kv_copy(pool[1].data_ptr(), pool[0].data_ptr(), half, None, stream), "copy")

            arms += [(case, "fwd kernel", lambda x=x, w=w, b=b, p=p: conv1_bias_relu(x, w, b, p)),
                     (case, "fwd torch", lambda x=x, w=w, b=b, p=p: F.relu(F.conv2d(x, w, b, padding=p))),
                     (case, f"fwd copy {fwd_bytes / 1e6:.1f} MB", copy(fwd_bytes)),
                     (case, "bwd kernel", lambda y=y_k, w=w, b=b, dy=dy: torch.autograd.grad(y, (w, b), dy, retain_graph=True)),
                     (case, "bwd torch", lambda y=y_t, w=w, b=b, dy=dy: torch.autograd.grad(y, (w, b), dy, retain_graph=True)),
                     (case, f"bwd copy {bwd_bytes / 1e6:.1f} MB", copy(bwd_bytes))]
    # deepnn's form with its 2x2 max-pool in the op (csrc/conv1_pool.hip): pooled y and a uint8 idx instead of the
    # full-resolution y, against max_pool2d over the composition
    label, k, p = FORMS[1]
    for n in (64, 128):
        case = f"{label} pooled batch {n}"
        x = torch.rand(n, 1, 28, 28, device=dev, generator=gen)
        w = (torch.randn(32, 1, k, k, device=dev, generator=gen) * 0.2).requires_grad_()
        b = torch.zeros(32, device=dev).requires_grad_()
        y_k = conv1_bias_relu(x, w, b, p, pool=True)
        y_t = F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=p)), 2)
        assert isinstance(y_k.grad_fn, _Conv1BiasReLUPool._backward_cls) and y_k.shape == y_t.shape
        dy = torch.randn(y_k.shape, device=dev, generator=gen)
        fwd_bytes, bwd_bytes = 4 * x.numel() + 5 * y_k.numel(), 4 * x.numel() + 9 * y_k.numel()
        arms += [(case, "fwd kernel", lambda x=x, w=w, b=b, p=p: conv1_bias_relu(x, w, b, p, pool=True)),
                 (case, "fwd torch", lambda x=x, w=w, b=b, p=p: F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=p)), 2)),
                 (case, f"fwd copy {fwd_bytes / 1e6:.1f} MB", copy(fwd_bytes)),
                 (case, "bwd kernel", lambda y=y_k, w=w, b=b, dy=dy: torch.autograd.grad(y, (w, b), dy, retain_graph=True)),
                 (case, "bwd torch", lambda y=y_t, w=w, b=b, dy=dy: torch.autograd.grad(y, (w, b), dy, retain_graph=True)),
                 (case, f"bwd copy {bwd_bytes / 1e6:.1f} MB", copy(bwd_bytes))]
    for _, _, fn in arms:  # warm up: code objects loaded, MIOpen's algorithms chosen, clocks up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {(c, n): [] for c, n, _ in arms}
    for _ in range(a.rounds):
        for c, n, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            us[(c, n)].append(1e3 * e0.elapsed_time(e1) / a.launches)
    print(f"{a.launches} launches per window, {a.rounds} rounds, arms alternating; us per call")
    for (c, n), v in us.items():
        print(f"{c:36s} {n:18s} median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}")
    print("condition: the kernel arm's slowest round below the composition's fastest")
    for c in dict.fromkeys(c for c, _, _ in arms):
        for d in ("fwd", "bwd"):
            kmax, tmin = max(us[(c, f"{d} kernel")]), min(us[(c, f"{d} torch")])
            print(f"{c:36s} {d}  kernel slowest {kmax:8.2f} {'<' if kmax < tmin else '>='} torch fastest {tmin:8.2f}  "
                  f"({'met' if kmax < tmin else 'MISSED'})")


if __name__ == "__main__":
    main()
