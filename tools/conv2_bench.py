#!/usr/bin/env python3
"""Device-event timing of the MNIST CNNs' 32 -> 64 conv + bias + ReLU + 2x2 max-pool (csrc/conv2.hip, ops/conv2.py)
beside the torch composition it replaces and beside plain copies of the bytes it must move: 100 calls per window, the
arms taking turns window by window so drift hits all of them alike.

    python tools/conv2_bench.py [--launches 100] [--rounds 5]

The two layer forms (deepnn: k = 5, pad 2 on 14x14; hvd_cnn: k = 3, pad 0 on 26x26) at batch 64 and 128.  Forward:
``tony_conv2_fwd`` against ``F.max_pool2d(F.relu(F.conv2d(x, w, b)), 2)``.  Backward: autograd's backward of either
graph with ``x`` requiring grad, which for the kernels is ``tony_conv2_dgrad`` + ``tony_conv2_wgrad`` +
``tony_conv2_fold``.  Bytes: the forward reads x and writes y and idx, the backward reads dy, y, idx and x and writes
dx; a ``tony_kv_copy`` moves each count, half read and half written.  These tensors fit in the caches, so the copy is
a latency yardstick more than a bandwidth one.  Prints per arm the median / min / max us per call over the rounds,
then whether each kernel arm's slowest round is below the composition's fastest.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FORMS = [("deepnn k5 p2 14x14", 5, 2, 14), ("hvd_cnn k3 p0 26x26", 3, 0, 26)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.ops.conv2 import _Conv2BiasReLUPool, conv2_bias_relu_pool

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.empty(2, 64 << 20, dtype=torch.uint8, device=dev)

    def torch_form(x, w, b, p):
        return F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=p)), 2)

    def copy(nbytes):
        half = nbytes // 2 // 16 * 16
        return lambda: _lib.check(L.tony_kv_copy(pool[1].data_ptr(), pool[0].data_ptr(), half, None, stream), "copy")

    arms = []  # (case, arm, callable)
    for label, k, p, hw in FORMS:
        for n in (64, 128):
            case = f"{label} batch {n}"
            x = torch.rand(n, 32, hw, hw, device=dev, generator=gen).requires_grad_()
            w = (torch.randn(64, 32, k, k, device=dev, generator=gen) * 0.05).requires_grad_()
            b = torch.zeros(64, device=dev).requires_grad_()
            y_k, y_t = conv2_bias_relu_pool(x, w, b, p), torch_form(x, w, b, p)
            assert isinstance(y_k.grad_fn, _Conv2BiasReLUPool._backward_cls)
            dy = torch.randn(y_k.shape, device=dev, generator=gen)
            fwd_bytes = 4 * x.numel() + 5 * y_k.numel()
            bwd_bytes = 8 * x.numel() + 9 * y_k.numel()
            arms += [(case, "fwd kernel", lambda x=x, w=w, b=b, p=p: conv2_bias_relu_pool(x, w, b, p)),
                     (case, "fwd torch", lambda x=x, w=w, b=b, p=p: torch_form(x, w, b, p)),
                     (case, f"fwd copy {fwd_bytes / 1e6:.1f} MB", copy(fwd_bytes)),
                     (case, "bwd kernel",
                      lambda y=y_k, x=x, w=w, b=b, dy=dy: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)),
                     (case, "bwd torch",
                      lambda y=y_t, x=x, w=w, b=b, dy=dy: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)),
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
        print(f"{c:30s} {n:18s} median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}")
    print("condition: the kernel arm's slowest round below the composition's fastest")
    for c in dict.fromkeys(c for c, _, _ in arms):
        for d in ("fwd", "bwd"):
            kmax, tmin = max(us[(c, f"{d} kernel")]), min(us[(c, f"{d} torch")])
            print(f"{c:30s} {d}  kernel slowest {kmax:8.2f} {'<' if kmax < tmin else '>='} torch fastest {tmin:8.2f}  "
                  f"({'met' if kmax < tmin else 'MISSED'})")


if __name__ == "__main__":
    main()
