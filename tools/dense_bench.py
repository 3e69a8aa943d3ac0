#!/usr/bin/env python3
"""Device-event timing of the MNIST networks' fp32 dense layers (csrc/dense.hip, ops/dense.py) beside the torch
composition they replace and beside plain copies of the bytes they must move: 100 calls per window, the arms taking
turns window by window so drift hits all of them alike.

    python tools/dense_bench.py [--launches 100] [--rounds 5]

Every layer of the five models (K -> N, +R with the ReLU after it) at batch 64 and 128.  Forward: ``ops.dense.dense``
(``tony_dense_fwd``, and ``tony_dense_fold`` where K is split) against ``F.linear`` or ``F.relu(F.linear(...))``.
Backward: autograd's backward of either graph with ``x`` requiring grad, which for the kernels is
``tony_dense_dgrad`` + ``tony_dense_wgrad``.  Bytes: the forward reads x, w and b and writes y; the backward reads dy,
y, w and x and writes dx, dw and db; a ``tony_kv_copy`` moves each count, half read and half written.  These tensors
sit in the Infinity Cache, so the copy is a latency yardstick more than a bandwidth one.  Prints per arm the median /
min / max us per call over the rounds, then whether each kernel arm's slowest round is below the composition's fastest.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

LAYERS = [("linear", 784, 10, False), ("dnn", 784, 256, True), ("dnn", 256, 128, True), ("dnn", 128, 10, False),
          ("deepnn", 3136, 1024, True), ("deepnn", 1024, 10, False), ("keras_cnn", 21632, 128, True),
          ("hvd_cnn", 9216, 128, True)]  # keras_cnn's and hvd_cnn's 128 -> 10 is dnn's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.ops.dense import _Dense, dense

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.empty(2, 64 << 20, dtype=torch.uint8, device=dev)

    def torch_form(x, w, b, relu):
        y = F.linear(x, w, b)
        return F.relu(y) if relu else y

    def copy(nbytes):
        half = max(16, nbytes // 2 // 16 * 16)
        return lambda: _lib.check(L.tony_kv_copy(pool[1].data_ptr(), pool[0].data_ptr(), half, None, stream), "copy")

    arms = []  # (case, arm, callable)
    for model, k, n, relu in LAYERS:
        for m in (64, 128):
            case = f"{model} {k} -> {n}{' +R' if relu else ''} batch {m}"
            x = torch.rand(m, k, device=dev, generator=gen).requires_grad_()
            w = (torch.randn(n, k, device=dev, generator=gen) * 0.05).requires_grad_()
            b = torch.zeros(n, device=dev).requires_grad_()
            y_k, y_t = dense(x, w, b, relu), torch_form(x, w, b, relu)
            assert isinstance(y_k.grad_fn, _Dense._backward_cls)
            dy = torch.randn(m, n, device=dev, generator=gen)
            fwd_bytes = 4 * (m * k + n * k + n + m * n)
            bwd_bytes = 4 * (2 * m * n + 2 * n * k + 2 * m * k + n)
            arms += [(case, "fwd kernel", lambda x=x, w=w, b=b, r=relu: dense(x, w, b, r)),
                     (case, "fwd torch", lambda x=x, w=w, b=b, r=relu: torch_form(x, w, b, r)),
                     (case, f"fwd copy {fwd_bytes / 1e6:.2f} MB", copy(fwd_bytes)),
                     (case, "bwd kernel",
                      lambda y=y_k, x=x, w=w, b=b, dy=dy: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)),
                     (case, "bwd torch",
                      lambda y=y_t, x=x, w=w, b=b, dy=dy: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)),
                     (case, f"bwd copy {bwd_bytes / 1e6:.2f} MB", copy(bwd_bytes))]
    for _, _, fn in arms:  # warm up: code objects loaded, the BLAS's algorithms chosen, clocks up
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
