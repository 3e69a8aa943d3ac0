#!/usr/bin/env python3
"""Device-event timing of the MNIST classifier head as one op (csrc/dense_xent.hip, ops/dense_xent.py) beside the
composition it stands for, ``ops.cross_entropy(ops.dense.dense(x, w, b), y)``, and beside the jobs' default loss line,
``F.cross_entropy(F.linear(x, w, b), y)``: 100 calls per window, the arms taking turns window by window so drift hits
all of them alike.

    python tools/dense_xent_bench.py [--launches 100] [--rounds 5]

The three head shapes (K -> 10 for K = 784, 1024, 128) at batch 64 and 128, mean reduction.  ``fwd`` is the loss alone;
``fwd+bwd`` adds ``torch.autograd.grad`` of it with respect to x, w and b.  Launches per arm, forward / backward: the op
1 / 1 plus torch's mean and its backward; the composition 2 - 3 / 3 plus the same; torch's line 3 - 4 / 5 - 6.  Every
call includes its Python and autograd issue cost, on all sides.  Prints per arm the median / min / max us per call over
the rounds, then whether the op's slowest round is below the fastest round of each other arm.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HEADS = [("linear", 784), ("deepnn", 1024), ("dnn / keras_cnn / hvd_cnn", 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops.dense import dense
    from tony_amd.ops.dense_xent import _DenseXent, dense_xent
    from tony_amd.ops.loss import cross_entropy

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    forms = {"op": dense_xent, "composition": lambda x, w, b, y: cross_entropy(dense(x, w, b), y),
             "torch": lambda x, w, b, y: F.cross_entropy(F.linear(x, w, b), y)}

    def both(form, x, w, b, y):
        return torch.autograd.grad(form(x, w, b, y), (x, w, b))

    arms = []  # (case, arm, callable)
    for model, k in HEADS:
        for m in (64, 128):
            case = f"{model} {k} -> 10 batch {m}"
            x = torch.rand(m, k, device=dev, generator=gen).requires_grad_()
            w = (torch.randn(10, k, device=dev, generator=gen) * 0.05).requires_grad_()
            b = torch.zeros(10, device=dev).requires_grad_()
            y = torch.randint(0, 10, (m,), device=dev, generator=gen)
            per_row = dense_xent(x, w, b, y, reduction="none")
            assert isinstance(per_row.grad_fn, _DenseXent._backward_cls)
            want = F.cross_entropy(F.linear(x, w, b), y)
            assert all(abs(float(f(x, w, b, y)) - float(want)) < 1e-4 for f in forms.values()), case
            for name, form in forms.items():
                arms += [(case, f"fwd {name}", lambda f=form, t=(x, w, b, y): f(*t)),
                         (case, f"fwd+bwd {name}", lambda f=form, t=(x, w, b, y): both(f, *t))]
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
        print(f"{c:46s} {n:20s} median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}")
    print("condition: the op's slowest round below the other arm's fastest")
    for c in dict.fromkeys(c for c, _, _ in arms):
        for d in ("fwd", "fwd+bwd"):
            omax = max(us[(c, f"{d} op")])
            for other in ("composition", "torch"):
                tmin = min(us[(c, f"{d} {other}")])
                print(f"{c:46s} {d:8s} op slowest {omax:8.2f} {'<' if omax < tmin else '>='} {other} fastest "
                      f"{tmin:8.2f}  ({'met' if omax < tmin else 'MISSED'})")


if __name__ == "__main__":
    main()
