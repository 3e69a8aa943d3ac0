#!/usr/bin/env python3
"""Device-event timing of the flat optimizer kernels (csrc/optim.hip, csrc/layerwise.hip) alone, the method of the
README's optimizer paragraphs: 27.2 M parameters (Inception-v3), bf16 gradient in, bf16 copy out, 100 launches per
window, the variants taking turns window by window so drift hits all of them alike.

    python tools/optim_bench.py [--params 27200000] [--launches 100] [--rounds 5]

Prints per variant the median / min / max ms per launch over the rounds and the HBM rate its bytes imply.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=27_200_000)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops import FlatAdam, FlatLAMB, FlatLARS, FlatRMSProp, FlatSGD, Segments

    dev = torch.device("cuda", 0)
    n = (a.params + 3) // 4 * 4
    grad = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
    out = torch.zeros(n, dtype=torch.bfloat16, device=dev)

    def sgd(**kw):
        return FlatSGD(torch.randn(n, device=dev), 1e-3, momentum=0.9, weight_decay=4e-5, **kw)

    def rms(**kw):
        return FlatRMSProp(torch.randn(n, device=dev), 1e-3, momentum=0.9, eps=1.0, weight_decay=4e-5, tf_style=True,
                           **kw)

    def adam():
        return FlatAdam(torch.randn(n, device=dev), 1e-3, weight_decay=4e-5)

    # LARS / LAMB: 94 weight tensors of equal length, each followed by a BatchNorm scale and shift of 256 floats
    # (not adapted), about the tensor count and the mix of Inception-v3
    big = (n - 94 * 512) // 94 // 4 * 4
    starts, adapt = [0], []
    for i in range(94):
        last = n - 512 if i == 93 else starts[-1] + big
        starts += [last, last + 256, last + 512]
        adapt += [True, False, False]
    seg = Segments(starts, list(range(len(adapt))), adapt)
    lars = FlatLARS(torch.randn(n, device=dev), 1e-3, momentum=0.9, weight_decay=4e-5, segments=seg)
    lamb = FlatLAMB(torch.randn(n, device=dev), 1e-3, weight_decay=4e-5, segments=seg)
    for opt in (lars, lamb):  # one whole step: the ratio table the timed applies read
        opt.step(grad, out_bf16=out)
        opt.begin_step()

    def apply(opt):
        opt.begin_step()
        if opt.needs_norm:  # the coefficient of one norm pass, outside the timed windows
            opt.accumulate_sumsq(grad, 0)
            opt.finish_norm(1)
        return lambda: opt.apply_range(grad, 0, out_bf16=out)

    norm_opt = sgd(clip_norm=2.0)
    norm_opt.begin_step()
    many = sgd(clip_norm=2.0)
    many.begin_step()
    many.partials(16)
    # (name, bytes per parameter, launch)
    variants = [
        ("tony_sgd_step", 20, apply(sgd())),
        ("apply_x sgd, clip", 20, apply(sgd(clip_norm=2.0))),
        ("apply_x sgd, clip + ema", 28, apply(sgd(clip_norm=2.0, ema_decay=0.9999))),
        ("tony_adam_step", 28, apply(adam())),
        ("tony_lars_norm", 6, lambda: lars.norm_range(grad, 0)),
        ("tony_lars_apply", 20, lambda: lars.apply_range(grad, 0, out_bf16=out)),
        ("tony_lamb_norm", 22, lambda: lamb.norm_range(grad, 0)),
        ("tony_lamb_apply", 18, lambda: lamb.apply_range(grad, 0, out_bf16=out)),
        ("tony_layerwise_fold + ratio", 0, lambda: (lars.fold_norms(), lars.finish_ratios())),
        ("tony_rmsprop_step (tf)", 28, apply(rms())),
        ("apply_x rmsprop_tf, clip", 28, apply(rms(clip_norm=2.0))),
        ("apply_x rmsprop_tf, clip + ema", 36, apply(rms(clip_norm=2.0, ema_decay=0.9999))),
        ("tony_grad_sumsq (bf16)", 2, lambda: norm_opt.accumulate_sumsq(grad, 0)),
        ("tony_clip_ctl, 1 block", 0, lambda: norm_opt.finish_norm(1)),
        ("tony_clip_ctl, 16 blocks", 0, lambda: many.finish_norm(16)),
    ]
    for _, _, fn in variants:  # warm up: code objects loaded, clocks up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    print(f"{n} parameters, {a.launches} launches per window, {a.rounds} rounds")
    for name, bpp, _ in variants:
        v = ms[name]
        med = statistics.median(v)
        rate = f"{bpp * n / med / 1e9:6.2f} TB/s" if bpp else "           "
        print(f"{name:32s} {med:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {bpp:2d} B/param  {rate}")


if __name__ == "__main__":
    main()
