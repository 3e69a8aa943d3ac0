#!/usr/bin/env python3
"""Device-event timing of the image preprocess kernel (csrc/image.hip) alone against the same work composed from
stock torch ops on the same device tensors and boxes: per-sample crop, ``F.interpolate`` (bilinear), flip,
normalise, then the cast to channels_last bf16 / fp32.  The method of tools/optim_bench.py: warm-up, then the
arms take turns window by window so drift hits both alike.

    python tools/image_bench.py [--batch 128] [--src 346] [--size 299] [--launches 20] [--rounds 5]

Prints per arm and dtype the median / min / max us per batch over the rounds, and for the kernel the GB/s its
bytes imply: the source bytes inside the boxes plus the output bytes.  The colour-distortion forms of the kernel
(``preprocess(..., colour=table)``) take their turns in the same rounds: the fast form (brightness and saturation:
one launch), the full form (statistics + fold + apply) and the full form's apply pass alone (the same table with
the statistics skipped); the statistics pass is listed as the difference of the two medians.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--src", type=int, default=346)
    ap.add_argument("--size", type=int, default=299)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops.image import (colour_scratch_floats, inception_colour_params, inception_train_boxes,
                                    normalisation, preprocess)

    dev = torch.device("cuda", 0)
    N, S, O = a.batch, a.src, a.size
    src = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev)
    table = inception_train_boxes(np.random.default_rng(0), N, S, S)
    boxes = torch.from_numpy(table).to(dev)
    host_boxes = table.tolist()
    scale, bias = normalisation("inception")
    sc = torch.tensor(scale, device=dev).view(1, 3, 1, 1)
    bi = torch.tensor(bias, device=dev).view(1, 3, 1, 1)
    box_bytes = int((table[:, 2].astype(np.int64) * table[:, 3]).sum()) * 3

    def kernel(dtype):
        out = torch.empty((N, O, O, 3), dtype=dtype, device=dev).permute(0, 3, 1, 2)
        return lambda: preprocess(src, boxes, O, dtype, scale, bias, out=out)

    crng = np.random.default_rng(1)
    fast = torch.from_numpy(inception_colour_params(crng, N, fast=True)).to(dev)
    full = torch.from_numpy(inception_colour_params(crng, N)).to(dev)
    scratch = torch.empty(colour_scratch_floats(N, O, O), dtype=torch.float32, device=dev)

    def coloured(dtype, table, stats):
        out = torch.empty((N, O, O, 3), dtype=dtype, device=dev).permute(0, 3, 1, 2)
        return lambda: preprocess(src, boxes, O, dtype, scale, bias, out=out, colour=table,
                                  colour_has_contrast=stats, scratch=scratch if stats else None)

    def composed(dtype):
        out = torch.empty((N, O, O, 3), dtype=dtype, device=dev).permute(0, 3, 1, 2)

        def run():
            for n, (y0, x0, h, w, flip) in enumerate(host_boxes):
                crop = src[n, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].float()
                r = F.interpolate(crop, size=(O, O), mode="bilinear", align_corners=False, antialias=False)
                if flip:
                    r = r.flip(-1)
                out[n:n + 1].copy_(r * sc + bi)  # normalise; the copy casts and changes the layout

        return run

    variants = []
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        esz = 2 if dtype == torch.bfloat16 else 4
        variants.append((f"tony_image_preprocess {name}", box_bytes + N * O * O * 3 * esz, kernel(dtype)))
        variants.append((f"colour fast           {name}", 0, coloured(dtype, fast, False)))
        variants.append((f"colour full           {name}", 0, coloured(dtype, full, True)))
        variants.append((f"colour full, apply    {name}", 0, coloured(dtype, full, False)))
        variants.append((f"torch composition     {name}", 0, composed(dtype)))
    for _, _, fn in variants:  # warm up: code objects loaded, clocks up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    print(f"N={N}, {S}x{S} -> {O}x{O}, {box_bytes / 1e6:.1f} MB inside the boxes, {a.launches} batches per window, "
          f"{a.rounds} rounds")
    for name, nbytes, _ in variants:
        v = us[name]
        med = statistics.median(v)
        rate = f"{nbytes / med / 1e3:8.1f} GB/s" if nbytes else ""
        print(f"{name:30s} {med:10.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {rate}")
        if name.startswith("colour full, apply"):
            stats = statistics.median(us[name.replace("full, apply", "full       ")]) - med
            print(f"{name.replace('full, apply', 'full, stats'):30s} {stats:10.1f} us  (full - apply)")


if __name__ == "__main__":
    main()
