"""Shared by the image-pipeline tests (test_image_cpu.py, test_image_gpu.py): the float64 reference of
``ops.image.preprocess``, its error bound, and the box tables that cover every kind of box."""
import numpy as np
import torch
import torch.nn.functional as F

INCEPTION = ((1 / 127.5,) * 3, (-1.0,) * 3)
RESNET = (tuple(1 / (255 * s) for s in (0.229, 0.224, 0.225)),
          tuple(-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))))

# (N, (H, W), (OH, OW)): the smallest geometries at which the kernel can still go wrong
GEOMETRIES = [
    (3, (37, 53), (19, 23)),  # 3933 output elements (no multiple of 8), 1311 per sample (odd): groups straddle
    (2, (20, 20), (33, 31)),  # upscale
    (1, (5, 7), (40, 3)),
    (2, (320, 360), (299, 299)),  # one real-sized case
]


def f32(v):
    """The fp32 constants the op receives, widened to float64."""
    return torch.tensor([float(np.float32(t)) for t in v], dtype=torch.float64)


def reference(src, boxes, size, scale, bias):
    """float64 [N, 3, OH, OW]: crop, convert to float64, ``F.interpolate(bilinear, align_corners=False,
    antialias=False)``, flip, then ``* scale + bias`` with the fp32 constants widened to float64."""
    out = []
    for img, (y0, x0, h, w, flip) in zip(src.cpu(), boxes.cpu().tolist()):
        crop = img[y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].to(torch.float64)
        r = F.interpolate(crop, size=tuple(size), mode="bilinear", align_corners=False, antialias=False)
        out.append(r.flip(-1) if flip else r)
    return torch.cat(out) * f32(scale)[None, :, None, None] + f32(bias)[None, :, None, None]


def bound(scale, bias):
    """B_c [1, 3, 1, 1] = 16 * 2^-24 * (255 |scale_c| + |bias_c|): the worst case of the ~14 fp32 roundings of the
    formula, each on a magnitude <= 255, plus the final multiply-add."""
    return (16 * 2.0 ** -24 * (255 * f32(scale).abs() + f32(bias).abs()))[None, :, None, None]


def halfulp_bf16(ref):
    """Half a bf16 ulp (8 significand bits) at ``ref``: 2^(floor(log2 |ref|) - 8)."""
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -126))  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e - 1 - 8)


def assert_close(got, ref, scale, bias, what):
    """fp32: |got - ref| <= B_c; bf16: |got - ref| <= halfulp_bf16(ref) + B_c."""
    lim = bound(scale, bias).expand_as(ref)
    if got.dtype == torch.bfloat16:
        lim = lim + halfulp_bf16(ref)
    err = (got.detach().cpu().to(torch.float64) - ref).abs()
    over = err > lim
    worst = float((err / lim).max())
    print(f"{what}: max |got - ref| / bound = {worst:.4f}")
    assert not bool(over.any()), \
        f"{what}: {int(over.sum())} of {err.numel()} elements over the bound (worst {worst:.3f}x)"


def box_tables(N, H, W, seed=0):
    """int32 [N, 5] tables that together hold: random interior boxes with both flips, a 1 x 1 box, a box ending on
    the image's last row and column, the full image with both flips, one-row and one-column boxes."""
    rng = np.random.default_rng(seed)

    def interior(flip):
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        return [int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, flip]

    hh, ww = max(1, H // 2), max(1, W // 3)
    kinds = [interior(0), interior(1),
             [int(rng.integers(0, H)), int(rng.integers(0, W)), 1, 1, 0], [H - 1, W - 1, 1, 1, 1],
             [H - hh, W - ww, hh, ww, 1], [H - hh, W - ww, hh, ww, 0],
             [0, 0, H, W, 0], [0, 0, H, W, 1],
             [H // 2, 0, 1, W, 1], [0, W // 2, H, 1, 0]]
    while len(kinds) % N:
        kinds.append(interior(len(kinds) % 2))
    return [torch.tensor(kinds[i:i + N], dtype=torch.int32) for i in range(0, len(kinds), N)]


def pixels(N, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
