"""Image input pipeline: uint8 NHWC batch + per-sample crop boxes -> the model's channels_last input in one
launch (HIP kernel in csrc/image.hip), and the host-side box samplers that fill the box table.

``out = bilinear(crop) * scale[c] + bias[c]`` with torch's ``bilinear, align_corners=False, antialias=False``
positions, formed as exact rationals: for output row ``oy`` of a crop ``h`` rows high,
``num = max((2*oy+1)*h - OH, 0)``, ``iy0 = num // (2*OH)``, ``ly = float(num % (2*OH)) / float(2*OH)``,
``iy1 = min(iy0+1, h-1)``; columns alike, and with ``flip`` column ``ox`` samples position ``OW-1-ox``.
On CPU tensors (local-mode jobs) a torch implementation of the same formula in fp32 is used.

Colour distortion (Inception's training recipe) sits between the bilinear sample ``v`` and the normalisation: with a
float32 table ``colour`` ``[N, 5]`` of ``(order, brightness delta, saturation factor, hue delta, contrast factor)``
a sample computes ``u = v / 255``, applies its ops in the order of its code (``COLOUR_ORDERS``), clips to [0, 1]
and writes ``u * (255 * scale[c]) + bias[c]``; a sample with code -1 is written exactly as without a table.  With
``M = max``, ``m = min``, ``R = M - m`` of a pixel and its hue sextant coordinate ``h6`` in [0, 6) (0 if ``R == 0``;
``(g-b)/R`` (+6 if negative) if ``M == r``; ``(b-r)/R + 2`` if ``M == g``; else ``(r-g)/R + 4``) and the channel
weights ``d_r = clamp(|h6-3| - 1, 0, 1)``, ``d_g = clamp(2 - |h6-2|, 0, 1)``, ``d_b = clamp(2 - |h6-4|, 0, 1)``:

    brightness(d)   x_c + d
    saturation(f)   R' = max(0, min(R*f, M));  (M - R') + R' * d_c(h6)
    hue(d)          h6' = (h6 + 6*d) mod 6 in [0, 6);  m + R * d_c(h6')
    contrast(f)     (x_c - mean_c) * f + mean_c, mean_c the mean over the sample's OH x OW output pixels of the
                    (unclipped) value entering the contrast stage

These forms equal the RGB -> HSV -> RGB formulas on [0, 1] and are continuous everywhere.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_DIM = 4096  # csrc/image.hip kMaxDim: (2*o+1)*h stays inside int32

# colour table order code -> the ops of a sample, in order (-1: none; 4 / 5: TF-slim's fast mode)
COLOUR_ORDERS = {-1: "", 0: "bshc", 1: "sbch", 2: "chbs", 3: "hscb", 4: "bs", 5: "sb"}
STAT_BLOCKS = 64  # csrc/image.hip kStatBlocks: at most this many partial sums per sample and channel

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalisation(model: str) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """(scale, bias) of ``pixel * scale + bias``: Inception maps [0, 255] to [-1, 1], ResNet applies the
    ImageNet mean / std to pixel / 255."""
    if model == "inception":
        return (1 / 127.5,) * 3, (-1.0,) * 3
    if model == "resnet":
        return tuple(1 / (255 * s) for s in IMAGENET_STD), tuple(-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD))
    raise ValueError(f"model must be 'inception' or 'resnet', got {model!r}")


def _f32x3(v) -> Tuple[float, float, float]:
    v = (v,) * 3 if np.isscalar(v) else tuple(v)
    if len(v) != 3:
        raise ValueError(f"scale / bias take one value or three, got {len(v)}")
    return tuple(float(np.float32(t)) for t in v)  # the fp32 constants the kernel receives by value


def _positions(length: torch.Tensor, o: int, flip=None):
    """(i0, i1, l) [N, o] of the ``o`` output positions over crops ``length`` [N] long (module docstring)."""
    pos = torch.arange(o, dtype=torch.int64, device=length.device)[None, :].expand(length.numel(), o)
    if flip is not None:
        pos = torch.where(flip[:, None] != 0, o - 1 - pos, pos)
    num = ((2 * pos + 1) * length[:, None] - o).clamp_(min=0)
    i0 = num // (2 * o)
    frac = (num % (2 * o)).to(torch.float32) / float(2 * o)
    i1 = torch.minimum(i0 + 1, length[:, None] - 1)
    return i0, i1, frac


def _preprocess_cpu(src, boxes, OH: int, OW: int, scale, bias, colour=None) -> torch.Tensor:
    """fp32 [N, OH, OW, 3] by the kernel's formula."""
    N, H, W, _ = src.shape
    b = boxes.to(torch.int64)
    y0, x0 = b[:, 0].clamp(0, H - 1), b[:, 1].clamp(0, W - 1)
    h, w = b[:, 2].clamp(1, H), b[:, 3].clamp(1, W)
    iy0, iy1, ly = _positions(h, OH)
    ix0, ix1, lx = _positions(w, OW, b[:, 4])
    r0, r1 = (y0[:, None] + iy0).clamp_(max=H - 1), (y0[:, None] + iy1).clamp_(max=H - 1)
    c0, c1 = (x0[:, None] + ix0).clamp_(max=W - 1), (x0[:, None] + ix1).clamp_(max=W - 1)
    n = torch.arange(N)[:, None, None]

    def px(r, c):
        return src[n, r[:, :, None], c[:, None, :]].to(torch.float32)  # [N, OH, OW, 3]

    lx, ly = lx[:, None, :, None], ly[:, :, None, None]
    a, bb, c, d = px(r0, c0), px(r0, c1), px(r1, c0), px(r1, c1)
    top = a + lx * (bb - a)
    bot = c + lx * (d - c)
    v = top + ly * (bot - top)
    plain = v * torch.tensor(scale, dtype=torch.float32) + torch.tensor(bias, dtype=torch.float32)
    if colour is None:
        return plain
    k = torch.tensor([float(np.float32(255.0) * np.float32(s)) for s in scale], dtype=torch.float32)
    for n in range(N):
        order = float(colour[n, 0])
        ops = COLOUR_ORDERS.get(int(order), "") if order == int(order) else ""
        if ops:
            u = _colour_ops_cpu(v[n] / 255.0, ops, *(colour[n, 1:].to(torch.float32)))
            plain[n] = u.clamp(0.0, 1.0) * k + torch.tensor(bias, dtype=torch.float32)
    return plain


def _hue6(x: torch.Tensor):
    """(M, m, R, h6) of fp32 pixels ``[..., 3]`` (module docstring)."""
    r, g, b = x.unbind(-1)
    M, m = x.amax(-1), x.amin(-1)
    R = M - m
    safe = torch.where(R == 0, torch.ones_like(R), R)
    hr = (g - b) / safe
    hr = torch.where(hr < 0, hr + 6.0, hr)
    h6 = torch.where(M == r, hr, torch.where(M == g, (b - r) / safe + 2.0, (r - g) / safe + 4.0))
    return M, m, R, torch.where(R == 0, torch.zeros_like(R), h6)


def _hue_weights(h6: torch.Tensor) -> torch.Tensor:
    return torch.stack([((h6 - 3.0).abs() - 1.0), 2.0 - (h6 - 2.0).abs(), 2.0 - (h6 - 4.0).abs()], -1).clamp(0.0, 1.0)


def _colour_ops_cpu(x: torch.Tensor, ops: str, db, fs, dh, fc) -> torch.Tensor:
    """The ops of one sample on its fp32 ``[OH, OW, 3]`` pixels in [0, 1] units, unclipped."""
    for op in ops:
        if op == "b":
            x = x + db
        elif op == "s":
            M, _, R, h6 = _hue6(x)
            Rp = torch.minimum(R * fs, M).clamp(min=0.0)
            x = (M - Rp)[..., None] + Rp[..., None] * _hue_weights(h6)
        elif op == "h":
            _, m, R, h6 = _hue6(x)
            t = h6 + 6.0 * dh
            t = t - 6.0 * torch.floor(t / 6.0)
            t = torch.where(t >= 6.0, t - 6.0, torch.where(t < 0, t + 6.0, t))
            x = m[..., None] + R[..., None] * _hue_weights(t)
        else:  # the mean of the fp32 values, summed in float64 and rounded once
            mean = x.to(torch.float64).mean((0, 1)).to(torch.float32)
            x = (x - mean) * fc + mean
    return x


def colour_scratch_floats(N: int, OH: int, OW: int) -> int:
    """fp32 elements of the statistics scratch of a ``[N, 3, OH, OW]`` launch whose table may hold contrast:
    ``N * (B + 1) * 3`` with ``B = min(STAT_BLOCKS, ceil(OH * OW / 256))`` partial sums per sample and channel,
    then the means (``tony_image_colour_scratch_floats`` answers the same)."""
    return N * (min(STAT_BLOCKS, -(-(OH * OW) // 256)) + 1) * 3


def preprocess(src_u8: torch.Tensor, boxes: torch.Tensor, size, dtype=torch.bfloat16, scale=1.0, bias=0.0,
               out: torch.Tensor = None, colour: torch.Tensor = None, colour_has_contrast: bool = True,
               scratch: torch.Tensor = None) -> torch.Tensor:
    """The channels_last ``[N, 3, OH, OW]`` input of ``dtype`` (bf16 / fp32) from the dense uint8 ``src_u8``
    ``[N, H, W, 3]`` and the int32 box table ``boxes`` ``[N, 5]`` of ``(y0, x0, h, w, flip)`` on the same device.
    ``out``: a channels_last ``[N, 3, OH, OW]`` tensor to write into (one persistent buffer across steps).

    ``colour``: a float32 ``[N, 5]`` table of ``(order, brightness delta, saturation factor, hue delta, contrast
    factor)`` on the same device (module docstring); ``None`` is the call without colour distortion.
    ``colour_has_contrast=False`` promises that no row's order is 0..3 and skips the statistics launches (a row
    that breaks the promise has its contrast taken about a zero mean).  ``scratch``: a contiguous fp32 buffer of
    at least ``colour_scratch_floats(N, OH, OW)`` elements for the statistics, allocated when not given."""
    OH, OW = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError(f"src must be a dense [N, H, W, 3] tensor, got {tuple(src_u8.shape)}")
    N, H, W, _ = src_u8.shape
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (N, 5) or not boxes.is_contiguous() \
            or boxes.device != src_u8.device:
        raise ValueError(f"boxes must be a contiguous int32 [{N}, 5] table on {src_u8.device}, got {boxes.dtype} "
                         f"{tuple(boxes.shape)} on {boxes.device}")
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"preprocess writes bf16 or fp32, got {dtype}")
    scale, bias = _f32x3(scale), _f32x3(bias)
    if out is None:
        out = torch.empty((N, OH, OW, 3), dtype=dtype, device=src_u8.device).permute(0, 3, 1, 2)
    elif tuple(out.shape) != (N, 3, OH, OW) or out.dtype != dtype or out.device != src_u8.device \
            or not out.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError(f"out must be a channels_last {dtype} [{N}, 3, {OH}, {OW}] tensor on {src_u8.device}")
    if colour is not None and (colour.dtype != torch.float32 or tuple(colour.shape) != (N, 5)
                               or not colour.is_contiguous() or colour.device != src_u8.device):
        raise ValueError(f"colour must be a contiguous float32 [{N}, 5] table on {src_u8.device}, got {colour.dtype} "
                         f"{tuple(colour.shape)} on {colour.device}")
    if not src_u8.is_cuda:
        if src_u8.dtype != torch.uint8:
            raise TypeError(f"src must be uint8, got {src_u8.dtype}")
        if max(H, W, OH, OW) > MAX_DIM:
            raise ValueError(f"H, W, OH, OW must be at most {MAX_DIM}")
        out.permute(0, 2, 3, 1).copy_(_preprocess_cpu(src_u8, boxes, OH, OW, scale, bias, colour))
        return out
    if colour is None:
        rc = _lib.lib().tony_image_preprocess(src_u8.data_ptr(), int(src_u8.dtype == torch.uint8), boxes.data_ptr(),
                                              out.data_ptr(), int(dtype == torch.bfloat16), N, H, W, OH, OW, *scale,
                                              *bias, _lib.stream_ptr(src_u8.device))
        _lib.check(rc, "tony_image_preprocess")
        return out
    if colour_has_contrast and scratch is None:
        scratch = torch.empty(colour_scratch_floats(N, OH, OW), dtype=torch.float32, device=src_u8.device)
    if scratch is not None and (scratch.dtype != torch.float32 or not scratch.is_contiguous()
                                or scratch.device != src_u8.device):
        raise ValueError(f"scratch must be a contiguous float32 buffer on {src_u8.device}, got {scratch.dtype} on "
                         f"{scratch.device}")
    rc = _lib.lib().tony_image_preprocess_colour(
        src_u8.data_ptr(), int(src_u8.dtype == torch.uint8), boxes.data_ptr(), colour.data_ptr(),
        int(bool(colour_has_contrast)), _lib.ptr(scratch), 0 if scratch is None else scratch.numel(), out.data_ptr(),
        int(dtype == torch.bfloat16), N, H, W, OH, OW, *scale, *bias, _lib.stream_ptr(src_u8.device))
    _lib.check(rc, "tony_image_preprocess_colour")
    return out


# -- host-side box samplers (numpy only) ------------------------------------------------------------------

ATTEMPTS = 100  # TF sample_distorted_bounding_box's max_attempts


def validate_boxes(table: np.ndarray, H: int, W: int) -> np.ndarray:
    """Refuse a box table with a box outside the ``H x W`` image (checked on the host, before the copy)."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 5 or t.dtype != np.int32:
        raise ValueError(f"box table must be int32 [N, 5], got {t.dtype} {t.shape}")
    y0, x0, h, w, flip = t.T
    bad = (y0 < 0) | (x0 < 0) | (h < 1) | (w < 1) | (y0.astype(np.int64) + h > H) | (x0.astype(np.int64) + w > W) \
        | (flip < 0) | (flip > 1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"box {i} = {t[i].tolist()} does not lie inside the {H} x {W} image")
    return t


def validate_colour(table: np.ndarray) -> np.ndarray:
    """Refuse a colour table with an order outside -1..5, a non-finite value or a factor <= 0 (checked on the
    host, before the copy)."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 5 or t.dtype != np.float32:
        raise ValueError(f"colour table must be float32 [N, 5], got {t.dtype} {t.shape}")
    order, _, fs, _, fc = t.T
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(t).all(axis=1) | (order != np.floor(order)) | (order < -1) | (order > 5) | ~(fs > 0) \
            | ~(fc > 0)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"colour row {i} = {t[i].tolist()}: the order must be an integer in -1..5, every value "
                         f"finite and both factors > 0")
    return t


def inception_colour_params(rng: np.random.Generator, n: int, fast: bool = False) -> np.ndarray:
    """TF-slim ``inception_preprocessing``'s colour distortion as a float32 ``[n, 5]`` table: order uniform over
    {0, 1, 2, 3}, brightness delta in [-32/255, 32/255), saturation and contrast factors in [0.5, 1.5), hue delta
    in [-0.2, 0.2).  ``fast``: the order is 4 (brightness, saturation), hue is stored as 0 and contrast as 1."""
    order = rng.integers(0, 4, size=n)
    db = rng.uniform(-32 / 255, 32 / 255, size=n)
    fs = rng.uniform(0.5, 1.5, size=n)
    dh = rng.uniform(-0.2, 0.2, size=n)
    fc = rng.uniform(0.5, 1.5, size=n)
    if fast:
        order, dh, fc = np.full(n, 4), np.zeros(n), np.ones(n)
    table = np.stack([order, db, fs, dh, fc], axis=1).astype(np.float32)
    # the cast to fp32 may round a draw just under an open end onto it: keep the ranges half-open
    table[:, 1] = np.clip(table[:, 1], np.float32(-32 / 255), np.nextafter(np.float32(32 / 255), np.float32(0)))
    table[:, 2] = np.minimum(table[:, 2], np.nextafter(np.float32(1.5), np.float32(0)))
    table[:, 3] = np.minimum(table[:, 3], np.nextafter(np.float32(0.2), np.float32(0)))
    table[:, 4] = np.minimum(table[:, 4], np.float32(1.0) if fast else np.nextafter(np.float32(1.5), np.float32(0)))
    return validate_colour(table)


def _distorted_boxes(rng: np.random.Generator, n: int, H: int, W: int, area, ratio=(3 / 4, 4 / 3)) -> np.ndarray:
    """TF ``sample_distorted_bounding_box``'s contract over the whole image: up to ATTEMPTS draws of an aspect
    ratio (w / h) in ``ratio`` and an area fraction in ``area``; the first whose rounded (h, w) fits the image
    is placed uniformly, a sample whose attempts all fail gets the whole image.  Flip with probability 1/2."""
    ar = rng.uniform(ratio[0], ratio[1], size=(n, ATTEMPTS))
    target = rng.uniform(area[0], area[1], size=(n, ATTEMPTS)) * (H * W)
    uy, ux, uf = rng.random(n), rng.random(n), rng.random(n)
    h = np.rint(np.sqrt(target / ar)).astype(np.int64)
    w = np.rint(np.sqrt(target * ar)).astype(np.int64)
    ok = (h >= 1) & (w >= 1) & (h <= H) & (w <= W)
    first = np.argmax(ok, axis=1)
    found = ok[np.arange(n), first]
    h = np.where(found, h[np.arange(n), first], H)
    w = np.where(found, w[np.arange(n), first], W)
    y0 = np.minimum((uy * (H - h + 1)).astype(np.int64), H - h)
    x0 = np.minimum((ux * (W - w + 1)).astype(np.int64), W - w)
    table = np.stack([y0, x0, h, w, (uf < 0.5).astype(np.int64)], axis=1).astype(np.int32)
    return validate_boxes(table, H, W)


def inception_train_boxes(rng: np.random.Generator, n: int, H: int, W: int) -> np.ndarray:
    """Inception's training crop: area fraction in [0.05, 1], aspect ratio in [3/4, 4/3], random flip."""
    return _distorted_boxes(rng, n, H, W, (0.05, 1.0))


def resnet_train_boxes(rng: np.random.Generator, n: int, H: int, W: int) -> np.ndarray:
    """ResNet's training crop: area fraction in [0.08, 1], aspect ratio in [3/4, 4/3], random flip."""
    return _distorted_boxes(rng, n, H, W, (0.08, 1.0))


def central_boxes(n: int, H: int, W: int, fraction: float = 0.875) -> np.ndarray:
    """The evaluation crop (TF ``central_crop``): ``y0 = int((H - H*fraction) / 2)``, ``h = H - 2*y0``, columns
    alike; never flipped."""
    if not 0 < fraction <= 1:
        raise ValueError(f"fraction must be in (0, 1], got {fraction}")
    y0, x0 = int((H - H * fraction) / 2), int((W - W * fraction) / 2)
    table = np.tile(np.array([[y0, x0, H - 2 * y0, W - 2 * x0, 0]], dtype=np.int32), (n, 1))
    return validate_boxes(table, H, W)
