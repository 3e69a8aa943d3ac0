"""Image input pipeline: uint8 NHWC batch + per-sample crop boxes -> the model's channels_last input in one
launch (HIP kernel in csrc/image.hip), and the host-side box samplers that fill the box table.

``out = bilinear(crop) * scale[c] + bias[c]`` with torch's ``bilinear, align_corners=False, antialias=False``
positions, formed as exact rationals: for output row ``oy`` of a crop ``h`` rows high,
``num = max((2*oy+1)*h - OH, 0)``, ``iy0 = num // (2*OH)``, ``ly = float(num % (2*OH)) / float(2*OH)``,
``iy1 = min(iy0+1, h-1)``; columns alike, and with ``flip`` column ``ox`` samples position ``OW-1-ox``.
On CPU tensors (local-mode jobs) a torch implementation of the same formula in fp32 is used.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_DIM = 4096  # csrc/image.hip kMaxDim: (2*o+1)*h stays inside int32

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


def _preprocess_cpu(src, boxes, OH: int, OW: int, scale, bias) -> torch.Tensor:
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
    return v * torch.tensor(scale, dtype=torch.float32) + torch.tensor(bias, dtype=torch.float32)


def preprocess(src_u8: torch.Tensor, boxes: torch.Tensor, size, dtype=torch.bfloat16, scale=1.0, bias=0.0,
               out: torch.Tensor = None) -> torch.Tensor:
    """The channels_last ``[N, 3, OH, OW]`` input of ``dtype`` (bf16 / fp32) from the dense uint8 ``src_u8``
    ``[N, H, W, 3]`` and the int32 box table ``boxes`` ``[N, 5]`` of ``(y0, x0, h, w, flip)`` on the same device.
    ``out``: a channels_last ``[N, 3, OH, OW]`` tensor to write into (one persistent buffer across steps)."""
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
    if not src_u8.is_cuda:
        if src_u8.dtype != torch.uint8:
            raise TypeError(f"src must be uint8, got {src_u8.dtype}")
        if max(H, W, OH, OW) > MAX_DIM:
            raise ValueError(f"H, W, OH, OW must be at most {MAX_DIM}")
        out.permute(0, 2, 3, 1).copy_(_preprocess_cpu(src_u8, boxes, OH, OW, scale, bias))
        return out
    rc = _lib.lib().tony_image_preprocess(src_u8.data_ptr(), int(src_u8.dtype == torch.uint8), boxes.data_ptr(),
                                          out.data_ptr(), int(dtype == torch.bfloat16), N, H, W, OH, OW, *scale, *bias,
                                          _lib.stream_ptr(src_u8.device))
    _lib.check(rc, "tony_image_preprocess")
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
