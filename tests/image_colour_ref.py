"""Shared by the colour-distortion tests (test_image_colour_cpu.py, test_image_colour_gpu.py): a float64
reference of ``ops.image.preprocess(..., colour=table)`` written from the contract, its error bound, and colour
tables that hold every order code with parameters at both ends of their ranges and inside them.

The contract.  ``v`` is the bilinear value in [0, 255] after the crop box and the flip.  A row of the float32
table ``[N, 5]`` is ``(order, brightness delta, saturation factor, hue delta, contrast factor)``.  A sample with
order -1 writes ``v * scale_c + bias_c``.  Any other sample computes ``u = v / 255``, applies the ops of its order
(``ORDERS``), clips to [0, 1] and writes ``u * (255 * scale_c) + bias_c``.  With ``M = max``, ``m = min``,
``R = M - m`` of a pixel, ``h6`` in [0, 6) (0 if ``R == 0``; ``(g-b)/R``, +6 if negative, if ``M == r``;
``(b-r)/R + 2`` if ``M == g``; else ``(r-g)/R + 4``) and ``d_r = clamp(|h6-3| - 1, 0, 1)``,
``d_g = clamp(2 - |h6-2|, 0, 1)``, ``d_b = clamp(2 - |h6-4|, 0, 1)``:

    b  brightness   x_c + delta
    s  saturation   R' = max(0, min(R*f, M));  (M - R') + R' * d_c(h6)
    h  hue          h6' = (h6 + 6*delta) mod 6 in [0, 6);  m + R * d_c(h6')
    c  contrast     (x_c - mean_c) * f + mean_c, mean_c the mean over the sample's OH x OW output pixels of the
                    unclipped value entering the contrast stage

The bound, counted the way ``image_ref.bound`` is: fp32 roundings x 2^-24 x the magnitude of the rounded value,
in [0, 1] units, in multiples of e = 2^-24.

    u = v / 255       the 14 roundings of the bilinear value on a magnitude <= 255 (image_ref.bound), divided by
                      255, and the division's own: 15 e.
    brightness        one addition on a magnitude <= 1 + 32/255 (1.125 from here on): 1.125 e.
    h6                g - b, R = M - m and the quotient, on a fraction <= 1: 3 e; the sextant offset on a magnitude
                      < 6: 6 e.  9 e.
    d_c               |h6 - k| on a magnitude <= 4 and the subtraction from 2 (or of 1) on one <= 2: 6 e more.
    saturation        d_c off by 9 + 6 = 15 e, times R' <= 1.125: 16.9 e; R' itself (R, R*f: 2 roundings on
                      <= 1.125, times |1 - d_c| <= 1): 2.25 e; M - R' and the multiply-add: 2.25 e.  21.4 e.
    hue               h6 + 6*delta (one multiply-add on a magnitude < 7.2) and the reduction into [0, 6) (at most one
                      rounding on a magnitude < 6): h6' off by 9 + 7.2 + 6 = 22.2 e, d_c by 28.2 e, times R <= 1.125:
                      31.7 e; R's rounding and the multiply-add: 2.25 e.  34 e.
    contrast          the mean: the fp32 values are summed in float64 and rounded to fp32 once per stored partial and
                      once at the end, so it is off by 2 x 1.125 e, and enters with |1 - f| <= 0.5: 1.125 e; x - mean
                      on a magnitude <= 2.25, times f <= 1.5: 3.4 e; the multiply-add on a magnitude <= 3: 3 e.  7.5 e.

A full order (0..3) has all four: 15 + 1.125 + 21.4 + 34 + 7.5 = 79 e, taken as 80 e; a fast order (4, 5) has
brightness and saturation: 15 + 1.125 + 21.4 = 37.5 e, taken as 38 e.  The clip adds nothing.  The output
``u * (255 scale_c) + bias_c`` multiplies that by ``|255 scale_c|`` (whose own rounding is one more e of it) and
rounds once on a magnitude <= ``|255 scale_c| + |bias_c|``:

    B_c = (E + 1) e |255 scale_c| + e (|255 scale_c| + |bias_c|),   E = 80 (orders 0..3) or 38 (orders 4, 5)

and a sample of order -1 keeps ``image_ref.bound``.  For bf16 add ``halfulp_bf16(ref)``.  The count treats each
op as passing on the error it receives unamplified (every op is piecewise linear in the pixel with slopes about
one); a plain fp32 transcription measured 13.6 e over these tests' geometries and all six orders, a sixth of E.
"""
import numpy as np
import torch

import image_ref
from image_ref import f32, halfulp_bf16

ORDERS = {-1: "", 0: "bshc", 1: "sbch", 2: "chbs", 3: "hscb", 4: "bs", 5: "sb"}
E_FULL, E_FAST = 80.0, 38.0
EPS = 2.0 ** -24

B_LO, B_HI = -32 / 255, 32 / 255  # brightness delta
F_LO, F_HI = 0.5, 1.5  # saturation and contrast factors
H_LO, H_HI = -0.2, 0.2  # hue delta


def _hue6(x):
    """(M, m, R, h6) of float64 pixels [..., 3]."""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    M, m = x.max(-1), x.min(-1)
    R = M - m
    safe = np.where(R == 0, 1.0, R)
    hr = (g - b) / safe
    hr = np.where(hr < 0, hr + 6.0, hr)
    h6 = np.where(M == r, hr, np.where(M == g, (b - r) / safe + 2.0, (r - g) / safe + 4.0))
    return M, m, R, np.where(R == 0, 0.0, h6)


def _weights(h6):
    d = np.stack([np.abs(h6 - 3.0) - 1.0, 2.0 - np.abs(h6 - 2.0), 2.0 - np.abs(h6 - 4.0)], -1)
    return np.clip(d, 0.0, 1.0)


def distort(x, ops, db, fs, dh, fc):
    """The ops of one sample on its float64 pixels [OH, OW, 3] in [0, 1] units, unclipped."""
    for op in ops:
        if op == "b":
            x = x + db
        elif op == "s":
            M, _, R, h6 = _hue6(x)
            Rp = np.maximum(0.0, np.minimum(R * fs, M))
            x = (M - Rp)[..., None] + Rp[..., None] * _weights(h6)
        elif op == "h":
            _, m, R, h6 = _hue6(x)
            x = m[..., None] + R[..., None] * _weights(np.mod(h6 + 6.0 * dh, 6.0))
        else:
            mean = x.mean((0, 1))
            x = (x - mean) * fc + mean
    return x


def reference(src, boxes, colour, size, scale, bias):
    """float64 [N, 3, OH, OW] of the contract; the table's fp32 values and the fp32 constants widened to float64."""
    plain = image_ref.reference(src, boxes, size, scale, bias)
    v = image_ref.reference(src, boxes, size, (1.0,) * 3, (0.0,) * 3).permute(0, 2, 3, 1).numpy()  # exact constants
    k = (255.0 * f32(scale)).numpy()  # the fp32 product 255 * scale_c differs from this by one rounding: in B_c
    out = plain.clone()
    for n, row in enumerate(colour.cpu().to(torch.float64).tolist()):
        ops = ORDERS[int(row[0])]
        if ops:
            u = np.clip(distort(v[n] / 255.0, ops, *row[1:]), 0.0, 1.0)
            out[n] = torch.from_numpy(u * k + f32(bias).numpy()).permute(2, 0, 1)
    return out


def bound(colour, scale, bias):
    """B [N, 3, 1, 1] (module docstring): per sample by its order, per channel by the normalisation."""
    k, b = 255 * f32(scale).abs(), f32(bias).abs()
    plain = image_ref.bound(scale, bias)[0]  # [3, 1, 1]
    rows = []
    for order in colour[:, 0].tolist():
        if int(order) < 0:
            rows.append(plain)
        else:
            e = E_FULL if int(order) <= 3 else E_FAST
            rows.append((((e + 1) * k + (k + b)) * EPS)[:, None, None])
    return torch.stack(rows)


def assert_close(got, ref, colour, scale, bias, what):
    """fp32: |got - ref| <= B; bf16: |got - ref| <= halfulp_bf16(ref) + B.  Returns the worst error / bound."""
    lim = bound(colour, scale, bias).expand_as(ref)
    if got.dtype == torch.bfloat16:
        lim = lim + halfulp_bf16(ref)
    err = (got.detach().cpu().to(torch.float64) - ref).abs()
    over = err > lim
    worst = float((err / lim).max())
    print(f"{what}: max |got - ref| / bound = {worst:.4f}")
    assert not bool(over.any()), \
        f"{what}: {int(over.sum())} of {err.numel()} elements over the bound (worst {worst:.3f}x)"
    return worst


def colour_tables(N, seed=0):
    """float32 [N, 5] tables in which every row of a table has a different order where N allows it, every code
    -1..5 occurs over the tables, and the parameters sit at both ends of their ranges and inside them."""
    rng = np.random.default_rng(seed)
    top = [np.nextafter(np.float32(v), np.float32(0)) for v in (B_HI, F_HI, H_HI, F_HI)]  # the open ends
    rows = []
    for i, order in enumerate([0, 1, 2, 3, 4, 5, -1]):
        kind = i % 3
        if kind == 0:
            p = [B_LO, F_LO, H_LO, F_LO]
        elif kind == 1:
            p = top
        else:
            p = [rng.uniform(B_LO, B_HI), rng.uniform(F_LO, F_HI), rng.uniform(H_LO, H_HI), rng.uniform(F_LO, F_HI)]
        rows.append([order] + list(p))
    # the opposite ends for the full orders, and mixed ends
    rows += [[0] + list(top), [1, B_LO, F_HI, H_HI, F_LO], [2, B_HI, F_LO, H_LO, F_HI], [3, B_LO, F_LO, H_HI, F_HI],
             [4] + list(top), [5, B_LO, F_LO, 0.0, 1.0]]
    while len(rows) % N:
        rows.append([len(rows) % 6, rng.uniform(B_LO, B_HI), rng.uniform(F_LO, F_HI), rng.uniform(H_LO, H_HI),
                     rng.uniform(F_LO, F_HI)])
    return [torch.tensor(np.array(rows[i:i + N], dtype=np.float32)) for i in range(0, len(rows), N)]


ADVERSARIAL = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (1, 0, 0),
               (255, 255, 0), (0, 255, 255), (254, 255, 255)]


def adversarial_pixels(src):
    """A copy of ``src`` [N, H, W, 3] with the adversarial pixels written over the start of every image, each as a
    run of two so that a crop also samples them unmixed."""
    out = src.clone()
    flat = out.view(out.shape[0], -1, 3)
    for i, px in enumerate(ADVERSARIAL):
        if 2 * i + 2 <= flat.shape[1]:
            flat[:, 2 * i:2 * i + 2] = torch.tensor(px, dtype=torch.uint8)
    return out
