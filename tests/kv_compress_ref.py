"""The kvstore's 2-bit gradient compression in numpy, elementwise on float32 arrays -- the one reference of
test_kv_compress_cpu.py and test_kv_compress_gpu.py (the torch implementation in parallel/kvstore.py is code
under test, like the kernels).

A worker keeps a residual ``r`` per key (zero before the first push).  A push of ``g``, every line one IEEE
fp32 operation::

    t = r + g
    if   t >=  thr: code = 1; r = t - thr
    elif t <= -thr: code = 2; r = t + thr
    else:           code = 0; r = t          (a NaN t compares false twice)

Element ``i`` is bits ``2 * (i & 15)`` and ``2 * (i & 15) + 1`` of u32 word ``i >> 4``; ``ceil(n / 16)`` words, the
unused pairs of the last one 0.  Codes decode 0 -> 0.0, 1 -> +thr, 2 -> -thr, 3 -> 0.0.
"""
import numpy as np


def n_words(n):
    return (n + 15) // 16


def quantise(g, r, thr):
    """(words uint32 [ceil(n/16)], new residual float32 [n]) of pushing ``g`` on residual ``r``."""
    g, r, thr = np.asarray(g, np.float32), np.asarray(r, np.float32), np.float32(thr)
    assert g.ndim == 1 and g.shape == r.shape
    with np.errstate(invalid="ignore", over="ignore"):
        t = r + g
        pos, neg = t >= thr, t <= -thr
        new_r = np.where(pos, t - thr, np.where(neg, t + thr, t)).astype(np.float32)
    code = np.where(pos, 1, np.where(neg, 2, 0)).astype(np.uint32)
    words = np.zeros(n_words(g.size), np.uint32)
    for i in range(16):  # element 16 w + i: bits 2 i, 2 i + 1 of word w
        part = code[i::16]
        words[:part.size] |= part << np.uint32(2 * i)
    return words, new_r


def codes(words, n):
    words = np.asarray(words, np.uint32)
    c = np.empty((words.size, 16), np.uint32)
    for i in range(16):
        c[:, i] = (words >> np.uint32(2 * i)) & np.uint32(3)
    return c.reshape(-1)[:n]


def decode(words, n, thr):
    """float32 [n]: the values one packed push stands for."""
    thr = np.float32(thr)
    lut = np.array([0.0, thr, -thr, 0.0], np.float32)
    return lut[codes(words, n)]


def merge(pushes, n, thr):
    """The ordered fp32 sum a receiver forms of several packed pushes: ``acc = v_0; acc += v_1; ...``."""
    acc = decode(pushes[0], n, thr).copy()
    for w in pushes[1:]:
        acc += decode(w, n, thr)
    return acc


def specials(thr):
    """The edge values every test puts at the front of its gradient (42 values): the thresholds and their
    neighbours, zeros, infinities, NaN, denormals and values past the threshold."""
    t = np.float32(thr)
    inf = np.float32(np.inf)
    v = [t, -t, np.nextafter(t, np.float32(0)), np.nextafter(-t, np.float32(0)), np.nextafter(t, inf),
         np.nextafter(-t, -inf), 0.0, -0.0, inf, -inf, np.nan, 1e-40, -1e-40, 3 * t, -3 * t]
    # each once against a zero residual slot and twice more so that the chained pushes meet them with residuals
    return np.array(v + v[::-1] + v[:12], np.float32)


def gradient(n, thr, seed, with_specials=True):
    """``0.7 * thr * randn`` (all three codes common), the special values in its first elements."""
    rng = np.random.default_rng(seed)
    g = (np.float32(0.7) * np.float32(thr) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    if with_specials:
        s = specials(thr)
        g[:min(n, s.size)] = s[:n]
    return g


def sgd_update(w, merged, lr, rescale):
    """``Optimizer.update`` of plain sgd (no momentum, wd 0, no clip) in fp32: w += -lr * (merged * rescale)."""
    g = (np.asarray(merged, np.float32) * np.float32(rescale)).astype(np.float32)
    g = (g + np.float32(0.0) * w).astype(np.float32)  # g.add_(w, alpha=wd) with wd = 0
    return (w + np.float32(-lr) * g).astype(np.float32)
