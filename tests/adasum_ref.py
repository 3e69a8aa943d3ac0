"""Shared by the Adasum tests (test_adasum_cpu.py, test_adasum_gpu.py, test_adasum_ranks_gpu.py): the contract of
``tony_amd.ops.adasum`` in numpy, a float64 reference of the rank tree that carries a magnitude and an error bound
beside every value, and inputs for which that bound means something.

The contract.  Combining ``a`` and ``b`` of one parameter tensor (``a`` the lower rank's side):

    dot = sum a_i b_i      na = sum a_i^2      nb = sum b_i^2        (every product exact in double, summed in double)
    ca  = fl32(1 - dot / (2 na))   if na >= sqrt(DBL_MIN), else 1      (formed in double, rounded once)
    cb  = fl32(1 - dot / (2 nb))   if nb >= sqrt(DBL_MIN), else 1
    out_i = fl32(fl32(ca a_i) + fl32(cb b_i))                          (no fused multiply-add)

a bf16 buffer is read as bf16 and ``out_i`` rounded once more, to bf16, nearest-even.  ``N`` ranks, a power of two:
level d = 1, 2, 4, ... combines rank r's value with rank ``r ^ d``'s, so ``adasum(g0..g3) = combine(combine(g0, g1),
combine(g2, g3))``, with one coefficient pair per parameter tensor and level.  ``combine_np`` / ``tree_np`` are that,
operation for operation (numpy rounds every float32 operation on its own); only the ORDER of the double sums is free, so
code that follows the contract agrees with them bit for bit whenever the two orders round ``ca`` and ``cb`` alike.

The reference and the bound.  ``tree_ref`` computes the tree in float64 and carries, for every tensor of every node,

    mag   a leaf has mag = |g|; a combine has mag = |ca| mag_a + |cb| mag_b  (elementwise, mag >= |value|)
    K     the error of a value computed under the contract is at most K e mag elementwise, e = 2^-24

Errors are judged against ``e mag`` and not against the result: results cancel across levels, the errors of earlier
levels do not.  A leaf is exact, K = 0.  A combine of inputs that are off by at most ``Ka e mag_a`` and ``Kb e mag_b``
counts, for the a side (the b side alike), all per unit of ``e |ca| mag_a``:

    Ka      the input's own error, scaled by ca like the input
    1       the rounding of ca to fp32: e |ca|, times |a_i| <= mag_a
    2       the two roundings that touch the a side: fl32(ca a_i), and the a side's share of the sum's rounding (the
            sum rounds once, on a magnitude <= |ca a_i| + |cb b_i|)
    S_a     the sensitivity of ca to the errors of BOTH inputs:  ca = 1 - dot / (2 na) moves by at most
                s_a = D / (2 na) + |dot| N_a / (2 na^2)
                D   = e (Ka sum mag_a |b| + Kb sum |a| mag_b) + g sum mag_a mag_b       (the error of dot)
                N_a = 2 e Ka sum mag_a |a| + g sum mag_a^2                             (the error of na)
            with g = n 2^-53 for the n additions of a double sum in any order; it moves out_i by s_a |a_i|, which is
            S_a = s_a / (e |ca|) in these units.  The sums over the actual vectors are taken by the reference (Cauchy-
            Schwarz would replace them by products of norms and lose a factor of the dimension's square root for
            nothing)

    K' = max(Ka + S_a, Kb + S_b) + 3 + R          K_out = K' (1 + 2 K' e)^4

``R`` is the rounding of the output to its buffer's format: 0 for fp32; for bf16 the half ulp of the output, 2^-8 of
its magnitude, R = 2^16.  The last factor covers the products of small terms dropped above (each of the four places
where a computed quantity stood in for an exact one is off by a factor within 1 + 2 K' e).  Without the sensitivities
the count is 3 per level, 9 after three levels; with them it depends on the inputs through ``|dot| / na`` and
``1 / |ca|``, so the inputs of the tests (``make_grads``) keep every pairwise cosine within about [-0.5, 0.9] and
every ratio of norms within [0.5, 2], which puts every coefficient of every level in [0.1, 1.5], away from zero.  For
such inputs K comes in fp32 to 3 after one level, 10 to 15 after two (up to 37 for tensors of 4 and 7 elements) and
65 to 70 after three (130 to 190 for those two); in bf16 R + 3 takes the place of the 3 (1.03 R, about 6 R, about
55 R).  test_adasum_cpu.py prints it beside the measured error: the numpy transcription of the contract measured at most 3.5 e mag over three
levels there (4.1 over n from 5 to 10^6), so the bound sits 3 to 20 times above what is measured on tensors of 4096
elements and more, and is looser only on the tiny ones.
"""
import math

import numpy as np
import torch

EPS = 2.0 ** -24
R_BF16 = 2.0 ** 16          # half an ulp of bf16, 2^-8, in units of EPS
TINY = 1.4916681462400413e-154  # sqrt(DBL_MIN)
LENGTHS = [4, 7, 4096, 4100, 3 * 4096 + 8]  # one item, an item and a 4-element tail, several items, two tiny tensors
ALIGN = 64                  # the flat buffers' slot alignment


def to_bf16(x):
    """float32 values rounded to bf16 (nearest-even), as float32."""
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def layout(lengths=LENGTHS, align=ALIGN):
    """(offsets, segments, total): tensors at multiples of ``align``; a segment runs to the next tensor's offset (the
    padding belongs to the tensor before it), as ``parallel.flat.build_segments`` lays a flat buffer out."""
    offs, n = [], 0
    for ln in lengths:
        offs.append(n)
        n += (ln + align - 1) // align * align
    return offs, list(zip(offs, offs[1:] + [n])), n


def coefs(a, b):
    """(ca, cb) as float32 from float32 (or bf16-valued float32) vectors: exact products, double sums."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dot, na, nb = float(a64 @ b64), float(a64 @ a64), float(b64 @ b64)
    ca = np.float32(1.0 - dot / (2.0 * na)) if na >= TINY else np.float32(1.0)
    cb = np.float32(1.0 - dot / (2.0 * nb)) if nb >= TINY else np.float32(1.0)
    return ca, cb


def apply_np(a, b, ca, cb, bf16=False):
    """``fl32(fl32(ca a) + fl32(cb b))`` (then bf16) of float32 arrays with given float32 coefficients."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    out = (np.float32(ca) * a).astype(np.float32) + (np.float32(cb) * b).astype(np.float32)
    return to_bf16(out) if bf16 else out.astype(np.float32)


def combine_np(a, b, segs, bf16=False):
    """The contract's combine of two flat float32 arrays, tensor by tensor of ``segs`` ((lo, hi) pairs)."""
    out = np.empty_like(a, dtype=np.float32)
    for lo, hi in segs:
        ca, cb = coefs(a[lo:hi], b[lo:hi])
        out[lo:hi] = apply_np(a[lo:hi], b[lo:hi], ca, cb, bf16)
    return out


def _tree(vals, combine):
    cur, n, d = list(vals), len(vals), 1
    assert n >= 1 and n & (n - 1) == 0
    while d < n:
        for r in range(0, n, 2 * d):
            cur[r] = combine(cur[r], cur[r + d])  # r < r + d = r ^ d: the lower rank's side is a
        d *= 2
    return cur[0]


def tree_np(grads, segs, bf16=False):
    """The contract over the ranks' flat float32 gradients (bf16: already bf16-valued)."""
    return _tree([np.asarray(g, dtype=np.float32) for g in grads], lambda a, b: combine_np(a, b, segs, bf16))


class Ref:
    """One node of the float64 tree: ``val``, ``mag`` (arrays) and ``K`` (one per tensor of ``segs``); ``coefs`` lists
    every (ca, cb) met below and at this node."""

    def __init__(self, val, mag, K, coefs=()):
        self.val, self.mag, self.K, self.coefs = val, mag, K, list(coefs)

    def bound(self, segs):
        """The elementwise error bound ``K e mag``."""
        out = np.empty_like(self.mag)
        for k, (lo, hi) in zip(self.K, segs):
            out[lo:hi] = k * EPS * self.mag[lo:hi]
        return out


def _combine_ref(A, B, segs, R):
    val, mag = np.empty_like(A.val), np.empty_like(A.mag)
    K, cs = [], []
    for t, (lo, hi) in enumerate(segs):
        a, b, ma, mb = A.val[lo:hi], B.val[lo:hi], A.mag[lo:hi], B.mag[lo:hi]
        Ka, Kb = A.K[t], B.K[t]
        dot, na, nb = float(a @ b), float(a @ a), float(b @ b)
        g = (hi - lo) * 2.0 ** -53
        D = EPS * (Ka * float(ma @ np.abs(b)) + Kb * float(np.abs(a) @ mb)) + g * float(ma @ mb)
        side = []
        for nn, m, x, Kx in ((na, ma, a, Ka), (nb, mb, b, Kb)):
            if nn < TINY:
                side.append((1.0, Kx))  # a zero side: the coefficient is 1 on both sides of the comparison
                continue
            c = 1.0 - dot / (2.0 * nn)
            N = 2.0 * EPS * Kx * float(m @ np.abs(x)) + g * float(m @ m)
            s = D / (2.0 * nn) + abs(dot) * N / (2.0 * nn * nn)
            side.append((c, Kx + s / (EPS * max(abs(c), 1e-300))))
        (ca, ka), (cb, kb) = side
        k = max(ka, kb) + 3.0 + R
        k *= (1.0 + 2.0 * k * EPS) ** 4
        val[lo:hi] = ca * a + cb * b
        mag[lo:hi] = abs(ca) * ma + abs(cb) * mb
        K.append(k)
        cs.append((ca, cb))
    return Ref(val, mag, K, A.coefs + B.coefs + cs)


def tree_ref(grads, segs, bf16=False):
    """The float64 tree over the ranks' gradients (the values the contract starts from: bf16-valued for a bf16
    buffer), as a ``Ref``."""
    R = R_BF16 if bf16 else 0.0
    leaves = [Ref(np.asarray(g, dtype=np.float64), np.abs(np.asarray(g, dtype=np.float64)), [0.0] * len(segs))
              for g in grads]
    return _tree(leaves, lambda A, B: _combine_ref(A, B, segs, R))


def measured(got, ref, segs):
    """Per tensor: max |got - ref| / (e mag) over the elements with mag > 0 (where mag is 0 the value must be 0)."""
    out = []
    for lo, hi in segs:
        m = ref.mag[lo:hi]
        err = np.abs(np.asarray(got[lo:hi], dtype=np.float64) - ref.val[lo:hi])
        assert (err[m == 0] == 0).all()
        out.append(float((err[m > 0] / (EPS * m[m > 0])).max()) if (m > 0).any() else 0.0)
    return out


def make_grads(world, lengths=LENGTHS, seed=0, bf16=False, align=ALIGN):
    """``world`` flat float32 gradients over ``layout(lengths)``, zero on the padding: correlated Gaussians (a shared
    part and a part of each rank's own, scaled per rank within [0.75, 1.4]), every tensor redrawn until every
    coefficient of every level of its float64 tree lies in [0.1, 1.5]."""
    offs, segs, n = layout(lengths, align)
    out = [np.zeros(n, dtype=np.float32) for _ in range(world)]
    scales = [1.0, 1.4, 0.75, 1.2, 0.9, 1.3, 0.8, 1.1]
    for t, (off, ln) in enumerate(zip(offs, lengths)):
        for attempt in range(1000):
            rng = np.random.default_rng([seed, t, attempt])
            common = rng.standard_normal(ln)
            gs = [(scales[r % 8] * (common + rng.standard_normal(ln))).astype(np.float32) for r in range(world)]
            if bf16:
                gs = [to_bf16(g) for g in gs]
            cs = tree_ref(gs, [(0, ln)]).coefs if world > 1 else []
            if all(0.1 <= c <= 1.5 for pair in cs for c in pair):
                break
        else:
            raise AssertionError(f"no draw of tensor {t} ({ln} elements) keeps its coefficients in [0.1, 1.5]")
        for r in range(world):
            out[r][off:off + ln] = gs[r]
    return out, segs


def fsum_triple(a, b):
    """(a.b, a.a, b.b) of float32 vectors, correctly rounded (``math.fsum`` of the exact double products), and the
    sums of the products' magnitudes."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    prods = (a64 * b64, a64 * a64, b64 * b64)
    return [math.fsum(p) for p in prods], [math.fsum(np.abs(p)) for p in prods]
