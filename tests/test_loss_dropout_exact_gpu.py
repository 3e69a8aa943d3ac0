"""Exact and bounded tests of the cross-entropy (csrc/loss.hip) and dropout (csrc/dropout.hip) kernels.

``tony_xent_fwd`` / ``tony_xent_bwd`` / ``tony_dropout_fwd`` / ``tony_dropout_bwd`` / ``tony_counter_bump`` are
called directly, on operands that live as slices of poisoned allocations, and compared with references written
from the definition: float64 on the CPU for the loss, a numpy ``uint64`` model of the counter hash for the
dropout mask (never a mask read back from the kernel).  One pass per family goes through the public wrapper.

Cross-entropy
=============
Reference (float64, the STORED bf16 / fp32 logits taken as exact, s = the fp32 value of the smoothing):
    lse = logsumexp(x);  loss = (1-s)(lse - x_t) + s(lse - mean(x));  d = (softmax(x) - (1-s) onehot - s/K) gout
A label outside [0, K) marks an ignored row: loss = 0, lse as always, d = 0 (what
``F.cross_entropy(reduction="none", ignore_index=t)`` gives for that row).  ``reduction="mean"`` divides by N,
ignored rows included (pinned by test_wrapper_ignored_rows_and_mean_over_n).

Exact (``torch.equal``): the ignored rows (loss == 0, d == 0, whatever the smoothing); K = 1 (loss == 0,
lse == x, d == 0); equal logits with K a power of two, s = 0 and gout a power of two, where
d == (1/K - onehot) gout rounded once to the output dtype; K = 4097 refused with -1 and nothing written.

Bounded, with U = 2^-24 (half an fp32 ulp, relative) and every magnitude computed in float64 next to the
reference.  The kernel forms lse = mx + __logf(sum __expf(v - mx)) and p = __expf(x - lse).
  * Intrinsic accuracy.  The HIP headers of the ROCm install define __expf(x) as the hardware exp2 of
    fl(log2e * x) and __logf as the library logf; NO accuracy figure for either is documented anywhere in the
    install.  ASSUMED here: 1 ulp (2 U relative) for the hardware exp2 (the figure the public CDNA ISA
    manuals give for V_EXP_F32 / V_LOG_F32) and 2 ulp for logf; results below 2^-126 may be flushed to 0.
  * sum exp.  The argument of exp2 carries three roundings (v - mx, the constant log2e, the product): 3 U |a|,
    which is a relative 3 U |v - mx| of the term; weighted by the terms themselves that is 3 U E_p|x - mx| <=
    3 U H with H = lse - E_p[x] the softmax entropy (<= ln K).  exp2: 2 U.  The sum is 16 serial + 6 butterfly
    + 3 serial additions of positive terms: 25 U.  A relative error of the sum is an absolute error of its log.
  * log and the final add: 4 U |lse - mx| (2 ulp of the log) + U |lse| (the rounding of mx + log).  The last
    term is counted twice: the plain-fp32 floor below was measured at 1.1 U |lse|, and the bound may not be
    tighter than it at a large |lse|, where the absolute terms do not make up the difference.
        E_lse = U (27 + 3 H + 4 |lse - mx| + 2 |lse|)
    The last term is the cancellation the '+1000' family is dominated by: an fp32 ulp of |lse|.
  * loss.  With A = (1-s)|lse - x_t|, B = s|lse - mean x|: the two differences, two products, 1-s and the final
    add are <= 4 U (A + B); mean x is 25 additions and a division: 26 U mean|x|, times s.
        E_loss = E_lse + U (4 A + 4 B + 26 s mean|x|)
    A masked (-inf) class with s > 0 makes the loss +inf by definition; there got == +inf is required.
  * d.  x - lse inherits E_lse from the STORED lse; the argument adds 3 U |x - lse|, exp2 2 U; the target
    (1-s) onehot + s/K has three roundings, the difference and the product with gout one each:
        E_d = |gout| (p (1.01 (E_lse + 3 U |x - lse|) + 2 U) + 3 U target + 2 U |p - target|) + 2^-125
    (1.01: second order of exp; 2^-125: flush of a p below the normal range).  bf16 d: + 1/2 ulp_bf16(ref).
The bound sits between the two conditions of the issue, asserted by test_cpu_bound_sits_between_floor_and_ceiling
for lse AND loss: never tighter than the plain-fp32 floor 1.1 * 2^-24 * max(1, |lse|) (E_lse >= 27 U + 2 U |lse|),
and at K = 4096 with equal logits (|lse| ~ 9) E_lse = 6.2e-6 and E_loss = 8.3e-6, far below half of
log(4096/4095) = 2.44e-4, so a dropped or doubled class cannot hide.

Sensitivity (test_cpu_xent_*): the float64 reference is mutated the way a wrong kernel would be, and the mutant
must break the assertion the GPU result is held to, at every K used: one class dropped from the sum and the last
class doubled (lse and loss of the equal-logits rows, where the shift is the smallest: log(K/(K-1))); the target
off by one (d at K >= 2; at K = 1 there is no other class); s/(K-1) for s/K (fp32 d at every K >= 2; bf16 d only
for K <= 257 -- beyond that the change, a relative 1/(K-1) of s/K, is below half a bf16 ulp of d and no test of a
bf16 output can see it); gout of the neighbouring row (N = 3, K >= 2: at K = 1 d is 0); the ignored row's gradient
left at p * gout.

Dropout
=======
Host model (numpy uint64, from the header comment and dropout_fwd_kernel): key = mix64(seed ^ mix64(t +
0x632be59bd9b4e019)); group g draws mix64(key + 2g), mix64(key + 2g + 1); element e takes bits 16 (e & 3) of the
first (e < 4) or second draw; keep = r >= thr, thr = uint32(float32(p) * 65536f + 0.5f); scale = 1f / (1f - p).
Exact (bit patterns, so a -0 for a dropped element shows): the n live mask bits, y, dx from dy and a STORED mask
of arbitrary bytes, rng == [seed, t + 1] after the wrapper and unchanged by the bare forward.  A p whose thr
rounds to 65536 (0.999995) drops everything.  Each n also runs with p = r / 65536 of its last live element, so
that one element sits exactly on the threshold and ``>`` for ``>=`` cannot pass.  x 16-byte misaligned: -3,
nothing written.  The statistics (keep rate, agreement between steps and seeds within 5 sigma) are asserted on
the model; the GPU equality carries them over.
Sensitivity (test_cpu_dropout_*): ``>`` for ``>=``, the draws swapped, key + g, scale 1/p and the tail group
shifted by one each break equality at every n (the tail shift at every n % 8 != 0: at n = 8, 2048 there is no
tail group and the mutant is the identity, which is asserted too; key + g at every n > 8: group 0 draws the same
pair either way, so a single group cannot show it).  "Breaks equality at n" means: some (seed, t, p) run of the
GPU test at that n would fail.

Poison.  Operands are slices of NaN allocations, destinations slices of sentinel allocations (mask: 0xA5); no
byte outside a destination changes and no NaN reaches an output.

Largest observed error / bound per family on an MI355X (RECORD below; a record, never a knob;
test_zz_every_loss_and_dropout_entry_point_ran prints the live figures): lse 0.15 - 0.33, loss 0.11 - 0.32,
d 0.14 - 0.62 (the wide family, where p spans 70 decades), wrappers 0.27 / 0.26.  Every exact comparison held,
the fp32 d == (1/K - onehot) gout at K = 64, 256, 4096 included.

Defect this module exposed: with a class masked by -inf and NO smoothing the forward formed
0 * (lse - sum x / K) = 0 * inf and stored a NaN loss; the kernel now leaves the smoothing term out at s = 0.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exact_helpers import SENT, Slab, assert_equal

gpu = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24

# measured on an MI355X by this module (family -> largest error / bound); the bounds stay derived
RECORD = {"lse equal": 0.1463, "lse masked": 0.2096, "lse offset+1000": 0.2483, "lse randn*3": 0.1787,
          "lse wide+-80": 0.3260, "loss equal": 0.1106, "loss masked": 0.1370, "loss offset+1000": 0.2444,
          "loss randn*3": 0.2124, "loss wide+-80": 0.3209, "d equal": 0.1445, "d masked": 0.4168,
          "d offset+1000": 0.3976, "d randn*3": 0.4203, "d wide+-80": 0.6226, "wrapper loss": 0.2715,
          "wrapper d": 0.2569}

KS = (1, 2, 63, 64, 255, 256, 257, 1000, 1001, 4095, 4096)
NS = (1, 3)
SMOOTH = (0.0, 0.1)
FAMILIES = ("randn*3", "equal", "offset+1000", "wide+-80", "masked")

_CALLED = set()
_WORST = {}


def _f32(v):
    """The value a C float argument carries, as a Python float."""
    return float(torch.tensor(v, dtype=F32).double())


# ------------------------------------------------------------------------------ cross-entropy reference --
def cases(K, N):
    """The row families of the issue (name, [N, K] fp32 logits before the cast to the stored dtype)."""
    g = torch.Generator().manual_seed(8 * K + N)
    yield "randn*3", torch.randn(N, K, generator=g) * 3
    yield "equal", torch.full((N, K), 0.75)
    yield "offset+1000", torch.randn(N, K, generator=g) * 3 + 1000
    yield "wide+-80", (torch.rand(N, K, generator=g) * 160 - 80)
    x = torch.randn(N, K, generator=g) * 3
    if K > 2:
        x[:, ::3] = float("-inf")
    yield "masked", x


def _labels(K, N, fam, ignore):
    """Class 0, class K-1 and a random class (N = 1: class K-1); never a masked class.  ``ignore``: -100 and K."""
    g = torch.Generator().manual_seed(31 * K + N)
    ok = [k for k in range(K) if not (fam == "masked" and K > 2 and k % 3 == 0)]
    rnd = ok[int(torch.randint(0, len(ok), (1,), generator=g))]
    lab = [ok[-1]] if N == 1 else [ok[0], ok[-1], rnd][:N]
    if ignore:
        lab[0] = -100
        if N > 2:
            lab[2] = K
    return torch.tensor(lab, dtype=torch.int64)


def _gout(N, fam):
    """Per-row upstream gradients: powers of two for the equal family (its d is exact), else arbitrary."""
    return torch.tensor(([2.0, -0.5, 0.25] if fam == "equal" else [1.25, -0.7, 0.3])[:N], dtype=F32)


def xent_ref(xq, labels, s, gout, mut=None):
    """Float64 reference and bounds for the stored logits ``xq`` [N, K]; ``mut`` names a mutant (CPU tests)."""
    x = xq.double()
    N, K = x.shape
    s = _f32(s)
    go = gout.double()
    live = (labels >= 0) & (labels < K)
    t = labels.clamp(0, K - 1)
    if mut == "target+1":
        t = (t + 1) % K
    if mut == "gout neighbour":
        go = go.roll(1)
    mx = x.max(1).values
    if mut == "class dropped":
        lse = torch.logsumexp(x[:, :-1], 1) if K > 1 else torch.full((N,), float("-inf"), dtype=F64)
    elif mut == "last doubled":
        lse = torch.logsumexp(torch.cat([x, x[:, -1:]], 1), 1)
    else:
        lse = torch.logsumexp(x, 1)
    xt = x.gather(1, t[:, None])[:, 0]
    mean = x.mean(1)
    loss = (1 - s) * (lse - xt)
    if s:
        loss = loss + s * (lse - mean)
    loss = torch.where(live, loss, torch.zeros_like(loss))
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    target = (1 - s) * onehot + s / ((K - 1) if (mut == "s/(K-1)" and K > 1) else K)
    if mut == "s/(K-1)" and K == 1:
        target = target + float("inf")
    d = (p - target) * go[:, None]
    if mut == "ignored p*gout":
        d = torch.where(live[:, None], d, p * go[:, None])
    else:
        d = torch.where(live[:, None], d, torch.zeros_like(d))
    # magnitudes and bounds (docstring)
    pos = p > 0
    xl = torch.where(pos, (x - lse[:, None]).abs(), torch.zeros_like(x))
    H = (p * xl).sum(1)
    e_lse = U * (27 + 3 * H + 4 * (lse - mx).abs() + 2 * lse.abs())
    A = (1 - s) * (lse - xt).abs()
    B = s * (lse - mean).abs() if s else torch.zeros_like(A)
    e_loss = e_lse + U * (4 * A + 4 * B + (26 * s * x.abs().mean(1) if s else 0.0))
    e_d = go.abs()[:, None] * (p * (1.01 * (e_lse[:, None] + 3 * U * xl) + 2 * U) + 3 * U * target.abs()
                               + 2 * U * (p - target).abs()) + 2.0 ** -125
    return dict(lse=lse, loss=loss, d=d, live=live, e_lse=e_lse, e_loss=e_loss, e_d=e_d, K=K, N=N, s=s)


@functools.lru_cache(maxsize=None)
def _xcase(K, N, dtype, s, fam, ignore):
    """Stored logits, labels, gout and the float64 reference of one case; computed once, shared read-only."""
    xq = dict(cases(K, N))[fam].to(dtype)
    labels, gout = _labels(K, N, fam, ignore), _gout(N, fam)
    return xq, labels, gout, xent_ref(xq, labels, s, gout)


def _ulp_bf16(ref):
    _, e = torch.frexp(ref)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 8))


def _outside(got, ref, bound):
    """(mask of elements outside |got - ref| <= bound, error / bound); an infinite ref demands equality."""
    got = got.double()
    inf = torch.isinf(ref)
    err = torch.where(inf, torch.zeros_like(ref), (got - torch.where(inf, torch.zeros_like(ref), ref)).abs())
    bad = torch.where(inf, got != ref, ~(err <= bound))
    return bad, torch.where(inf, torch.zeros_like(err), err / bound.clamp_min(1e-300))


def xent_failures(loss, lse, d, r, dtype):
    """Every assertion a (loss, lse, d) triple of one case is held to -> {name: (violations, largest ratio)}.
    The GPU tests demand that all counts are 0; the CPU tests that a mutant makes one of them positive."""
    out = {}
    live = r["live"]
    bad, ratio = _outside(lse, r["lse"], r["e_lse"])
    out["lse"] = (int(bad.sum()), float(ratio.max()))
    bad, ratio = _outside(loss, r["loss"], r["e_loss"])
    out["loss"] = (int(bad[live].sum()), float(ratio[live].max()) if live.any() else 0.0)
    free = 0.5 * _ulp_bf16(r["d"]) if dtype == BF16 else torch.zeros_like(r["d"])
    err = (d.double() - r["d"]).abs()
    bad = ~(err <= free + r["e_d"])
    ratio = (err - free).clamp_min(0) / r["e_d"]
    out["d"] = (int(bad[live].sum()), float(ratio[live].max()) if live.any() else 0.0)
    # exact by construction
    out["ignored loss == 0"] = (int((loss[~live] != 0).sum() + torch.isnan(loss[~live]).sum()), 0.0)
    out["ignored d == 0"] = (int((d[~live] != 0).sum() + torch.isnan(d[~live].float()).sum()), 0.0)
    out["finite"] = (int((~torch.isfinite(lse)).sum() + torch.isnan(loss).sum() + (~torch.isfinite(d.float())).sum()),
                     0.0)
    return out


def _pow2(K):
    return K & (K - 1) == 0


# ------------------------------------------------------------------------- cross-entropy: CPU (no GPU) --
def _stored(r, dtype):
    """The reference rounded as a perfect kernel would store it."""
    return r["loss"].float(), r["lse"].float(), r["d"].to(dtype)


@pytest.mark.parametrize("K", KS)
def test_cpu_bound_sits_between_floor_and_ceiling(K):
    """lse and loss bounds: never below the measured error of a plain fp32 evaluation (1.1 * 2^-24 max(1, |lse|)),
    and at K = 4096 with equal logits below half the shift of one dropped class; the reference passes itself."""
    ceiling = 0.5 * math.log(4096 / 4095)
    for N in NS:
        for dtype in (F32, BF16):
            for s in SMOOTH:
                for fam in FAMILIES:
                    xq, labels, gout, r = _xcase(K, N, dtype, s, fam, False)
                    floor = 1.1 * U * r["lse"].abs().clamp_min(1)
                    assert (r["e_lse"] >= floor).all() and (r["e_loss"] >= floor).all(), (fam, "floor")
                    if fam == "equal" and K == 4096:
                        assert float(r["e_lse"].max()) < ceiling and float(r["e_loss"].max()) < ceiling
                    # a plain fp32 evaluation of the kernel's formula stays inside the bound (the floor's origin)
                    x32 = xq.float()
                    m = x32.max(1, keepdim=True).values
                    lse32 = m[:, 0] + torch.log(torch.exp(x32 - m).sum(1))
                    assert not _outside(lse32, r["lse"], r["e_lse"])[0].any(), (fam, "fp32 lse")
                    fails = xent_failures(*_stored(r, dtype), r, dtype)
                    assert all(c == 0 for c, _ in fails.values()), (fam, fails)


@pytest.mark.parametrize("K", KS)
def test_cpu_xent_mutants_break_the_assertions(K):
    for N in NS:
        for s in SMOOTH:
            seen = {}
            for dtype in (F32, BF16):
                for fam in FAMILIES:
                    xq, labels, gout, r = _xcase(K, N, dtype, s, fam, False)
                    for mut in ("class dropped", "last doubled", "target+1", "s/(K-1)", "gout neighbour"):
                        m = xent_ref(xq, labels, s, gout, mut)
                        seen[(mut, dtype, fam)] = xent_failures(*_stored(m, dtype), r, dtype)
                    xq, labels, gout, ri = _xcase(K, N, dtype, s, fam, True)
                    m = xent_ref(xq, labels, s, gout, "ignored p*gout")
                    got = xent_failures(*_stored(m, dtype), ri, dtype)
                    # (bf16 stores a p below 2^-133 as 0: the row still holds a class with p >= 1 / K)
                    assert got["ignored d == 0"][0] > 0, (fam, dtype, "ignored row's gradient")
            for dtype in (F32, BF16):
                for mut in ("class dropped", "last doubled"):  # the smallest shift: equal logits
                    f = seen[(mut, dtype, "equal")]
                    assert f["lse"][0] == N, (mut, K, f)
                    assert f["loss"][0] == N or K == 1, (mut, K, f)
                if K >= 2:
                    for fam in FAMILIES:
                        assert seen[("target+1", dtype, fam)]["d"][0] > 0, ("target+1", fam, dtype)
                if N > 1 and K >= 2:  # (K = 1: d == 0 whatever gout)
                    for fam in FAMILIES:
                        assert seen[("gout neighbour", dtype, fam)]["d"][0] > 0, ("gout neighbour", fam, dtype)
            if s and K >= 2:
                assert all(seen[("s/(K-1)", F32, fam)]["d"][0] > 0 for fam in FAMILIES), "s/(K-1) fp32"
                if K <= 257:
                    assert seen[("s/(K-1)", BF16, "wide+-80")]["d"][0] > 0, "s/(K-1) bf16"


def test_cpu_wrapper_ignores_out_of_range_labels():
    """The CPU path of ops.cross_entropy follows the kernels: ignored rows give 0 / a zero gradient row, and
    the mean divides by N."""
    from tony_amd.ops.loss import cross_entropy

    K = 7
    x = torch.randn(4, K, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    labels = torch.tensor([5, -100, K, 2])
    for s in SMOOTH:
        per = cross_entropy(x, labels, s, "none")
        r = xent_ref(x.detach(), labels, s, torch.full((4,), 0.25))
        assert torch.equal(per[[1, 2]], torch.zeros(2)) and torch.allclose(per.double(), r["loss"], atol=1e-5)
        x.grad = None
        mean = cross_entropy(x, labels, s, "mean")
        assert abs(float(mean.detach()) - float(r["loss"].sum()) / 4) < 1e-5
        mean.backward()
        assert torch.equal(x.grad[[1, 2]], torch.zeros(2, K)) and torch.allclose(x.grad.double(), r["d"], atol=1e-6)


# ----------------------------------------------------------------------------------- dropout host model --
_U64 = np.uint64


def _mix64(z):
    with np.errstate(over="ignore"):
        z = z + _U64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> _U64(30))) * _U64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94d049bb133111eb)
        return z ^ (z >> _U64(31))


def _thr(p):
    return int(np.float32(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))


def _draws(seed, t, n, mut=None):
    """r [groups, 8]: the 16 bits of every element of every group of 8."""
    with np.errstate(over="ignore"):
        g = np.arange((n + 7) // 8, dtype=_U64)
        key = _mix64(_U64(seed) ^ _mix64(_U64(t) + _U64(0x632be59bd9b4e019)))
        step = _U64(1) if mut == "key+g" else _U64(2)
        h0, h1 = _mix64(key + step * g), _mix64(key + step * g + _U64(1))
    if mut == "swapped":
        h0, h1 = h1, h0
    r = np.empty((len(g), 8), dtype=np.uint32)
    for e in range(8):
        h = h0 if e < 4 else h1
        r[:, e] = ((h >> _U64(16 * (e & 3))) & _U64(0xffff)).astype(np.uint32)
    return r


def drop_model(seed, t, n, p, mut=None):
    """(keep [n] bool, scale as an fp32 number) of the counter-based mask; ``mut`` names a mutant."""
    thr = _thr(p)
    r = _draws(seed, t, n, mut)
    k = (r > thr) if mut == "r > thr" else (r >= thr)
    if mut == "tail shift" and n % 8:
        k[-1, :-1] = k[-1, 1:].copy()
    one = np.float32(1.0)
    with np.errstate(divide="ignore"):
        scale = one / np.float32(p) if mut == "scale 1/p" else one / (one - np.float32(p))
    return torch.from_numpy(k.reshape(-1)[:n].copy()), float(scale)


def _edge_p(seed, t, n):
    """The p whose threshold equals the 16 bits of the last live element: that element is kept by ``>=`` only."""
    return float(_draws(seed, t, n).reshape(-1)[n - 1]) / 65536.0


def drop_apply(x, keep, scale):
    """y as the kernel stores it: x * scale in fp32 rounded once to x's dtype where kept, +0 where dropped."""
    y = (x.float() * torch.tensor(scale, dtype=F32)).to(x.dtype)
    return torch.where(keep.view(x.shape), y, torch.zeros_like(y))


def _bits(t):
    """The bit patterns (a -0 is not a +0)."""
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pack(keep):
    n = keep.numel()
    k = torch.zeros((n + 7) // 8 * 8, dtype=torch.uint8)
    k[:n] = keep.to(torch.uint8)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32)
    return (k.view(-1, 8).int() * w).sum(1).to(torch.uint8)


def _live(mask_bytes, n):
    """The n live keep bits of packed mask bytes (bit e of byte g: element 8 g + e)."""
    b = mask_bytes.cpu().int()
    bits = ((b[:, None] >> torch.arange(8, dtype=torch.int32)) & 1).reshape(-1)
    return bits[:n].bool()


DROP_NS = (1, 7, 8, 9, 2047, 2048, 2049, 8 * 256 * 3 + 5)
DROP_PS = (0.0, 0.1, 0.2, 0.5, 0.9, 0.99999)
DROP_RNG = ((1234, 0), (1234, 1), (2 ** 62 - 1, 2 ** 40))


def _drop_cases(n):
    for seed, t in DROP_RNG:
        for p in DROP_PS + (_edge_p(seed, t, n),):
            yield seed, t, p


@functools.lru_cache(maxsize=None)
def _drop_x(n, dtype):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(dtype)
    return torch.where(x == 0, torch.ones_like(x), x)  # no zero input: y == 0 only where dropped


def test_cpu_dropout_model_thresholds():
    assert _thr(0.0) == 0 and _thr(0.99999) == 65535 and _thr(0.999995) == 65536 and _thr(0.5) == 32768
    k, scale = drop_model(1234, 0, 4099, 0.0)
    assert k.all() and scale == 1.0
    assert not drop_model(1234, 0, 4099, 0.999995)[0].any()
    for n in DROP_NS:
        k = drop_model(1234, 0, n, 0.5)[0]
        assert torch.equal(_live(_pack(k), n), k)


def test_cpu_dropout_model_statistics():
    """Keep rate within 5 sigma of 1 - thr / 65536; agreement between steps t / t + 1 and seeds s / s + 1 within
    5 sigma of q^2 + (1 - q)^2 (independent masks).  The GPU mask is compared with this model bit for bit."""
    n = 1 << 16
    for p in (0.1, 0.2, 0.5, 0.9):
        k0, k1, k2 = (drop_model(s, t, n, p)[0] for s, t in ((1234, 0), (1234, 1), (1235, 0)))
        q = 1 - _thr(p) / 65536
        assert abs(float(k0.float().mean()) - q) <= 5 * (q * (1 - q) / n) ** 0.5
        a = q * q + (1 - q) ** 2
        for other in (k1, k2):
            assert abs(float((k0 == other).float().mean()) - a) <= 5 * (a * (1 - a) / n) ** 0.5


@pytest.mark.parametrize("n", DROP_NS)
def test_cpu_dropout_mutants_break_equality(n):
    """Each mutant of the model differs from the model in the mask or in y for some (seed, t, p) run at this n."""
    for dtype in (F32, BF16):
        x = _drop_x(n, dtype)
        for mut in ("r > thr", "swapped", "key+g", "scale 1/p", "tail shift"):
            differs = False
            for seed, t, p in _drop_cases(n):
                k, sc = drop_model(seed, t, n, p)
                km, scm = drop_model(seed, t, n, p, mut)
                with np.errstate(all="ignore"):
                    ym = drop_apply(x, km, scm)
                differs |= not torch.equal(k, km) or not torch.equal(_bits(drop_apply(x, k, sc)), _bits(ym))
            if mut == "tail shift" and n % 8 == 0:
                assert not differs  # no tail group at this n
            elif mut == "key+g" and n <= 8:
                # one group: g = 0 draws the same pair either way; the mutant needs a second group to show
                assert not differs
            else:
                assert differs, (mut, n, dtype)


# -------------------------------------------------------------------------------------- GPU plumbing --
def _L():
    from tony_amd.ops import _lib

    return _lib


def _k(name, *args, rc=0):
    lib = _L()
    if rc == 0:
        _CALLED.add(name)
    got = getattr(lib.lib(), name)(*args)
    assert got == rc, f"{name} returned {got}, expected {rc}"


def _slab(rows, cols, c0, dtype, fill, dev):
    return Slab(rows, cols, c0, dtype, fill, dev, vector_rows=False)


def _src(t2d, c0, dev):
    s = _slab(t2d.shape[0], t2d.shape[1], c0, t2d.dtype, float("nan"), dev)
    s.view.copy_(t2d.to(dev))
    return s


def _run_xent(dev, xq, labels, s, gout, want_rc=0, K=None):
    """Forward + backward through the C entry points on poisoned operands (ld = K + 16, ldd = K + 16)."""
    N, Kx = xq.shape
    K = K or Kx
    st = _L().stream_ptr(dev)
    bf = int(xq.dtype == BF16)
    x = _src(xq, 8, dev)
    lab = labels.to(dev)
    go = _src(gout.view(1, -1), 8, dev)
    loss, lse = _slab(1, N, 8, F32, SENT, dev), _slab(1, N, 8, F32, SENT, dev)
    d = _slab(N, Kx, 8, xq.dtype, SENT, dev)
    _k("tony_xent_fwd", x.ptr(), bf, N, K, x.ld, lab.data_ptr(), s, loss.ptr(), lse.ptr(), st, rc=want_rc)
    if want_rc == 0:
        _k("tony_xent_bwd", x.ptr(), bf, N, K, x.ld, lab.data_ptr(), s, lse.ptr(), go.ptr(), d.ptr(), d.ld, st)
    torch.cuda.synchronize()
    for sl, what in ((loss, "loss"), (lse, "lse"), (d, "dlogits")):
        sl.assert_surroundings_intact(what)
    return loss.view[0].cpu(), lse.view[0].cpu(), d.view.cpu()


def _note(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_xent_kernels_against_float64(cuda, K, dtype):
    """Every N, smoothing, row family and label kind at this K and dtype: bounds, exact cases, guards."""
    problems = []
    for N in NS:
        for s in SMOOTH:
            for fam in FAMILIES:
                for ignore in (False, True):
                    xq, labels, gout, r = _xcase(K, N, dtype, s, fam, ignore)
                    what = f"K={K} N={N} s={s} {fam} ignore={ignore}"
                    loss, lse, d = _run_xent(cuda, xq, labels, s, gout)
                    fails = xent_failures(loss, lse, d, r, dtype)
                    for name in ("lse", "loss", "d"):
                        _note(f"{name} {fam}", fails[name][1])
                    print(what, {k: v for k, v in fails.items() if v[1]})
                    if any(c for c, _ in fails.values()):
                        problems.append(f"{what}: {fails}")
                    exact = []
                    if K == 1:
                        exact += [(loss, torch.zeros(N), "loss == 0"), (lse, xq[:, 0].float(), "lse == x"),
                                  (d, torch.zeros(N, 1, dtype=dtype), "d == 0")]
                    if fam == "equal" and _pow2(K) and s == 0.0 and not ignore:
                        onehot = F.one_hot(labels, K).double()
                        exact.append((d, ((1.0 / K - onehot) * gout.double()[:, None]).to(dtype),
                                      "d == (1/K - onehot) gout"))
                    for got, want, name in exact:
                        if not torch.equal(got, want):
                            bad = got != want
                            problems.append(f"{what} {name}: {int(bad.sum())} of {got.numel()} differ, largest "
                                            f"|got - want| {float((got.double() - want.double()).abs().max()):.3e}")
    assert not problems, "\n".join(problems)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_xent_refuses_k_above_the_register_limit(cuda, dtype):
    xq = torch.zeros(3, 4097).to(dtype)
    loss, lse, _ = _run_xent(cuda, xq, torch.tensor([0, 1, 2]), 0.0, torch.ones(3), want_rc=-1)
    assert_equal(loss, torch.full((3,), SENT), "loss untouched")
    assert_equal(lse, torch.full((3,), SENT), "lse untouched")


def _torch_ref(x, labels, s, reduction, w=None):
    xr = x.detach().double().requires_grad_(True)
    per = F.cross_entropy(xr, labels, reduction="none", label_smoothing=_f32(s))
    out = per if reduction == "none" else per.sum() if reduction == "sum" else per.mean()
    (out * w.double()).sum().backward() if w is not None else out.backward()
    return out.detach(), xr.grad


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_wrapper_reductions_against_torch(cuda, reduction, dtype):
    """ops.cross_entropy: the three reductions and their gradients (the 1/N of the mean, an expanded scalar
    gout) against torch's float64 cross-entropy of the stored logits; non-contiguous logits give the same."""
    from tony_amd.ops import cross_entropy

    _CALLED.add("ops.cross_entropy")
    N, K, s = 5, 1001, 0.1
    g = torch.Generator().manual_seed(77)
    xq = (torch.randn(N, K, generator=g) * 3).to(dtype)
    labels = torch.randint(0, K, (N,), generator=g)
    w = torch.tensor([1.0, -2.0, 0.5, 4.0, 0.25]) if reduction == "none" else None
    gout = w if w is not None else torch.full((N,), 1.0 / N if reduction == "mean" else 1.0)
    r = xent_ref(xq, labels, s, gout)
    want, dwant = _torch_ref(xq, labels, s, reduction, w)
    assert torch.allclose(dwant, r["d"], rtol=2e-7, atol=1e-15), "the two float64 references agree (gout is fp32)"
    outs = []
    for x in (xq.to(cuda), xq.t().contiguous().to(cuda).t()):
        x.requires_grad_(True)
        out = cross_entropy(x, labels.to(cuda), s, reduction)
        ((out * w.to(cuda)).sum() if w is not None else out).backward()
        outs.append((out.detach().cpu(), x.grad.cpu()))
    assert outs[1][1].shape == (N, K) and not xq.t().contiguous().t().is_contiguous()
    assert_equal(outs[1][0], outs[0][0], "non-contiguous logits: loss")
    assert_equal(outs[1][1], outs[0][1], "non-contiguous logits: gradient")
    out, grad = outs[0]
    assert out.dtype == F32
    # the reduction adds N - 1 fp32 additions of the rows (and one division): N U sum |loss|
    e = r["e_loss"] if reduction == "none" else r["e_loss"].sum() + N * U * r["loss"].abs().sum()
    if reduction == "mean":
        e = e / N
    bad, ratio = _outside(out, want, e + torch.zeros_like(want))
    _note("wrapper loss", float(ratio.max()))
    assert not bad.any(), f"{reduction}: loss off by {float(ratio.max()):.2f} x bound"
    free = 0.5 * _ulp_bf16(dwant) if dtype == BF16 else 0.0
    err = (grad.double() - dwant).abs()
    lim = free + r["e_d"] + 2 * U * dwant.abs()  # (1 / N itself is rounded to fp32)
    _note("wrapper d", float(((err - free).clamp_min(0) / (lim - free)).max()))
    assert (err <= lim).all(), f"{reduction}: gradient outside the bound"


@gpu
def test_wrapper_ignored_rows_and_mean_over_n(cuda):
    """Labels outside [0, K): the row's loss and gradient are 0 (torch's ignore_index per row), whatever the
    smoothing, and reduction='mean' still divides by N (torch divides by the rows that count)."""
    from tony_amd.ops import cross_entropy

    N, K = 4, 257
    g = torch.Generator().manual_seed(3)
    xq = torch.randn(N, K, generator=g) * 3
    labels = torch.tensor([5, -100, K, 256])
    for s in SMOOTH:
        x = xq.to(cuda).requires_grad_(True)
        per = cross_entropy(x, labels.to(cuda), s, "none")
        tl = labels.clone()
        tl[2] = -100
        want = F.cross_entropy(xq.double(), tl, reduction="none", label_smoothing=_f32(s), ignore_index=-100)
        assert_equal(per.detach().cpu()[[1, 2]], torch.zeros(2), "ignored rows' loss")
        r = xent_ref(xq, labels, s, torch.ones(N))
        assert not _outside(per.detach().cpu(), want, r["e_loss"])[0].any()
        mean = cross_entropy(x, labels.to(cuda), s, "mean")
        lim = float(r["e_loss"].sum()) / N + N * U * float(want.sum())
        assert abs(float(mean.detach()) - float(want.sum()) / N) <= lim, "the mean divides by N, not by 2"
        mean.backward()
        assert_equal(x.grad.cpu()[[1, 2]], torch.zeros(2, K), "ignored rows' gradient")
        assert (x.grad.cpu()[[0, 3]] != 0).any(1).all()


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_wrapper_accepts_no_rows(cuda, dtype):
    """N = 0: both launchers return before a <<<0, 256>>> launch; the sum is 0 and the gradient empty."""
    from tony_amd.ops import cross_entropy

    x = torch.empty(0, 10, device=cuda, dtype=dtype, requires_grad=True)
    out = cross_entropy(x, torch.empty(0, dtype=torch.int64, device=cuda), 0.1, "sum")
    assert float(out) == 0.0
    out.backward()
    assert x.grad.shape == (0, 10) and x.grad.dtype == dtype
    st = _L().stream_ptr(cuda)
    _k("tony_xent_fwd", 0, 0, 0, 10, 10, 0, 0.0, 0, 0, st)
    _k("tony_xent_bwd", 0, 0, 0, 10, 10, 0, 0.0, 0, 0, 0, 10, st)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- GPU: dropout --
def _run_dropout(dev, x, seed, t, p, want_rc=0, offset=0):
    """The bare forward on a poisoned x; returns (y, mask bytes, rng) on the CPU after checking the guards."""
    n, dtype = x.numel(), x.dtype
    st = _L().stream_ptr(dev)
    xs = _src(torch.cat([x, x[:1]]).view(1, -1), 8, dev)  # (one spare element: the misaligned slice stays inside)
    y = _slab(1, n, 8, dtype, SENT, dev)
    mask = _slab(1, (n + 7) // 8, 16, torch.uint8, 0xA5, dev)
    rng = torch.tensor([seed, t], dtype=torch.int64, device=dev)
    esz = 2 if dtype == BF16 else 4
    assert xs.ptr() % 16 == 0 and y.ptr() % 16 == 0
    _k("tony_dropout_fwd", xs.ptr() + offset * esz, y.ptr(), mask.ptr(), n, int(dtype == BF16), p, rng.data_ptr(), st,
       rc=want_rc)
    torch.cuda.synchronize()
    y.assert_surroundings_intact("y")
    mask.assert_surroundings_intact("mask")
    return y.view[0].cpu(), mask.view[0].cpu(), rng.cpu()


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", DROP_NS)
def test_dropout_forward_is_the_host_model(cuda, n, dtype):
    x = _drop_x(n, dtype)
    for seed, t, p in _drop_cases(n):
        keep, scale = drop_model(seed, t, n, p)
        y, mask, rng = _run_dropout(cuda, x, seed, t, p)
        what = f"n={n} seed={seed} t={t} p={p}"
        assert_equal(_live(mask, n), keep, f"{what} mask bits")
        assert_equal(_bits(y), _bits(drop_apply(x, keep, scale)), f"{what} y")
        assert rng.tolist() == [seed, t], f"{what}: the bare forward changed rng"
        if p == 0.0:
            assert_equal(_bits(y), _bits(x), f"{what} y == x")


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dropout_threshold_65536_drops_everything(cuda, dtype):
    """p = 0.999995: float32(p) * 65536 + 0.5 truncates to 65536, above every 16-bit draw."""
    n = 2049
    x = _drop_x(n, dtype)
    y, mask, _ = _run_dropout(cuda, x, 1234, 0, 0.999995)
    assert not _live(mask, n).any()
    assert_equal(_bits(y), _bits(torch.zeros_like(x)), "y == +0")


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dropout_refuses_a_misaligned_x(cuda, dtype):
    n = 2049
    x = _drop_x(n, dtype)
    y, mask, _ = _run_dropout(cuda, x, 1234, 0, 0.5, want_rc=-3, offset=1)
    assert_equal(y, torch.full_like(x, SENT), "y untouched")
    assert_equal(mask, torch.full_like(mask, 0xA5), "mask untouched")


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", DROP_NS)
def test_dropout_backward_reads_the_stored_mask(cuda, n, dtype):
    """dx from dy and STORED mask bytes that no forward produced (the unused high bits of the last byte set)."""
    g = torch.Generator().manual_seed(5 * n + 1)
    dy = _drop_x(n, dtype).flip(0)
    mb = torch.randint(0, 256, ((n + 7) // 8,), generator=g).to(torch.uint8)
    if n % 8:
        mb[-1] |= 0xFF & ~((1 << (n % 8)) - 1)
    st = _L().stream_ptr(cuda)
    for p in (0.1, 0.5, 0.99999):
        dys = _src(dy.view(1, -1), 8, cuda)
        mask =_slab(1, mb.numel(), 16, torch.uint8, 0xA5, cuda)
        mask.view.copy_(mb.view(1, -1).to(cuda))
        dx = _slab(1, n, 8, dtype, SENT, cuda)
        _k("tony_dropout_bwd", dys.ptr(), dx.ptr(), mask.ptr(), n, int(dtype == BF16), p, st)
        torch.cuda.synchronize()
        dx.assert_surroundings_intact("dx")
        mask.assert_surroundings_intact("mask")
        assert_equal(mask.view[0].cpu(), mb, "the backward left the mask alone")
        scale = drop_model(0, 0, 1, p)[1]
        assert_equal(_bits(dx.view[0].cpu()), _bits(drop_apply(dy, _live(mb, n), scale)), f"n={n} p={p} dx")


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dropout_wrapper_and_counter(cuda, dtype):
    """ops.dropout: y and dx are the model's, rng == [seed, t + 1] afterwards; tony_counter_bump alone."""
    from tony_amd.ops.dropout import dropout

    _CALLED.add("ops.dropout")
    n, p = 8 * 256 * 3 + 5, 0.2
    seed, t = 2 ** 62 - 1, 2 ** 40
    x = _drop_x(n, dtype)
    keep, scale = drop_model(seed, t, n, p)
    rng = torch.tensor([seed, t], dtype=torch.int64, device=cuda)
    xd = x.to(cuda).view(11, -1).requires_grad_(True)
    y = dropout(xd, p, rng)
    dy = _drop_x(n, dtype).flip(0)
    y.backward(dy.to(cuda).view(11, -1))
    assert rng.tolist() == [seed, t + 1]
    assert_equal(_bits(y.detach().cpu().view(-1)), _bits(drop_apply(x, keep, scale)), "wrapper y")
    assert_equal(_bits(xd.grad.cpu().view(-1)), _bits(drop_apply(dy, keep, scale)), "wrapper dx")
    _k("tony_counter_bump", rng.data_ptr(), _L().stream_ptr(cuda))
    assert rng.tolist() == [seed, t + 2]
    keep2 = drop_model(seed, t + 2, n, p)[0]
    y2 = dropout(x.to(cuda), p, rng)
    assert_equal(_bits(y2.cpu()), _bits(drop_apply(x, keep2, scale)), "the next step's mask")
    assert not torch.equal(keep2, keep)


@gpu
def test_zz_every_loss_and_dropout_entry_point_ran(cuda):
    """Every entry point of csrc/loss.hip and csrc/dropout.hip and both public wrappers ran in this session
    (the module run as a whole); prints the live error / bound figures per family."""
    for fam, worst in sorted(_WORST.items()):
        print(f"largest error / bound, {fam}: {worst:.4f}")
    names = {"tony_xent_fwd", "tony_xent_bwd", "tony_dropout_fwd", "tony_dropout_bwd", "tony_counter_bump",
             "ops.cross_entropy", "ops.dropout"}
    assert names <= set(_L()._SIGNATURES) | {"ops.cross_entropy", "ops.dropout"}
    missing = sorted(names - _CALLED)
    assert not missing, f"entry points no case of this module called: {missing}"
    assert all(w <= 1.0 for w in _WORST.values()), _WORST
