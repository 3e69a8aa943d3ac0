"""Exact and ulp-tight tests of the BatchNorm (csrc/bn_act.hip) and pooling (csrc/pool.hip) kernels.

Every ``tony_bn_*`` / ``tony_maxpool_*`` / ``tony_avgpool*`` entry point is called directly, on operands for
which a correct kernel has (almost) no freedom, and compared with a float64 CPU reference written from the
mathematical definition -- never from the kernels' folded coefficient tables.

Operands.  x, res, dy, z are small integers (|x| <= 4, |dy| <= 3) held in bf16 (fp32 for the ``_f32`` forms),
gamma and beta are bf16-representable, the backward entry points get an integer mean and a power-of-two invstd.
Then every per-channel sum (x, x^2, dy', dy' * xhat) is an exact fp32 number whatever the lane map, unroll,
shard, atomic order or grid, so a kernel that drops or doubles one row, or resolves one segment boundary
wrongly, cannot produce it.

What is held to ``torch.equal`` (a failure prints the count and first coordinates):
  * BN forward: the folded [sum | sumsq] of tony_bn_stats / _stats_f32 / tony_bn_fwd_train; the ReLU byte mask
    of tony_bn_apply_res_m (== packed bits of the stored y > 0); y == 0 exactly where the reference's
    pre-activation is <= 0 (the inputs keep every pre-activation 2^-10 * mag away from 0); each ``_segs`` form
    against the plain form; the x3 planes (hi == bf16(v), lo == bf16(v - hi), plane 2 == plane 0).
  * BN backward: the folded [dsum | dsumx] of every reduce form; dgamma / dbeta (fp32: the exact value; bf16:
    rounded once; accumulate: pre + value rounded once); dres == dy where the mask bit is set, 0 elsewhere;
    tony_bn_bwd_res against tony_bn_bwd_res_m; ``_segs`` against plain; one-pass against the reduce + apply pair.
  * Pools: max-pool value and argmax byte (distinct integers per plane: torch's argmax is the only answer), the
    max-pool backward forms on integer dy (acc: from an integer pre-fill), tony_bn_relu_maxpool against
    tony_bn_apply + tony_maxpool_fwd (compile-time window K = 3 and runtime windows K = 2, 5; P = 0, 1),
    tony_maxpool_bwd_bnred's sums and dX, tony_bn_bwd_pool_apply against tony_bn_bwd_apply on the stored dY.

What is held to half a bf16 ulp plus an fp32 slack (y of every apply form, dx / dz of every backward apply form,
the average pools):
    |got - ref64| <= 1/2 ulp_bf16(ref64) + 2^-18 * mag          (no ulp term for fp32 outputs)
mag is the float64 sum of the magnitudes of the terms of the result:
    y :  |x| |g is| + |mean| |g is| + |beta| (+ |res|)
    dx:  |g is| (|dy'| + |sum dy'| / M + (|x| + |mean|) is sum|dy' xhat| / M)
    avg: sum |tap| / K^2
Derivation: the kernels build <= 5 per-channel fp32 coefficients with <= 16 roundings in all (1/M, the products
g*is, mean*g*is, bm*is*mu ..., the fma of the row loop), each a relative 2^-24 of one of the terms above, so at
most 16 half-ulps of mag; rsqrtf is good to 2 ulp (4 half-ulps); var = sumsq/M - mean^2 cancels, which
amplifies the 2 roundings of mean and the 2 of sumsq/M by E[x^2]/var <= 4 (asserted per channel on the CPU
reference for M > 2; for M <= 2 the division is exact) and halves through the rsqrt: <= 16 half-ulps more.
That is 36 < 64 fp32 half-ulps = 2^-18.  The final bf16 store rounds the fp32 value once: half a bf16 ulp of it.
The x3 plane forms are compared as hi + lo with 2^-16 |ref| more (lo is itself rounded to bf16: 2^-9 of
|v - hi| <= 2^-9 |v|, i.e. 2^-18 |v|; 2^-16 leaves the same factor 4 as above).
save_mean / save_invstd / running_mean / running_var: 2^-20 relative to their own term magnitudes.

Sensitivity.  test_cpu_* (no GPU) mutate the float64 reference the way a wrong kernel would -- one row dropped,
one row doubled, one segment boundary 8 columns off -- and assert that each mutant breaks the very assertion
the GPU result is held to, at every shape used: exact sums differ, y and dx exceed the bound in more than one
element.

Poison.  Every operand is a channel slice (ld > C) of a NaN-filled allocation, every destination a slice of a
sentinel-filled one (exact_helpers.Slab); after each case no byte outside a destination has changed (masks,
argmax bytes and the gaps between x3 planes included) and no NaN has reached an output.

Largest observed excess / (2^-18 * mag) per family on an MI355X (a record, not a tuning knob; RECORD below,
test_zz_every_entry_point_ran prints the live figures): bn forward y 0.0099, bn backward dx 0.0081, bn residual
y 0.0000 / dx 0.0002, bn fp32 y 0.0410 / dx 0.0299, bn fp32 planes y 0.0066 / dx 0.0009, bn + pool y 0.0000 /
dz 0.0000, avg pool 0.0156, avg pool planes 0.0000, public wrappers 0.0125.  Every exact comparison held.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from exact_helpers import SENT, Slab, assert_equal, pix_rows, poisoned

gpu = pytest.mark.gpu

# measured on an MI355X by this module (family -> largest excess / (2^-18 * mag)); bounds stay derived
RECORD = {"bn forward y": 0.0099, "bn backward dx": 0.0081, "bn residual y": 0.0000, "bn residual dx": 0.0002,
          "bn fp32 y": 0.0410, "bn fp32 dx": 0.0299, "bn fp32 y planes": 0.0066, "bn fp32 dx planes": 0.0009,
          "bn + pool y": 0.0000, "bn + pool dz": 0.0000, "avg pool": 0.0156, "avg pool planes": 0.0000,
          "wrappers": 0.0125}

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SLACK = 2.0 ** -18
EPS = 1e-3
MOM = 0.1

# M x C of the plain forward / backward: see the issue's table (RPI = 256 // (C / 8))
PLAIN = [(1, 8), (2, 8), (255, 8), (257, 8), (4100, 8), (286, 40), (1023, 40), (2051, 48), (1023, 80), (105, 192),
         (37, 264), (37, 2048),
         # C = 40: RPI = 51, the 4x unrolled loop takes rows r .. r + 3 * 51: both sides of 4 * RPI * k, k = 1, 2
         (203, 40), (204, 40), (205, 40), (407, 40), (408, 40), (409, 40)]
# the other forms: a partial last workgroup, more than one workgroup, a C / 8 that does not divide 256
OTHER = [(286, 40), (2051, 48), (105, 192)]

_CALLED = set()
_WORST = {}


def _sid(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------- float64 references --
def _eps64():
    return float(torch.tensor(EPS, dtype=F32).double())  # the kernels get eps as a C float


def _fwd_ref(x, g, b, relu, res=None, w=None):
    """BatchNorm (+ residual) (+ ReLU) of the rows x [M, C] in float64.  ``w`` (mutants only): per-row weights of
    the statistics, as a kernel that dropped (0) or doubled (2) a row would accumulate them."""
    M = x.shape[0]
    if w is None:
        s, q = x.sum(0), (x * x).sum(0)
        mean = s / M
        var = ((x - mean) ** 2).sum(0) / M
    else:
        s, q = (w[:, None] * x).sum(0), (w[:, None] * x * x).sum(0)
        mean = s / M
        var = (q / M - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + _eps64())
    k = g * invstd
    pre = (x - mean) * k + b
    mag = x.abs() * k.abs() + mean.abs() * k.abs() + b.abs()
    if res is not None:
        pre = pre + res
        mag = mag + res.abs()
    return dict(sum=s, sumsq=q, mean=mean, var=var, invstd=invstd, pre=pre, mag=mag,
                y=pre.clamp_min(0) if relu else pre, ex2=q / M, absx=x.abs().sum(0) / M)


def _bwd_ref(x, dy, g, b, mu, is_, relu, keep=None, w=None):
    """BatchNorm backward with the caller's mean / invstd in float64.  ``keep``: the ReLU mask of the residual
    forms (y > 0); else recomputed from the pre-activation when ``relu``."""
    M = x.shape[0]
    xhat = (x - mu) * is_
    if keep is None:
        keep = ((xhat * g + b) > 0) if relu else torch.ones_like(x, dtype=torch.bool)
    d = dy * keep
    ww = 1.0 if w is None else w[:, None]
    ds, dsx = (ww * d).sum(0), (ww * d * xhat).sum(0)
    k = g * is_
    dx = k * (d - ds / M - xhat * dsx / M)
    mag = k.abs() * (d.abs() + ds.abs() / M + (x.abs() + mu.abs()) * is_ * (d * xhat).abs().sum(0) / M)
    return dict(d=d, ds=ds, dsx=dsx, dx=dx, mag=mag)


def _ulp_bf16(ref):
    """The bf16 ulp at ``ref`` (float64): 2^(floor(log2 |ref|) - 7); 0 at 0."""
    _, e = torch.frexp(ref)  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 8))


def _violations(got, ref, mag, bf16, extra=None):
    """Elements of ``got`` outside |got - ref| <= 1/2 ulp_bf16(ref) + 2^-18 mag (+ extra): the one bound of this
    module (derivation in the module docstring).  Returns (mask of violations, excess / (2^-18 mag))."""
    got = got.double()
    free = (0.5 * _ulp_bf16(ref)) if bf16 else torch.zeros_like(ref)
    if extra is not None:
        free = free + extra
    err = (got - ref).abs()
    bad = ~(err <= free + SLACK * mag)  # (a NaN is a violation)
    return bad, (err - free).clamp_min(0) / (SLACK * mag).clamp_min(1e-300)


def _within(got, ref, mag, bf16, what, family, extra=None):
    got = got.detach().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(got.double()).all(), f"{what}: a NaN or Inf reached the output"
    bad, ratio = _violations(got, ref, mag, bf16, extra)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _WORST[family] = max(_WORST.get(family, 0.0), worst)
    print(f"{what}: largest excess / (2^-18 mag) = {worst:.4f}")
    if bad.any():
        first = [tuple(i) for i in bad.nonzero()[:8].tolist()]
        detail = ", ".join(f"{i}: got {got[i].item()} want {ref[i].item()}" for i in first)
        pytest.fail(f"{what}: {int(bad.sum())} of {got.numel()} elements outside 1/2 ulp + 2^-18 mag "
                    f"(largest excess {worst:.2f} x 2^-18 mag); first {detail}")


def _rel20(got, ref, mag, what):
    """The saved / running statistics: 2^-20 relative to the magnitude of their terms."""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: NaN"
    bad = ~((got - ref).abs() <= 2.0 ** -20 * mag)
    assert not bad.any(), (f"{what}: {int(bad.sum())} channels off by more than 2^-20; worst "
                           f"{float(((got - ref).abs() / mag.clamp_min(1e-300)).max()) * 2 ** 20:.2f} x 2^-20")


def _is_bf16(t):
    return torch.equal(t.to(BF16).double(), t)


@functools.lru_cache(maxsize=None)
def _case(M, C, res=False, relu=True):
    """The integer operands of one (M, C) BatchNorm case with their float64 forward and backward references.
    Computed once per shape and shared (read-only) by every test that uses it."""
    gen = torch.Generator().manual_seed(1000003 * M + C)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).double()  # noqa: E731
    off = ri(-1, 1, (C,))
    x = ri(-3, 3, (M, C)) + off  # |x| <= 4, per-channel offsets
    dy = ri(-3, 3, (M, C))
    r = ri(-2, 2, (M, C)) if res else None
    g = ri(4, 12, (C,)) / 8
    g[::5] = -g[::5]  # a negative gamma flips the ReLU side of x
    b = ri(-8, 8, (C,)) / 16
    if M > 2:
        # precondition of the bound: E[x^2] / var <= 4.  A channel that misses it (small M) gets +-4 alternating
        f = _fwd_ref(x, g, b, relu, r)
        badc = f["ex2"] > 4 * f["var"]
        alt = torch.tensor([4.0, -4.0], dtype=F64).repeat(M // 2 + 1)[:M]
        if M % 2:
            alt[-1] = 0
        x[:, badc] = alt[:, None]
    # ReLU margin: every |pre-activation| > 2^-10 mag, by nudging beta of an offending channel one bf16 step
    # (1/256: beta stays k / 256, |beta| < 1, which bf16 holds exactly)
    for _ in range(300):
        f = _fwd_ref(x, g, b, relu, r)
        offend = (f["pre"].abs() <= 2.0 ** -10 * f["mag"]).any(0)
        if not relu or not offend.any():
            break
        b[offend] += 1.0 / 256
    f = _fwd_ref(x, g, b, relu, r)
    assert not relu or (f["pre"].abs() > 2.0 ** -10 * f["mag"]).all(), "ReLU margin"
    assert M <= 2 or (f["ex2"] <= 4 * f["var"]).all(), "E[x^2] / var <= 4"
    assert _is_bf16(g) and _is_bf16(b) and b.abs().max() < 1 and x.abs().max() <= 4 and dy.abs().max() <= 3
    mu = off.clone()  # the backward's caller-given statistics: an integer mean, a power-of-two invstd
    is_ = torch.tensor([0.5, 0.25]).double().repeat(C // 2 + 1)[:C].clone()
    keep = (f["y"].to(BF16) > 0) if res else None  # the residual forms mask by the STORED y
    bw = _bwd_ref(x, dy, g, b, mu, is_, relu, keep)
    for t in (bw["ds"], bw["dsx"], f["sum"], f["sumsq"]):
        assert torch.equal(t.float().double(), t) and t.abs().max() < 2 ** 22  # exact in fp32 with room to add
    return dict(M=M, C=C, x=x, dy=dy, res=r, g=g, b=b, relu=relu, f=f, mu=mu, is_=is_, bw=bw)


def _round_once(v, dtype):
    return v.to(dtype)  # float64 -> fp32 / bf16, round to nearest even, once


# ----------------------------------------------------------------------------- CPU sensitivity checks --
# every (M, C) a GPU case of this module uses: the plain table, the residual forms (OTHER), the _segs forms
# (C = 88), the pool-fused forms (M = N H W of FUSED) and the public wrappers
_EXTRA_MC = [(286, 88), (2051, 88), (126, 8), (126, 40), (510, 8), (510, 40)]
_CPU_CASES = [(s, False) for s in PLAIN + _EXTRA_MC] + [(s, True) for s in OTHER]


def _row_mutants(M):
    w0, w2 = torch.ones(M, dtype=F64), torch.ones(M, dtype=F64)
    w0[M // 2] = 0  # a dropped row
    w2[M - 1] = 2  # a doubled (last) row
    return {"dropped row": w0, "doubled row": w2}


@pytest.mark.parametrize("shape,res", _CPU_CASES, ids=[f"{_sid(s)}-{'res' if r else 'plain'}" for s, r in _CPU_CASES])
def test_cpu_forward_mutants_break_the_assertions(shape, res):
    """One row dropped from / doubled in the statistics: the exact sums differ and y (rounded to bf16 as the
    kernel stores it) leaves the half-ulp + 2^-18 bound in more than one element, at every shape used."""
    M, C = shape
    c = _case(M, C, res, True)
    f = c["f"]
    ok, _ = _violations(f["y"].to(BF16), f["y"], f["mag"], True)
    assert not ok.any(), "the reference itself must pass"
    if M == 1:
        return  # one row: dropping it leaves nothing to normalise, doubling it is the only mutant
    for name, w in _row_mutants(M).items():
        m = _fwd_ref(c["x"], c["g"], c["b"], True, c["res"], w)
        assert not torch.equal(m["sum"], f["sum"]) or not torch.equal(m["sumsq"], f["sumsq"]), name
        assert not torch.equal(torch.cat([m["sum"], m["sumsq"]]), torch.cat([f["sum"], f["sumsq"]])), name
        bad, _ = _violations(m["y"].to(BF16), f["y"], f["mag"], True)
        assert int(bad.sum()) > 1, f"{name} at {M}x{C}: only {int(bad.sum())} elements of y leave the bound"
        bad32, _ = _violations(m["y"].float(), f["y"], f["mag"], False)
        assert int(bad32.sum()) > 1, f"{name} at {M}x{C}: fp32 y stays inside the bound"


@pytest.mark.parametrize("shape,res", _CPU_CASES, ids=[f"{_sid(s)}-{'res' if r else 'plain'}" for s, r in _CPU_CASES])
def test_cpu_backward_mutants_break_the_assertions(shape, res):
    M, C = shape
    c = _case(M, C, res, True)
    bw = c["bw"]
    keep = (c["f"]["y"].to(BF16) > 0) if res else None
    ok, _ = _violations(bw["dx"].to(BF16), bw["dx"], bw["mag"], True)
    assert not ok.any(), "the reference itself must pass"
    if M == 1:
        return
    hit = 0
    for name, w in _row_mutants(M).items():
        m = _bwd_ref(c["x"], c["dy"], c["g"], c["b"], c["mu"], c["is_"], True, keep, w)
        if torch.equal(m["ds"], bw["ds"]) and torch.equal(m["dsx"], bw["dsx"]):
            continue  # (a row whose dy' is all zero: possible only at C = 8 with M tiny)
        hit += 1
        bad, _ = _violations(m["dx"].to(BF16), bw["dx"], bw["mag"], True)
        assert int(bad.sum()) > 1, f"{name} at {M}x{C}: only {int(bad.sum())} elements of dx leave the bound"
        bad32, _ = _violations(m["dx"].float(), bw["dx"], bw["mag"], False)
        assert int(bad32.sum()) > 1, f"{name} at {M}x{C}: fp32 dx stays inside the bound"
    assert hit >= 1, "no row mutant changed the sums"


SEG_SPLITS = {1: (88,), 2: (24, 88), 3: (24, 32, 88), 4: (24, 32, 72, 88)}  # 24 | 8 | 40 | 16


def test_cpu_segment_boundary_mutant_breaks_equality():
    """A segment boundary resolved 8 columns off: the lane at the boundary reads / writes another tensor's
    columns.  The ``_segs`` forms are held to equality with the plain form, which such a shift breaks."""
    c = _case(286, 88, False, True)
    e0 = SEG_SPLITS[4][0]
    y = c["f"]["y"].to(BF16)
    wrong = y.clone()
    wrong[:, e0:e0 + 8] = y[:, e0 + 8:e0 + 16]  # the lane of columns [e0, e0 + 8) addressed as if in segment 0
    assert not torch.equal(wrong, y)
    dy = c["dy"].clone()
    dy[:, e0:e0 + 8] = c["dy"][:, e0 + 8:e0 + 16]
    m = _bwd_ref(c["x"], dy, c["g"], c["b"], c["mu"], c["is_"], True)
    assert not torch.equal(m["ds"], c["bw"]["ds"]) and not torch.equal(m["dsx"], c["bw"]["dsx"])
    bad, _ = _violations(m["dx"].to(BF16), c["bw"]["dx"], c["bw"]["mag"], True)
    assert int(bad.sum()) > 1


def test_cpu_pool_mutants_break_the_assertions():
    """A pool that drops one window row / column, or an average that counts one tap twice."""
    x = _pool_planes(2, 8, 9, 7)
    y, idx = F.max_pool2d(x, 3, 2, 0, return_indices=True)
    y2 = F.max_pool2d(x[:, :, :, :-1], (3, 2), 2, 0)  # the last window column never read
    assert not torch.equal(y[..., :y2.shape[-1]], y2)
    a = _ints((2, 16, 9, 7), 4, 3)
    ref, mag = F.avg_pool2d(a, 3, 1, 1), F.avg_pool2d(a.abs(), 3, 1, 1)
    twice = ref + a / 9
    bad, _ = _violations(twice.to(BF16), ref, mag, True)
    assert int(bad.sum()) > 1


# ------------------------------------------------------------------------------------ GPU plumbing --
def _L():
    from tony_amd.ops import _lib

    return _lib


def _k(name, *args, rc=0):
    """Call entry point ``name`` directly, record that it ran, and check its return code."""
    lib = _L()
    if rc == 0:  # (a call that must be refused launches nothing: it does not count as coverage)
        _CALLED.add(name)
    got = getattr(lib.lib(), name)(*args)
    assert got == rc, f"{name} returned {got}, expected {rc}"


class _Run:
    """The device buffers of one case: operands in NaN-poisoned slabs, destinations in sentinel slabs whose
    surroundings ``done()`` checks."""

    def __init__(self, dev):
        self.dev, self.dsts = dev, []
        self.stream = _L().stream_ptr(dev)
        self._c0 = 0

    def _next_c0(self):
        self._c0 = self._c0 % 24 + 8  # 8, 16, 24: every tensor of a case has its own row stride
        return self._c0

    def src(self, t, dtype):
        """[rows, cols] float64 -> a channel slice (ld > cols) of a NaN allocation."""
        return poisoned(t.to(dtype).to(self.dev), self._next_c0())

    def dst(self, rows, cols, dtype, what, c0=None, fill=SENT):
        s = Slab(rows, cols, self._next_c0() if c0 is None else c0, dtype, fill, self.dev,
                 vector_rows=dtype != torch.uint8)
        self.dsts.append((s, what))
        return s

    def vec(self, t, dtype):
        """A per-channel operand: C values inside a NaN allocation."""
        s = Slab(1, t.numel(), 8, dtype, float("nan"), self.dev, vector_rows=False)
        s.view.copy_(t.to(dtype).to(self.dev).view(1, -1))
        return s

    def vdst(self, n, dtype, what, init=None):
        s = Slab(1, n, 8, dtype, SENT, self.dev, vector_rows=False)
        if init is not None:
            s.view.copy_(init.to(dtype).to(self.dev).view(1, -1))
        self.dsts.append((s, what))
        return s

    def stats(self, C, what, extra=0):
        """A zeroed sharded statistics workspace (+ ``extra`` words) between sentinel guards."""
        s = Slab(1, _L().stat_floats(C) + extra, 0, F32, SENT, self.dev, guard_ld=2 * C, vector_rows=False)
        s.view.zero_()
        self.dsts.append((s, what))
        return s

    def folded(self, ws, C):
        return _L().fold_stats(ws.view.reshape(-1), C).cpu()

    def done(self):
        torch.cuda.synchronize()
        for s, what in self.dsts:
            s.assert_surroundings_intact(what)


def _params(run, c, pb):
    dt = BF16 if pb else F32
    return run.vec(c["g"], dt), run.vec(c["b"], dt), dt


def _check_fwd_stats(run, c, sm, si, rm, rv, rm0, rv0, what):
    f, M = c["f"], c["M"]
    _rel20(sm.view[0], f["mean"], f["absx"], f"{what} save_mean")
    _rel20(si.view[0], f["invstd"], f["invstd"], f"{what} save_invstd")
    unb = f["var"] * (M / (M - 1) if M > 1 else 1.0)
    _rel20(rm.view[0], (1 - MOM) * rm0 + MOM * f["mean"], (1 - MOM) * rm0.abs() + MOM * f["absx"],
           f"{what} running_mean")
    # var = E[x^2] - mean^2: its terms' magnitude is E[x^2] + mean^2
    _rel20(rv.view[0], (1 - MOM) * rv0 + MOM * unb,
           (1 - MOM) * rv0.abs() + MOM * (f["ex2"] + f["mean"] ** 2) * (M / (M - 1) if M > 1 else 1.0),
           f"{what} running_var")


def _check_y(c, y, bf16, what, family):
    f = c["f"]
    _within(y, f["y"], f["mag"], bf16, what, family)
    if c["relu"]:
        assert_equal(y.cpu() == 0, f["pre"] <= 0, f"{what}: y == 0 exactly where the pre-activation is <= 0")


def _running(run, C):
    gen = torch.Generator().manual_seed(C)
    rm0 = torch.randint(-4, 5, (C,), generator=gen).double() / 4
    rv0 = torch.randint(1, 9, (C,), generator=gen).double() / 4
    return rm0, rv0, run.vdst(C, F32, "running_mean", rm0), run.vdst(C, F32, "running_var", rv0)


def _exact_sums(got, a, b, what):
    assert_equal(got, torch.cat([a, b]).float(), what)


# --------------------------------------------------------------------------- BatchNorm forward, plain --
@gpu
@pytest.mark.parametrize("shape", PLAIN, ids=_sid)
def test_bn_forward_plain(cuda, shape):
    """tony_bn_stats + tony_bn_apply (even cases) / tony_bn_fwd_train (odd cases), bf16 rows; fp32 and bf16
    parameters and ReLU on / off alternate over the shapes."""
    M, C = shape
    i = PLAIN.index(shape)
    relu, pb, one_call = i % 3 != 2, i % 2, (i // 2) % 2
    c = _case(M, C, False, relu)
    run = _Run(cuda)
    x = run.src(c["x"], BF16)
    y = run.dst(M, C, BF16, "y")
    g, b, _ = _params(run, c, pb)
    ws = run.stats(C, "statistics")
    sm, si = run.vdst(C, F32, "save_mean"), run.vdst(C, F32, "save_invstd")
    rm0, rv0, rm, rv = _running(run, C)
    if one_call:
        _k("tony_bn_fwd_train", x.ptr(), M, C, x.ld, y.ptr(), y.ld, g.ptr(), b.ptr(), pb, EPS, int(relu), ws.ptr(),
           sm.ptr(), si.ptr(), rm.ptr(), rv.ptr(), MOM, run.stream)
    else:
        _k("tony_bn_stats", x.ptr(), M, C, x.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
        _k("tony_bn_apply", x.ptr(), M, C, x.ld, y.ptr(), y.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, g.ptr(), b.ptr(),
           pb, EPS, int(relu), 0, sm.ptr(), si.ptr(), rm.ptr(), rv.ptr(), MOM, run.stream)
    run.done()
    what = f"bn forward {M}x{C}"
    _exact_sums(run.folded(ws, C), c["f"]["sum"], c["f"]["sumsq"], f"{what} folded [sum | sumsq] (channel)")
    _check_y(c, y.view, True, f"{what} y (row, channel)", "bn forward y")
    _check_fwd_stats(run, c, sm, si, rm, rv, rm0, rv0, what)


@gpu
def test_bn_forward_infer(cuda):
    """mode 1 (tony_bn_fwd_infer): y from the running statistics, which stay untouched."""
    M, C = 286, 40
    c = _case(M, C, False, True)
    run = _Run(cuda)
    x, y = run.src(c["x"], BF16), run.dst(M, C, BF16, "y")
    g, b, _ = _params(run, c, 1)
    rm0 = c["mu"]
    rv0 = 1.0 / c["is_"] ** 2 - _eps64()  # invstd = a power of two up to fp32 rounding of rv0
    rv0 = rv0.float().double()
    rm, rv = run.vdst(C, F32, "running_mean", rm0), run.vdst(C, F32, "running_var", rv0)
    _k("tony_bn_fwd_infer", x.ptr(), M, C, x.ld, y.ptr(), y.ld, g.ptr(), b.ptr(), 1, EPS, 0, rm.ptr(), rv.ptr(),
       run.stream)
    run.done()
    k = c["g"] / torch.sqrt(rv0 + _eps64())
    ref = (c["x"] - rm0) * k + c["b"]
    mag = (c["x"].abs() + rm0.abs()) * k.abs() + c["b"].abs()
    _within(y.view, ref, mag, True, "bn infer y (row, channel)", "bn forward y")
    assert_equal(rm.view[0].cpu(), rm0.float(), "running_mean untouched")
    assert_equal(rv.view[0].cpu(), rv0.float(), "running_var untouched")


# -------------------------------------------------------------------------- BatchNorm backward, plain --
def _check_param_grads(c, dg, db, pb, pre_g, pre_b, what):
    dt = BF16 if pb else F32
    bw = c["bw"]
    want_g = bw["dsx"] if pre_g is None else pre_g + bw["dsx"]
    want_b = bw["ds"] if pre_b is None else pre_b + bw["ds"]
    assert_equal(dg.view[0].cpu(), _round_once(want_g, dt), f"{what} dgamma (channel)")
    assert_equal(db.view[0].cpu(), _round_once(want_b, dt), f"{what} dbeta (channel)")


@gpu
@pytest.mark.parametrize("shape", PLAIN, ids=_sid)
def test_bn_backward_plain(cuda, shape, monkeypatch):
    """tony_bn_bwd_reduce + tony_bn_bwd_apply, then the one-call tony_bn_bwd and the one-launch
    tony_bn_bwd_onepass through _lib.bn_bwd: sums, dgamma, dbeta exact; dx inside the bound and bit-identical
    across the three forms."""
    M, C = shape
    i = PLAIN.index(shape)
    relu, pb, acc = i % 3 != 2, i % 2, (i // 2) % 2
    c = _case(M, C, False, relu)
    bw = c["bw"]
    lib = _L()
    run = _Run(cuda)
    x, dy = run.src(c["x"], BF16), run.src(c["dy"], BF16)
    g, b, dt = _params(run, c, pb)
    mu, is_ = run.vec(c["mu"], F32), run.vec(c["is_"], F32)
    gen = torch.Generator().manual_seed(7 * M + C)
    pre_g = torch.randint(-8, 9, (C,), generator=gen).double() if acc else None
    pre_b = torch.randint(-8, 9, (C,), generator=gen).double() if acc else None
    what = f"bn backward {M}x{C}"
    outs = []
    for form in ("pair", "one-call", "one-pass"):
        dx = run.dst(M, C, BF16, f"dx {form}")
        dg, db = run.vdst(C, dt, "dgamma", pre_g), run.vdst(C, dt, "dbeta", pre_b)
        ws = run.stats(C, f"workspace {form}", extra=4)
        if form == "pair":
            _k("tony_bn_bwd_reduce", x.ptr(), x.ld, dy.ptr(), dy.ld, M, C, mu.ptr(), is_.ptr(), g.ptr(), b.ptr(), pb,
               int(relu), ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
            _k("tony_bn_bwd_apply", x.ptr(), x.ld, dy.ptr(), dy.ld, dx.ptr(), dx.ld, M, C, mu.ptr(), is_.ptr(),
               g.ptr(), b.ptr(), pb, int(relu), ws.ptr(), ws.ptr() + 4 * C, 2 * C, dg.ptr(), db.ptr(), acc,
               run.stream)
        else:
            monkeypatch.setattr(lib, "BN_ONEPASS", form == "one-pass")
            monkeypatch.setattr(lib, "BN_ONEPASS_MAX_BYTES", 0)
            lib.bn_bwd(x.view, x.ld, dy.view, dy.ld, dx.view, dx.ld, M, C, mu.view, is_.view, g.view, b.view, pb, relu,
                       ws.view.reshape(-1), dg.view, db.view, bool(acc), cuda)
            _CALLED.add("tony_bn_bwd_onepass" if form == "one-pass" else "tony_bn_bwd")
        run.done()
        _exact_sums(run.folded(ws, C), bw["ds"], bw["dsx"], f"{what} {form} folded [dsum | dsumx] (channel)")
        _check_param_grads(c, dg, db, pb, pre_g, pre_b, f"{what} {form}")
        _within(dx.view, bw["dx"], bw["mag"], True, f"{what} {form} dx (row, channel)", "bn backward dx")
        outs.append(dx.view.cpu())
    assert_equal(outs[1], outs[0], f"{what}: one-call dx against the reduce + apply pair")
    assert_equal(outs[2], outs[0], f"{what}: one-pass dx against the reduce + apply pair")


# ------------------------------------------------------------------------- residual and mask forms --
@gpu
@pytest.mark.parametrize("shape", OTHER, ids=_sid)
def test_bn_residual_and_mask_forms(cuda, shape):
    M, C = shape
    pb = OTHER.index(shape) % 2
    c = _case(M, C, True, True)
    f, bw = c["f"], c["bw"]
    run = _Run(cuda)
    x, r, dy = run.src(c["x"], BF16), run.src(c["res"], BF16), run.src(c["dy"], BF16)
    g, b, dt = _params(run, c, pb)
    ws = run.stats(C, "statistics")
    _k("tony_bn_stats", x.ptr(), M, C, x.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
    ys = []
    mask = run.dst(M, C // 8, torch.uint8, "mask", fill=0xAB)
    for form in ("res", "res_m"):
        y = run.dst(M, C, BF16, f"y {form}")
        sm, si = run.vdst(C, F32, "save_mean"), run.vdst(C, F32, "save_invstd")
        rm0, rv0, rm, rv = _running(run, C)
        args = (x.ptr(), M, C, x.ld, r.ptr(), r.ld, y.ptr(), y.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, g.ptr(), b.ptr(),
                pb, EPS, 1, 0, sm.ptr(), si.ptr(), rm.ptr(), rv.ptr(), MOM)
        if form == "res":
            _k("tony_bn_apply_res", *args, run.stream)
        else:
            _k("tony_bn_apply_res_m", *args, mask.ptr(), mask.ld, run.stream)
        run.done()
        what = f"bn {form} forward {M}x{C}"
        _check_y(c, y.view, True, f"{what} y (row, channel)", "bn residual y")
        _check_fwd_stats(run, c, sm, si, rm, rv, rm0, rv0, what)
        ys.append(y)
    assert_equal(ys[1].view.cpu(), ys[0].view.cpu(), "apply_res_m y against apply_res y")
    keep = ys[0].view.cpu() > 0  # == the reference's, by _check_y
    bits = (keep.view(M, C // 8, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)
    assert_equal(mask.view.cpu(), bits, "ReLU byte mask == packed bits of the stored y > 0 (row, byte)")
    # backward: by the stored y, and by the byte mask
    mu, is_ = run.vec(c["mu"], F32), run.vec(c["is_"], F32)
    outs = []
    for form in ("res", "res_m"):
        dx, dres = run.dst(M, C, BF16, f"dx {form}"), run.dst(M, C, BF16, f"dres {form}")
        dg, db = run.vdst(C, dt, "dgamma"), run.vdst(C, dt, "dbeta")
        wsb = run.stats(C, f"workspace {form}")
        m = (ys[0].ptr(), ys[0].ld) if form == "res" else (mask.ptr(), mask.ld)
        _k("tony_bn_bwd_" + form, x.ptr(), x.ld, dy.ptr(), dy.ld, *m, dx.ptr(), dx.ld, dres.ptr(), dres.ld, M, C,
           mu.ptr(), is_.ptr(), g.ptr(), b.ptr(), pb, wsb.ptr(), dg.ptr(), db.ptr(), 0, run.stream)
        run.done()
        what = f"bn {form} backward {M}x{C}"
        _exact_sums(run.folded(wsb, C), bw["ds"], bw["dsx"], f"{what} folded [dsum | dsumx] (channel)")
        _check_param_grads(c, dg, db, pb, None, None, what)
        assert_equal(dres.view.cpu(), (c["dy"] * keep).to(BF16), f"{what} dres == dy where y > 0 (row, channel)")
        _within(dx.view, bw["dx"], bw["mag"], True, f"{what} dx (row, channel)", "bn residual dx")
        outs.append((dx.view.cpu(), dres.view.cpu(), dg.view.cpu(), db.view.cpu()))
    for a, bb, name in zip(outs[0], outs[1], ("dx", "dres", "dgamma", "dbeta")):
        assert_equal(bb, a, f"tony_bn_bwd_res_m {name} against tony_bn_bwd_res")


# ------------------------------------------------------------------------------------- _segs forms --
@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("M", [286, 2051])
def test_bn_segs_forms_match_plain(cuda, M, n):
    """C = 88 (RPI = 23) split 24 | 8 | 40 | 16 (n = 4) into tensors of their own, each with its own row stride:
    y, the backward sums and dx are bit-identical to the plain form on the same data."""
    C = 88
    ends = SEG_SPLITS[n]
    c = _case(M, C, False, True)
    run = _Run(cuda)
    x, dy = run.src(c["x"], BF16), run.src(c["dy"], BF16)
    g, b, dt = _params(run, c, 1)
    ws = run.stats(C, "statistics")
    _k("tony_bn_stats", x.ptr(), M, C, x.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
    starts = (0,) + ends[:-1]
    pad4 = lambda v: tuple(v) + (0,) * (4 - len(v))  # noqa: E731
    # forward
    y = run.dst(M, C, BF16, "y plain")
    ysegs = [run.dst(M, e - s, BF16, f"y segment {k}") for k, (s, e) in enumerate(zip(starts, ends))]
    stat = [[run.vdst(C, F32, "save/running", torch.ones(C).double()) for _ in range(4)] for _ in range(2)]

    def tail(st):
        return (ws.ptr(), ws.ptr() + 4 * C, 2 * C, g.ptr(), b.ptr(), 1, EPS, 1, 0, st[0].ptr(), st[1].ptr(),
                st[2].ptr(), st[3].ptr(), MOM, run.stream)

    _k("tony_bn_apply", x.ptr(), M, C, x.ld, y.ptr(), y.ld, *tail(stat[0]))
    _k("tony_bn_apply_segs", x.ptr(), M, C, x.ld, n, *pad4(ends), *pad4([s.ptr() for s in ysegs]),
       *pad4([s.ld for s in ysegs]), *tail(stat[1]))
    run.done()
    _check_y(c, y.view, True, f"bn apply {M}x{C} y", "bn forward y")
    assert_equal(torch.cat([s.view for s in ysegs], 1).cpu(), y.view.cpu(), f"apply_segs n={n} y against plain")
    for a, bb in zip(stat[0], stat[1]):
        assert_equal(bb.view.cpu(), a.view.cpu(), "apply_segs saved / running statistics against plain")
    # backward: dy lives in the segments
    mu, is_ = run.vec(c["mu"], F32), run.vec(c["is_"], F32)
    dsegs = [run.src(c["dy"][:, s:e], BF16) for s, e in zip(starts, ends)]
    segargs = (n, *pad4(ends), *pad4([s.ptr() for s in dsegs]), *pad4([s.ld for s in dsegs]))
    res = []
    for segs in (False, True):
        dx = run.dst(M, C, BF16, "dx")
        dg, db = run.vdst(C, dt, "dgamma"), run.vdst(C, dt, "dbeta")
        wsb = run.stats(C, "workspace")
        mid = (M, C, mu.ptr(), is_.ptr(), g.ptr(), b.ptr(), 1, 1)
        sums = (wsb.ptr(), wsb.ptr() + 4 * C, 2 * C)
        if segs:
            _k("tony_bn_bwd_reduce_segs", x.ptr(), x.ld, *segargs, *mid, *sums, run.stream)
            _k("tony_bn_bwd_apply_segs", x.ptr(), x.ld, *segargs, dx.ptr(), dx.ld, *mid, *sums, dg.ptr(), db.ptr(), 0,
               run.stream)
        else:
            _k("tony_bn_bwd_reduce", x.ptr(), x.ld, dy.ptr(), dy.ld, *mid, *sums, run.stream)
            _k("tony_bn_bwd_apply", x.ptr(), x.ld, dy.ptr(), dy.ld, dx.ptr(), dx.ld, *mid, *sums, dg.ptr(), db.ptr(), 0,
               run.stream)
        run.done()
        _exact_sums(run.folded(wsb, C), c["bw"]["ds"], c["bw"]["dsx"], f"segs={segs} n={n} folded [dsum | dsumx]")
        _check_param_grads(c, dg, db, 1, None, None, f"segs={segs} n={n}")
        res.append(dx.view.cpu())
    _within(res[0], c["bw"]["dx"], c["bw"]["mag"], True, f"bn backward {M}x{C} dx", "bn backward dx")
    assert_equal(res[1], res[0], f"bwd_apply_segs n={n} dx against plain")


# -------------------------------------------------------------------------------------- fp32 forms --
def _check_planes(planes, C, ps, v, what, lo_exact=True):
    """[hi | lo | hi] at columns 0, ps, 2 ps: plane 2 == plane 0; with the fp32 v of the same launch,
    hi == bf16(v) and lo == bf16(v - hi); the columns between the planes keep the sentinel.
    ``lo_exact=False`` (the average pool, whose v comes from the fp32 kernel's launch): v = sum * (1/9) may be
    contracted into the subtraction v - hi as one fma, so lo holds the residual of the unrounded product -- a
    legitimate fp32 evaluation, held to the bound as hi + lo by the caller."""
    p = planes.cpu()
    hi, lo, hi2 = p[:, :C], p[:, ps:ps + C], p[:, 2 * ps:2 * ps + C]
    assert_equal(hi2, hi, f"{what}: plane 2 == plane 0")
    if ps > C:
        gap = torch.cat([p[:, C:ps], p[:, ps + C:2 * ps]], 1)
        assert_equal(gap, torch.full_like(gap, SENT), f"{what}: columns between the planes untouched")
    if v is not None:
        v = v.cpu()
        assert_equal(hi, v.to(BF16), f"{what}: hi == bf16(v)")
        if lo_exact:
            assert_equal(lo, (v - v.to(BF16).float()).to(BF16), f"{what}: lo == bf16(v - hi)")
    return hi.double() + lo.double()


@gpu
@pytest.mark.parametrize("shape", OTHER + [(1, 8), (37, 264)], ids=_sid)
def test_bn_f32_forms(cuda, shape):
    """The fp32 rows of the x3 step: statistics and backward sums exact; y / dx inside 2^-18 mag (no bf16 ulp);
    the plane forms by their construction and, as hi + lo, inside the bound + 2^-16 |ref|."""
    M, C = shape
    relu = shape != (37, 264)
    c = _case(M, C, False, relu)
    f, bw = c["f"], c["bw"]
    run = _Run(cuda)
    x, dy = run.src(c["x"], F32), run.src(c["dy"], F32)
    g, b, dt = _params(run, c, 0)
    ws = run.stats(C, "statistics")
    _k("tony_bn_stats_f32", x.ptr(), M, C, x.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
    ps = C + 16
    split = 2.0 ** -16 * f["y"].abs()
    for form in ("f32", "f32_p3", "f32_x3"):
        sm, si = run.vdst(C, F32, "save_mean"), run.vdst(C, F32, "save_invstd")
        rm0, rv0, rm, rv = _running(run, C)
        tail = (ws.ptr(), ws.ptr() + 4 * C, 2 * C, g.ptr(), b.ptr(), 0, EPS, int(relu), 0, sm.ptr(), si.ptr(), rm.ptr(),
                rv.ptr(), MOM, run.stream)
        what = f"bn {form} forward {M}x{C}"
        if form == "f32_x3":
            y3 = run.dst(M, 3 * C, BF16, "y planes")
            _k("tony_bn_apply_f32_x3", x.ptr(), M, C, x.ld, y3.ptr(), y3.ld, *tail)
            run.done()
            v = _check_planes(y3.view, C, C, None, what)
            _within(v, f["y"], f["mag"], False, f"{what} hi + lo (row, channel)", "bn fp32 y planes", extra=split)
            if relu:
                assert_equal(v == 0, f["pre"] <= 0, f"{what}: planes == 0 exactly where the pre-activation is <= 0")
        else:
            y = run.dst(M, C, F32, "y")
            if form == "f32":
                _k("tony_bn_apply_f32", x.ptr(), M, C, x.ld, y.ptr(), y.ld, *tail)
            else:
                p3 = run.dst(M, 2 * ps + C, BF16, "y planes")
                _k("tony_bn_apply_f32_p3", x.ptr(), M, C, x.ld, y.ptr(), y.ld, p3.ptr(), p3.ld, ps, *tail)
            run.done()
            _check_y(c, y.view, False, f"{what} y (row, channel)", "bn fp32 y")
            if form == "f32_p3":
                v = _check_planes(p3.view, C, ps, y.view, what)
                _within(v, f["y"], f["mag"], False, f"{what} hi + lo (row, channel)", "bn fp32 y planes", extra=split)
        _check_fwd_stats(run, c, sm, si, rm, rv, rm0, rv0, what)
    _exact_sums(run.folded(ws, C), f["sum"], f["sumsq"], f"bn f32 {M}x{C} folded [sum | sumsq] (channel)")
    # backward
    mu, is_ = run.vec(c["mu"], F32), run.vec(c["is_"], F32)
    wsb = run.stats(C, "workspace")
    mid = (M, C, mu.ptr(), is_.ptr(), g.ptr(), b.ptr(), 0, int(relu))
    sums = (wsb.ptr(), wsb.ptr() + 4 * C, 2 * C)
    _k("tony_bn_bwd_reduce_f32", x.ptr(), x.ld, dy.ptr(), dy.ld, *mid, *sums, run.stream)
    run.done()
    _exact_sums(run.folded(wsb, C), bw["ds"], bw["dsx"], f"bn f32 {M}x{C} folded [dsum | dsumx] (channel)")
    split = 2.0 ** -16 * bw["dx"].abs()
    for form in ("f32", "f32_x3", "f32_x3p"):
        dg, db = run.vdst(C, F32, "dgamma"), run.vdst(C, F32, "dbeta")
        what = f"bn {form} backward {M}x{C}"
        if form == "f32":
            dx = run.dst(M, C, F32, "dx")
            _k("tony_bn_bwd_apply_f32", x.ptr(), x.ld, dy.ptr(), dy.ld, dx.ptr(), dx.ld, *mid, *sums, dg.ptr(),
               db.ptr(), 0, run.stream)
            run.done()
            _within(dx.view, bw["dx"], bw["mag"], False, f"{what} dx (row, channel)", "bn fp32 dx")
        else:
            pst = C if form == "f32_x3" else ps
            dx3 = run.dst(M, 2 * pst + C, BF16, "dx planes")
            extra = () if form == "f32_x3" else (pst,)
            _k("tony_bn_bwd_apply_" + form, x.ptr(), x.ld, dy.ptr(), dy.ld, dx3.ptr(), dx3.ld, *extra, *mid, *sums,
               dg.ptr(), db.ptr(), 0, run.stream)
            run.done()
            v = _check_planes(dx3.view, C, pst, None, what)
            _within(v, bw["dx"], bw["mag"], False, f"{what} hi + lo (row, channel)", "bn fp32 dx planes", extra=split)
        _check_param_grads(c, dg, db, 0, None, None, what)


# ------------------------------------------------------------------------------------------- pools --
def _ints(shape, amp, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def _pool_planes(N, C, H, W):
    """[N, C, H, W] float64: every (n, c) plane a permutation of distinct bf16-exact integers (H W <= 511), so no
    window has a tied maximum; and integer gradients are made by the callers."""
    assert H * W <= 511
    gen = torch.Generator().manual_seed(N * 1000 + C * 100 + H * 10 + W)
    x = torch.stack([torch.randperm(H * W, generator=gen) for _ in range(N * C)]).double() - (H * W) // 2
    x = x.view(N, C, H, W)
    assert _is_bf16(x)
    return x


def _max_ref(x, K, S, P):
    """float64 max pool: values and the window tap kh * K + kw of the maximum."""
    N, C, H, W = x.shape
    y, idx = F.max_pool2d(x, K, S, P, return_indices=True)
    OH, OW = y.shape[2:]
    ih, iw = idx // W, idx % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    tap = (ih - (oh * S - P)) * K + (iw - (ow * S - P))
    return y, tap.to(torch.uint8)


def _scatter_by_tap(dyp, tap, H, W, K, S, P):
    """The max-pool backward from the argmax bytes: dX[n, c, ih, iw] += dY[n, c, oh, ow] (float64, NCHW)."""
    N, C, OH, OW = dyp.shape
    t = tap.long()
    ih = torch.arange(OH).view(1, 1, OH, 1) * S - P + t // K
    iw = torch.arange(OW).view(1, 1, 1, OW) * S - P + t % K
    assert (ih >= 0).all() and (ih < H).all() and (iw >= 0).all() and (iw < W).all()
    dx = torch.zeros(N, C, H * W, dtype=F64)
    dx.scatter_add_(2, (ih * W + iw).view(N, C, -1), dyp.reshape(N, C, -1))
    return dx.view(N, C, H, W)


def _nchw(rows, N, H, W):
    return rows.view(N, H, W, -1).permute(0, 3, 1, 2)


MAXPOOL = [(2, 8, 9, 7, 3, 2, 0), (2, 8, 9, 7, 3, 2, 1), (2, 40, 15, 17, 3, 2, 0), (2, 40, 15, 17, 3, 2, 1),
           (2, 40, 9, 7, 2, 1, 1), (2, 8, 15, 17, 5, 3, 0), (2, 40, 9, 7, 2, 2, 0), (2, 8, 9, 7, 3, 1, 1)]


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", MAXPOOL, ids=_sid)
def test_maxpool_exact(cuda, shape, f32):
    N, C, H, W, K, S, P = shape
    dt, sfx = (F32, "_f32") if f32 else (BF16, "")
    x = _pool_planes(N, C, H, W)
    yr, tapr = _max_ref(x, K, S, P)
    OH, OW = yr.shape[2:]
    run = _Run(cuda)
    xs = run.src(pix_rows(x), dt)
    y = run.dst(N * OH * OW, C, dt, "y")
    arg = run.dst(1, N * OH * OW * C, torch.uint8, "argmax", c0=0, fill=0xAB)
    _k("tony_maxpool_fwd" + sfx, xs.ptr(), y.ptr(), arg.ptr(), N, H, W, C, K, S, P, xs.ld, y.ld, run.stream)
    run.done()
    what = f"maxpool{sfx} {_sid(shape)}"
    assert_equal(y.view.cpu(), pix_rows(yr).to(dt), f"{what} y (output pixel, channel)")
    assert_equal(arg.view.cpu().view(-1, C), pix_rows(tapr), f"{what} argmax tap kh * K + kw (output pixel, channel)")
    dyp = _ints((N, C, OH, OW), 3, 11)
    dxr = _scatter_by_tap(dyp, tapr, H, W, K, S, P)
    pre = _ints((N, C, H, W), 5, 12)
    ds = run.src(pix_rows(dyp), dt)
    dx = run.dst(N * H * W, C, dt, "dx")
    _k("tony_maxpool_bwd" + sfx, ds.ptr(), arg.ptr(), dx.ptr(), N, H, W, C, K, S, P, ds.ld, dx.ld, run.stream)
    dxa = run.dst(N * H * W, C, dt, "dx accumulated")
    dxa.view.copy_(pix_rows(pre).to(dt))
    _k("tony_maxpool_bwd_acc" + sfx, ds.ptr(), arg.ptr(), dxa.ptr(), N, H, W, C, K, S, P, ds.ld, dxa.ld, run.stream)
    run.done()
    assert_equal(dx.view.cpu(), pix_rows(dxr).to(dt), f"{what} dx (pixel, channel)")
    assert_equal(dxa.view.cpu(), pix_rows(pre + dxr).to(dt), f"{what} dx added into an integer pre-fill")


BOX = [(2, 16, 1, 1), (2, 16, 2, 5), (2, 40, 9, 7)]


@gpu
@pytest.mark.parametrize("shape", BOX, ids=_sid)
def test_avgpool3_forms(cuda, shape):
    """avg 3x3 / s1 / p1 (count_include_pad) on images that are all border: bf16, fp32, the accumulating forms
    and the x3 planes."""
    N, C, H, W = shape
    x = _ints(shape, 4, 21)
    ref, mag = F.avg_pool2d(x, 3, 1, 1), F.avg_pool2d(x.abs(), 3, 1, 1)
    pre = _ints(shape, 5, 22)
    R, rr, mm, pp = N * H * W, pix_rows(ref), pix_rows(mag), pix_rows(pre)
    run = _Run(cuda)
    what = f"avgpool3 {_sid(shape)}"
    for dt, sfx in ((BF16, ""), (F32, "_f32")):
        xs = run.src(pix_rows(x), dt)
        y, ya = run.dst(R, C, dt, "y"), run.dst(R, C, dt, "y accumulated")
        ya.view.copy_(pp.to(dt))
        _k("tony_avgpool3_s1p1" + sfx, xs.ptr(), y.ptr(), N, H, W, C, xs.ld, y.ld, run.stream)
        _k("tony_avgpool3_s1p1_acc", xs.ptr(), ya.ptr(), N, H, W, C, xs.ld, ya.ld, int(dt == F32), run.stream)
        run.done()
        _within(y.view, rr, mm, dt == BF16, f"{what}{sfx} y (pixel, channel)", "avg pool")
        _within(ya.view, pp + rr, pp.abs() + mm, dt == BF16, f"{what}{sfx} y added into a pre-fill", "avg pool")
    ps = C + 8
    y3, y3p = run.dst(R, 3 * C, BF16, "planes", c0=0), run.dst(R, 2 * ps + C, BF16, "wide planes")
    _k("tony_avgpool3_s1p1_x3", xs.ptr(), y3.ptr(), N, H, W, C, xs.ld, run.stream)
    _k("tony_avgpool3_s1p1_x3p", xs.ptr(), y3p.ptr(), N, H, W, C, xs.ld, y3p.ld, ps, run.stream)
    run.done()
    for pl, pst, name in ((y3, C, "x3"), (y3p, ps, "x3p")):
        v = _check_planes(pl.view, C, pst, y.view, f"{what} {name}", lo_exact=False)  # y: the fp32 form's output
        _within(v, rr, mm, False, f"{what} {name} hi + lo", "avg pool planes", extra=2.0 ** -16 * rr.abs())


AVG = [(2, 16, 17, 17, 5, 3), (2, 16, 8, 8, 8, 1), (2, 16, 1, 1, 1, 1), (2, 16, 9, 7, 3, 2)]


@gpu
@pytest.mark.parametrize("shape", AVG, ids=_sid)
def test_avgpool_kxk(cuda, shape):
    N, C, H, W, K, S = shape
    x = _ints((N, C, H, W), 4, 31)
    ref, mag = F.avg_pool2d(x, K, S), F.avg_pool2d(x.abs(), K, S)
    OH, OW = ref.shape[2:]
    dyp = _ints((N, C, OH, OW), 3, 32)

    def back(d):  # the gradient of avg_pool2d is linear in dy: the same routine gives its magnitude from |dy|
        xx = torch.zeros_like(x, requires_grad=True)
        F.avg_pool2d(xx, K, S).backward(d)
        return xx.grad

    dxr, dmag = back(dyp), back(dyp.abs())
    run = _Run(cuda)
    for dt, sfx in ((BF16, ""), (F32, "_f32")):
        xs, ds = run.src(pix_rows(x), dt), run.src(pix_rows(dyp), dt)
        y, dx = run.dst(N * OH * OW, C, dt, "y"), run.dst(N * H * W, C, dt, "dx")
        _k("tony_avgpool_fwd" + sfx, xs.ptr(), y.ptr(), N, H, W, C, K, S, xs.ld, y.ld, run.stream)
        _k("tony_avgpool_bwd" + sfx, ds.ptr(), dx.ptr(), N, H, W, C, K, S, ds.ld, dx.ld, run.stream)
        run.done()
        _within(y.view, pix_rows(ref), pix_rows(mag), dt == BF16, f"avgpool{sfx} {_sid(shape)} y", "avg pool")
        _within(dx.view, pix_rows(dxr), pix_rows(dmag), dt == BF16, f"avgpool{sfx} {_sid(shape)} dx", "avg pool")


# ------------------------------------------------------ BN + ReLU + max pool, forward and backward --
FUSED = [(2, 8, 9, 7, 3, 2, 0), (2, 8, 9, 7, 3, 2, 1), (2, 40, 15, 17, 3, 2, 0), (2, 40, 15, 17, 3, 2, 1),
         (2, 40, 9, 7, 2, 1, 0), (2, 40, 9, 7, 2, 1, 1), (2, 8, 15, 17, 5, 3, 0), (2, 8, 15, 17, 5, 3, 1)]


@gpu
@pytest.mark.parametrize("shape", FUSED, ids=_sid)
def test_bn_relu_maxpool_fused_forward_and_backward(cuda, shape):
    """tony_bn_relu_maxpool == tony_bn_apply + tony_maxpool_fwd on the same statistics buffer, bit for bit (K = 3:
    the compile-time window; K = 2, 5: the runtime window).  Then the pool backward with the BN reduction fused
    (tony_maxpool_bwd_bnred: exact sums, dX == tony_maxpool_bwd) and the BN apply that gathers the pooled gradient
    (tony_bn_bwd_pool_apply == tony_bn_bwd_apply on the stored dY; C = 8 at 9x7: RPI = 256 > H W)."""
    N, C, H, W, K, S, P = shape
    M = N * H * W
    pb = FUSED.index(shape) % 2
    c = _case(M, C, False, True)
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    MO = N * OH * OW
    run = _Run(cuda)
    z = run.src(c["x"], BF16)
    g, b, dt = _params(run, c, pb)
    ws = run.stats(C, "statistics")
    _k("tony_bn_stats", z.ptr(), M, C, z.ld, ws.ptr(), ws.ptr() + 4 * C, 2 * C, run.stream)
    yfull = run.dst(M, C, BF16, "y full resolution")
    yp = [run.dst(MO, C, BF16, "pooled y") for _ in range(2)]
    arg = [run.dst(1, MO * C, torch.uint8, "argmax", c0=0, fill=0xAB) for _ in range(2)]
    stat = [[run.vdst(C, F32, "save/running", torch.ones(C).double()) for _ in range(4)] for _ in range(2)]
    sums = (ws.ptr(), ws.ptr() + 4 * C, 2 * C)
    _k("tony_bn_apply", z.ptr(), M, C, z.ld, yfull.ptr(), yfull.ld, *sums, g.ptr(), b.ptr(), pb, EPS, 1, 0,
       *[s.ptr() for s in stat[0]], MOM, run.stream)
    _k("tony_maxpool_fwd", yfull.ptr(), yp[0].ptr(), arg[0].ptr(), N, H, W, C, K, S, P, yfull.ld, yp[0].ld, run.stream)
    _k("tony_bn_relu_maxpool", z.ptr(), z.ld, *sums, g.ptr(), b.ptr(), pb, EPS, *[s.ptr() for s in stat[1]], MOM,
       yp[1].ptr(), yp[1].ld, arg[1].ptr(), N, H, W, C, K, S, P, run.stream)
    run.done()
    what = f"bn+relu+maxpool {_sid(shape)}"
    _check_y(c, yfull.view, True, f"{what} unfused y", "bn forward y")
    assert_equal(yp[1].view.cpu(), yp[0].view.cpu(), f"{what} fused pooled y against apply + maxpool_fwd")
    assert_equal(arg[1].view.cpu(), arg[0].view.cpu(), f"{what} fused argmax against apply + maxpool_fwd")
    for a, bb in zip(stat[0], stat[1]):
        assert_equal(bb.view.cpu(), a.view.cpu(), f"{what} fused saved / running statistics against tony_bn_apply")
    # the pooled value against float64: max over the window of the reference (ReLU outputs are >= 0, so the ulp of
    # the window maximum bounds every tap's), with the window's largest mag
    f = c["f"]
    yr = F.max_pool2d(_nchw(f["y"], N, H, W), K, S, P)
    mg = F.max_pool2d(_nchw(f["mag"], N, H, W), K, S, P)
    _within(yp[1].view, pix_rows(yr), pix_rows(mg), True, f"{what} pooled y", "bn + pool y")
    # ---- backward, with the caller's integer mean / power-of-two invstd
    tap = _nchw(arg[1].view.cpu().view(MO, C), N, OH, OW)
    assert int(tap.max()) < K * K
    dyp = _ints((N, C, OH, OW), 3, 41)
    dfull = pix_rows(_scatter_by_tap(dyp, tap, H, W, K, S, P))  # integers, |.| <= 3 ceil(K / S)^2: bf16-exact
    bw = _bwd_ref(c["x"], dfull, c["g"], c["b"], c["mu"], c["is_"], True)
    mu, is_ = run.vec(c["mu"], F32), run.vec(c["is_"], F32)
    ds = run.src(pix_rows(dyp), BF16)
    dxp = run.dst(M, C, BF16, "pool dX")
    dxp2 = run.dst(M, C, BF16, "pool dX (tony_maxpool_bwd)")
    wsb = [run.stats(C, "workspace") for _ in range(2)]
    geo = (N, H, W, C, K, S, P)
    bn = (mu.ptr(), is_.ptr(), g.ptr(), b.ptr(), pb, 1)
    ncu = _L().num_cus(cuda)
    _k("tony_maxpool_bwd_bnred", ds.ptr(), arg[1].ptr(), dxp.ptr(), *geo, ds.ld, dxp.ld, z.ptr(), z.ld, *bn,
       wsb[0].ptr(), 2 * C, ncu, run.stream)
    _k("tony_maxpool_bwd_bnred", ds.ptr(), arg[1].ptr(), 0, *geo, ds.ld, 0, z.ptr(), z.ld, *bn, wsb[1].ptr(), 2 * C,
       ncu, run.stream)  # no dX store: the reduction only
    _k("tony_maxpool_bwd", ds.ptr(), arg[1].ptr(), dxp2.ptr(), *geo, ds.ld, dxp2.ld, run.stream)
    run.done()
    assert_equal(dxp.view.cpu(), dfull.to(BF16), f"{what} bnred dX (pixel, channel)")
    assert_equal(dxp2.view.cpu(), dxp.view.cpu(), f"{what} tony_maxpool_bwd dX against bnred's")
    for w_ in wsb:
        _exact_sums(run.folded(w_, C), bw["ds"], bw["dsx"], f"{what} bnred folded [dsum | dsumx] (channel)")
    gen = torch.Generator().manual_seed(M)
    pre_g = torch.randint(-8, 9, (C,), generator=gen).double()
    pre_b = torch.randint(-8, 9, (C,), generator=gen).double()
    out = []
    for form in ("pool_apply", "apply"):
        dz = run.dst(M, C, BF16, f"dz {form}")
        dg, db = run.vdst(C, dt, "dgamma", pre_g), run.vdst(C, dt, "dbeta", pre_b)
        if form == "pool_apply":
            _k("tony_bn_bwd_pool_apply", ds.ptr(), ds.ld, arg[1].ptr(), *geo, z.ptr(), z.ld, dz.ptr(), dz.ld, *bn,
               wsb[1].ptr(), 2 * C, dg.ptr(), db.ptr(), 1, run.stream)
        else:
            _k("tony_bn_bwd_apply", z.ptr(), z.ld, dxp.ptr(), dxp.ld, dz.ptr(), dz.ld, M, C, *bn, wsb[0].ptr(),
               wsb[0].ptr() + 4 * C, 2 * C, dg.ptr(), db.ptr(), 1, run.stream)
        run.done()
        cc = dict(c, bw=bw)
        _check_param_grads(cc, dg, db, pb, pre_g, pre_b, f"{what} {form}")
        _within(dz.view, bw["dx"], bw["mag"], True, f"{what} {form} dz (pixel, channel)", "bn + pool dz")
        out.append(dz.view.cpu())
    assert_equal(out[0], out[1], f"{what} tony_bn_bwd_pool_apply dz against tony_bn_bwd_apply on the stored dY")


# ------------------------------------------------------------------------------ contract refusals --
@gpu
def test_contract_violations_are_refused_and_write_nothing(cuda):
    """C % 8 != 0, C > 2048, a row stride that is no multiple of a vector, a segment table that does not end at
    C: the entry point returns -1 before any launch, the sentinel destinations stay untouched."""
    run = _Run(cuda)
    M, C = 16, 16
    x = run.src(torch.zeros(M, 2064, dtype=F64), BF16)
    xf = run.src(torch.zeros(M, 64, dtype=F64), F32)
    y, yf = run.dst(M, 2064, BF16, "y"), run.dst(M, 64, F32, "y fp32")
    ws = run.stats(2056, "statistics")
    ws.view.fill_(SENT)
    v = [run.vdst(2056, F32, "vector") for _ in range(6)]
    arg = run.dst(1, M * 64, torch.uint8, "argmax", c0=0, fill=0xAB)
    s = run.stream
    st = lambda Cc: (ws.ptr(), ws.ptr() + 4 * Cc, 2 * Cc)  # noqa: E731
    tail = (v[0].ptr(), v[1].ptr(), 0, EPS, 1, 0, v[2].ptr(), v[3].ptr(), v[4].ptr(), v[5].ptr(), MOM, s)
    for Cc, ld in ((12, x.ld), (2056, x.ld), (C, x.ld + 4)):
        _k("tony_bn_stats", x.ptr(), M, Cc, ld, *st(Cc), s, rc=-1)
        _k("tony_bn_apply", x.ptr(), M, Cc, ld, y.ptr(), y.ld, *st(Cc), *tail, rc=-1)
        _k("tony_bn_apply_res", x.ptr(), M, Cc, ld, x.ptr(), x.ld, y.ptr(), y.ld, *st(Cc), *tail, rc=-1)
        _k("tony_bn_bwd_reduce", x.ptr(), ld, x.ptr(), x.ld, M, Cc, v[0].ptr(), v[1].ptr(), v[0].ptr(), v[1].ptr(), 0,
           1, *st(Cc), s, rc=-1)
        _k("tony_bn_bwd_apply", x.ptr(), ld, x.ptr(), x.ld, y.ptr(), y.ld, M, Cc, v[0].ptr(), v[1].ptr(), v[0].ptr(),
           v[1].ptr(), 0, 1, *st(Cc), v[2].ptr(), v[3].ptr(), 0, s, rc=-1)
        _k("tony_bn_bwd_onepass", x.ptr(), ld, x.ptr(), x.ld, y.ptr(), y.ld, M, Cc, v[0].ptr(), v[1].ptr(), v[0].ptr(),
           v[1].ptr(), 0, 1, ws.ptr(), v[2].ptr(), v[3].ptr(), 0, ws.ptr(), 8, s, rc=-1)
        _k("tony_bn_relu_maxpool", x.ptr(), ld, *st(Cc), v[0].ptr(), v[1].ptr(), 0, EPS, v[2].ptr(), v[3].ptr(),
           v[4].ptr(), v[5].ptr(), MOM, y.ptr(), y.ld, arg.ptr(), 1, 4, 4, Cc, 3, 2, 0, s, rc=-1)
    for Cc, ld in ((12, xf.ld), (C, xf.ld + 2)):
        _k("tony_bn_stats_f32", xf.ptr(), M, Cc, ld, *st(Cc), s, rc=-1)
        _k("tony_bn_apply_f32", xf.ptr(), M, Cc, ld, yf.ptr(), yf.ld, *st(Cc), *tail, rc=-1)
        _k("tony_bn_bwd_apply_f32", xf.ptr(), ld, xf.ptr(), xf.ld, yf.ptr(), yf.ld, M, Cc, v[0].ptr(), v[1].ptr(),
           v[0].ptr(), v[1].ptr(), 0, 1, *st(Cc), v[2].ptr(), v[3].ptr(), 0, s, rc=-1)
    # planes narrower than 3 C / 2 pstride + C
    _k("tony_bn_apply_f32_x3", xf.ptr(), M, C, xf.ld, y.ptr(), 3 * C - 8, *st(C), *tail, rc=-1)
    _k("tony_bn_apply_f32_p3", xf.ptr(), M, C, xf.ld, yf.ptr(), yf.ld, y.ptr(), 3 * C, C - 8, *st(C), *tail, rc=-1)
    _k("tony_bn_bwd_apply_f32_x3p", xf.ptr(), xf.ld, xf.ptr(), xf.ld, y.ptr(), 2 * 24 + C - 8, 24, M, C, v[0].ptr(),
       v[1].ptr(), v[0].ptr(), v[1].ptr(), 0, 1, *st(C), v[2].ptr(), v[3].ptr(), 0, s, rc=-1)
    # segment tables: not ending at C, not increasing, an end that is no multiple of 8, n out of range
    bad_tables = ((2, (8, 24, 0, 0)), (2, (16, 16, 0, 0)), (2, (4, 16, 0, 0)), (5, (8, 16, 0, 0)), (0, (16, 0, 0, 0)))
    for n, ends in bad_tables:
        seg = (n, *ends, y.ptr(), y.ptr(), y.ptr(), y.ptr(), y.ld, y.ld, y.ld, y.ld)
        _k("tony_bn_apply_segs", x.ptr(), M, C, x.ld, *seg, *st(C), *tail, rc=-1)
        _k("tony_bn_bwd_reduce_segs", x.ptr(), x.ld, *seg, M, C, v[0].ptr(), v[1].ptr(), v[0].ptr(), v[1].ptr(), 0, 1,
           *st(C), s, rc=-1)
        _k("tony_bn_bwd_apply_segs", x.ptr(), x.ld, *seg, y.ptr(), y.ld, M, C, v[0].ptr(), v[1].ptr(), v[0].ptr(),
           v[1].ptr(), 0, 1, *st(C), v[2].ptr(), v[3].ptr(), 0, s, rc=-1)
    # pools: C % 8, a bad ld, a window larger than the padded image, too much padding
    for Cc, ld, K, P in ((12, x.ld, 3, 0), (C, x.ld + 4, 3, 0), (C, x.ld, 7, 0), (C, x.ld, 3, 2)):
        _k("tony_maxpool_fwd", x.ptr(), y.ptr(), arg.ptr(), 1, 4, 4, Cc, K, 2, P, ld, y.ld, s, rc=-1)
        _k("tony_maxpool_bwd", x.ptr(), arg.ptr(), y.ptr(), 1, 4, 4, Cc, K, 2, P, ld, y.ld, s, rc=-1)
        _k("tony_maxpool_bwd_acc", x.ptr(), arg.ptr(), y.ptr(), 1, 4, 4, Cc, K, 2, P, ld, y.ld, s, rc=-1)
        _k("tony_maxpool_bwd_bnred", x.ptr(), arg.ptr(), y.ptr(), 1, 4, 4, Cc, K, 2, P, ld, y.ld, x.ptr(), x.ld,
           v[0].ptr(), v[1].ptr(), v[0].ptr(), v[1].ptr(), 0, 1, ws.ptr(), 2 * Cc, 8, s, rc=-1)
        _k("tony_bn_bwd_pool_apply", x.ptr(), ld, arg.ptr(), 1, 4, 4, Cc, K, 2, P, x.ptr(), x.ld, y.ptr(), y.ld,
           v[0].ptr(), v[1].ptr(), v[0].ptr(), v[1].ptr(), 0, 1, ws.ptr(), 2 * Cc, v[2].ptr(), v[3].ptr(), 0, s, rc=-1)
    for Cc, ld in ((12, x.ld), (C, x.ld + 4)):
        _k("tony_avgpool3_s1p1", x.ptr(), y.ptr(), 1, 4, 4, Cc, ld, y.ld, s, rc=-1)
        _k("tony_avgpool3_s1p1_acc", x.ptr(), y.ptr(), 1, 4, 4, Cc, ld, y.ld, 0, s, rc=-1)
        _k("tony_avgpool_fwd", x.ptr(), y.ptr(), 1, 4, 4, Cc, 2, 2, ld, y.ld, s, rc=-1)
        _k("tony_avgpool_bwd", x.ptr(), y.ptr(), 1, 4, 4, Cc, 2, 2, ld, y.ld, s, rc=-1)
    _k("tony_avgpool_fwd", x.ptr(), y.ptr(), 1, 4, 4, C, 5, 1, x.ld, y.ld, s, rc=-1)  # window larger than the image
    _k("tony_avgpool3_s1p1_x3p", xf.ptr(), y.ptr(), 1, 4, 4, C, xf.ld, 2 * 24 + C - 8, 24, s, rc=-1)
    run.done()
    for slab, what in run.dsts:
        inner = slab.view.cpu()
        assert_equal(inner, torch.full_like(inner, slab.fill), f"refused call wrote into {what}")


# ------------------------------------------------------------------------------ the public wrappers --
def _cl(t, dtype, dev):
    return t.to(dtype).to(dev).contiguous(memory_format=torch.channels_last)


@gpu
def test_public_wrappers_bn(cuda):
    """One pass through ops.bn.bn_act and ops.residual.bn_add_relu: the autograd wiring around the kernels above.
    The backward runs on the batch's own (inexact) mean / invstd, so dgamma and dx are held to the bound with
    sum |dy'| (|x| + |mean|) is in place of sum |dy' xhat| (each xhat carries a relative fp32 error of its two
    terms, not of their difference); dbeta stays exact."""
    from tony_amd.ops.bn import bn_act
    from tony_amd.ops.residual import bn_add_relu

    N, C, H, W = 2, 40, 11, 13
    M = N * H * W
    for res in (False, True):
        c = _case(M, C, res, True)
        f = c["f"]
        x = _cl(_nchw(c["x"], N, H, W), BF16, cuda).requires_grad_(True)
        g = torch.nn.Parameter(c["g"].float().to(cuda))
        b = torch.nn.Parameter(c["b"].float().to(cuda))
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        if res:
            r = _cl(_nchw(c["res"], N, H, W), BF16, cuda).requires_grad_(True)
            y = bn_add_relu(x, r, g, b, rm, rv, True, MOM, EPS)
        else:
            y = bn_act(x, g, b, rm, rv, True, MOM, EPS, True)
        y.backward(_cl(_nchw(c["dy"], N, H, W), BF16, cuda))
        torch.cuda.synchronize()
        what = "bn_add_relu" if res else "bn_act"
        yr = pix_rows(y.detach())
        _check_y(c, yr, True, f"{what} y", "wrappers")
        keep = yr.cpu() > 0
        xhat = (c["x"] - f["mean"]) * f["invstd"]
        d = c["dy"] * keep
        ds, dsx = d.sum(0), (d * xhat).sum(0)
        k = c["g"] * f["invstd"]
        loose = (d.abs() * (c["x"].abs() + f["mean"].abs()) * f["invstd"]).sum(0)
        dxr = k * (d - ds / M - xhat * dsx / M)
        mag = k.abs() * (d.abs() + ds.abs() / M + (c["x"].abs() + f["mean"].abs()) * f["invstd"] * loose / M)
        assert_equal(b.grad.cpu(), ds.float(), f"{what} dbeta")
        _within(g.grad, dsx, loose, False, f"{what} dgamma", "wrappers")
        _within(pix_rows(x.grad), dxr, mag, True, f"{what} dx", "wrappers")
        if res:
            assert_equal(pix_rows(r.grad).cpu(), d.to(BF16), f"{what} dres")
        _rel20(rm, MOM * f["mean"], MOM * f["absx"], f"{what} running_mean")


@gpu
def test_public_wrappers_pools(cuda):
    from tony_amd.ops.pool import avg_pool, avg_pool3x3_s1, max_pool

    N, C, H, W = 2, 40, 9, 7
    xp = _pool_planes(N, C, H, W)
    for K, S, P in ((3, 2, 0), (3, 2, 1), (2, 1, 0)):
        x = _cl(xp, BF16, cuda).requires_grad_(True)
        y = max_pool(x, K, S, padding=P)
        yr, tap = _max_ref(xp, K, S, P)
        dyp = _ints(tuple(yr.shape), 3, 51)
        y.backward(_cl(dyp, BF16, cuda))
        assert_equal(y.detach().cpu(), yr.to(BF16), f"max_pool {K}/{S} p{P} y")
        assert_equal(x.grad.cpu(), _scatter_by_tap(dyp, tap, H, W, K, S, P).to(BF16), f"max_pool {K}/{S} p{P} dx")
    xi = _ints((N, C, H, W), 4, 52)
    for dt in (BF16, F32):
        for name, fn, ref in (("avg_pool3x3_s1", avg_pool3x3_s1, lambda t: F.avg_pool2d(t, 3, 1, 1)),
                              ("avg_pool 3/2", lambda t: avg_pool(t, 3, 2), lambda t: F.avg_pool2d(t, 3, 2))):
            x = _cl(xi, dt, cuda).requires_grad_(True)
            y = fn(x)
            x64 = xi.clone().requires_grad_(True)
            y64 = ref(x64)
            dyp = _ints(tuple(y64.shape), 3, 53)
            y.backward(_cl(dyp, dt, cuda))
            y64.backward(dyp)
            a64 = torch.zeros_like(xi, requires_grad=True)
            ref(a64).backward(dyp.abs())
            _within(y.detach(), y64.detach(), ref(xi.abs()), dt == BF16, f"{name} {dt} y", "wrappers")
            _within(x.grad, x64.grad, a64.grad, dt == BF16, f"{name} {dt} dx", "wrappers")


@gpu
def test_public_wrapper_conv_bn_act_pool(cuda):
    """ops.conv.conv_bn_act_pool (conv -> BN -> ReLU -> max pool 3x3/2): with two +-1 taps per output channel the
    conv output z is a small exact integer, so the pooled y is held to the bound and dbeta to equality."""
    from tony_amd.ops.conv import conv_bn_act_pool

    N, Ci, H, W, Co = 2, 32, 37, 37, 64
    gen = torch.Generator().manual_seed(61)
    xi = torch.randint(-1, 2, (N, Ci, H, W), generator=gen).double()
    wt = torch.zeros(Co, Ci * 9, dtype=F64)
    for co in range(Co):
        taps = torch.randperm(Ci * 9, generator=gen)[:2]
        wt[co, taps] = torch.tensor([1.0, -1.0 if co % 2 else 1.0], dtype=F64)
    wt = wt.view(Co, Ci, 3, 3)
    gam = torch.randint(4, 13, (Co,), generator=gen).double() / 8
    bet = torch.randint(1, 9, (Co,), generator=gen).double() / 16
    z = pix_rows(F.conv2d(xi, wt, None, 1, 1))
    M = z.shape[0]
    for _ in range(300):  # the ReLU margin, as in _case
        f = _fwd_ref(z, gam, bet, True)
        offend = (f["pre"].abs() <= 2.0 ** -10 * f["mag"]).any(0)
        if not offend.any():
            break
        bet[offend] += 1.0 / 256
    assert (f["pre"].abs() > 2.0 ** -10 * f["mag"]).all() and (f["ex2"] <= 4 * f["var"]).all()
    x = _cl(xi, BF16, cuda)
    w = torch.nn.Parameter(_cl(wt, BF16, cuda))
    g, b = torch.nn.Parameter(gam.float().to(cuda)), torch.nn.Parameter(bet.float().to(cuda))
    rm, rv = torch.zeros(Co, device=cuda), torch.ones(Co, device=cuda)
    y = conv_bn_act_pool(x, w, g, b, rm, rv, 1, 1, MOM, EPS, 3, 2)
    yfull = _nchw(f["y"], N, H, W)
    yr, idx = F.max_pool2d(yfull, 3, 2, 0, return_indices=True)
    mg = F.max_pool2d(_nchw(f["mag"], N, H, W), 3, 2, 0)
    dyp = _ints(tuple(yr.shape), 3, 62)
    y.backward(_cl(dyp, BF16, cuda))
    torch.cuda.synchronize()
    _within(y.detach(), yr, mg, True, "conv_bn_act_pool y", "wrappers")
    # dbeta = sum of the pooled gradient routed to each window's first maximum, where the ReLU passes (y > 0):
    # equal z give equal y in the kernel and in float64, different z differ by far more than a bf16 ulp, so the
    # first maximum is the same tap in both
    dfull = torch.zeros_like(yfull).view(N, Co, -1).scatter_add_(2, idx.view(N, Co, -1), dyp.view(N, Co, -1))
    dfull = dfull.view_as(yfull) * (yfull > 0)
    assert_equal(b.grad.cpu(), dfull.sum((0, 2, 3)).float(), "conv_bn_act_pool dbeta")
    _rel20(rm, MOM * f["mean"], MOM * f["absx"], "conv_bn_act_pool running_mean")


# ------------------------------------------------------------------------------------ the closing test --
@gpu
def test_zz_every_entry_point_ran(cuda):
    """Every tony_bn_* / tony_maxpool_* / tony_avgpool* entry point of _lib._SIGNATURES was called directly by
    some case of this module (run as a whole): a later entry point cannot arrive untested."""
    names = sorted(n for n in _L()._SIGNATURES if n.startswith(("tony_bn_", "tony_maxpool_", "tony_avgpool")))
    assert len(names) >= 41
    for fam, worst in sorted(_WORST.items()):
        print(f"largest excess / (2^-18 mag), {fam}: {worst:.4f}")
    missing = [n for n in names if n not in _CALLED]
    assert not missing, f"entry points no case of this module called: {missing}"
