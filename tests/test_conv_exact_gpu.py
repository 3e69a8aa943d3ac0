"""Bit-exact, poisoned-surroundings tests of every conv / GEMM tile variant.

Operands are small integers ({-2..2}) held in bf16, so every bf16 product and every fp32 partial sum of
a correct kernel is an exact integer: the output is determined bit for bit whatever the MFMA, split-K
or atomics order, and equals the float64 reference rounded ONCE to the output dtype.  The BN statistics
of the epilogues are sums of the fp32 accumulators, exact integers too.  Every check is ``torch.equal``
on the whole tensor; a failure prints the count and the first coordinates of the differing elements.

Part A pins every tile variant (0-31, and 9 / 10 / 40 on their own shapes) at conv level, part B runs
the C entry points on operands that are channel slices of NaN-filled allocations with sentinel-filled
destinations (no read of a NaN may reach an output, no byte outside the destination may change), part C
does the same for the Python-level slice producers and consumers.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from exact_helpers import SENT as _SENT
from exact_helpers import Slab as _Slab
from exact_helpers import assert_equal as _assert_equal
from exact_helpers import pix_rows as _pix_rows
from exact_helpers import poisoned as _poisoned

pytestmark = pytest.mark.gpu

_BF16 = torch.bfloat16
_EXACT = 2 ** 24  # integers below this magnitude are exact in fp32

# (N, Cin, H, W, Cout, (R, S), stride, (ph, pw))
S1_SHAPES = [
    (2, 40, 13, 11, 88, (3, 3), 1, (1, 1)),    # M = 286: partial row tile; K = 360; partial 32-column granule
    (1, 64, 9, 9, 64, (3, 3), 1, (0, 0)),      # M = 49 < every tile; uniform-tap
    (3, 96, 10, 7, 224, (1, 7), 1, (0, 3)),    # Cout above the 192-column cap: two uneven column tiles; 1 x T
    (2, 128, 6, 6, 32, (1, 1), 1, (0, 0)),     # 1x1, a single 32-column tile
    (2, 64, 17, 19, 64, (5, 5), 1, (2, 2)),    # uniform-tap for the 64-deep K-step variants; M = 646
    (2, 448, 8, 8, 384, (3, 3), 1, (1, 1)),    # long K (4032), several column tiles
]
STRIDED_SHAPES = [
    (2, 64, 15, 15, 64, (3, 3), 2, (0, 0)),
    (2, 32, 14, 14, 96, (3, 3), 2, (1, 1)),
    (2, 64, 10, 10, 128, (1, 1), 2, (0, 0)),   # tap-less residue classes
    (1, 32, 11, 11, 64, (5, 5), 3, (2, 2)),    # nine classes
    (2, 24, 14, 14, 40, (3, 3), 2, (1, 1)),    # Cout % 32 != 0: only the register-staged variants 0-8
]
ALL_SHAPES = S1_SHAPES + STRIDED_SHAPES
# tiny output images (OH * OW < 32 + OW): the weight gradient's general row walk
TINY_SHAPES = [(5, 128, 5, 5, 128, (3, 3), 1, (0, 0)), (3, 128, 12, 9, 160, (3, 3), 2, (1, 1))]
VARIANTS = list(range(32))
# 9 (halo) and 10 (direct) are 3x3 stride-1 conv kernels with contracts of their own: no GEMM form, no
# strided backward-data, no accumulating store (ops/conv.py hands an accum= to the built-in NT tile then)
OWN_CONTRACT = (9, 10)
NT_VARIANTS = [v for v in VARIANTS if v not in OWN_CONTRACT]


def _sid(s):
    return f"{s[0]}x{s[1]}x{s[2]}x{s[3]}-{s[4]}k{s[5][0]}{s[5][1]}s{s[6]}p{s[7][0]}{s[7][1]}"


def _rows_of(shape):
    n, _, h, w, _, (r, s), st, (ph, pw) = shape
    return n * ((h + 2 * ph - r) // st + 1) * ((w + 2 * pw - s) // st + 1)


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ints(gen, shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def _ref(shape, amp=2):
    """The integer operands of ``shape`` and the float64 reference of all three passes (CPU), with the
    preconditions that make a correct kernel's result exact asserted on the reference."""
    n, ci, h, w, co, (r, s), st, pad = shape
    gen = torch.Generator().manual_seed(1000 * ci + 10 * co + h + amp)
    x, wt = _ints(gen, (n, ci, h, w), amp), _ints(gen, (co, ci, r, s), amp)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, st, pad)
    dy = _ints(gen, tuple(y.shape), amp)
    g = _ints(gen, (n, ci, h, w), amp)
    pre = _ints(gen, (co, ci, r, s), amp)  # what a weight-gradient slot holds before dW is added
    y.backward(dy)
    y = y.detach()
    xa, wa = x.abs().requires_grad_(True), wt.abs().requires_grad_(True)
    ya = F.conv2d(xa, wa, None, st, pad)
    ya.backward(dy.abs())
    assert ya.max().item() < _EXACT, "sum |x w| per output"
    assert y.abs().sum((0, 2, 3)).max().item() < _EXACT and (y * y).sum((0, 2, 3)).max().item() < _EXACT
    assert xa.grad.max().item() < _EXACT, "sum |dy w| per dX element"
    assert wa.grad.max().item() < _EXACT, "sum |dy x| per dW element"
    return types.SimpleNamespace(x=x, w=wt, dy=dy, g=g, pre=pre, y=y, dx=xr.grad, dw=wr.grad, amp=amp)


@functools.lru_cache(maxsize=None)
def _gpu(shape, amp=2):
    """Operands (bf16 channels_last) and expected results of ``shape`` on the GPU; shared, never written."""
    r = _ref(shape, amp)
    dev = torch.device("cuda", 0)

    def op(t):
        return _nhwc(t.to(dev)).to(_BF16)

    co = shape[4]
    return types.SimpleNamespace(
        x=op(r.x), w=op(r.w), dy=op(r.dy), g=op(r.g),
        y=op(r.y), ysum=r.y.sum((0, 2, 3)).float().to(dev), ysq=(r.y * r.y).sum((0, 2, 3)).float().to(dev),
        y32=_nhwc(r.y.float().to(dev)), dx=op(r.dx), dx_acc=op(r.g + r.dx), dx32=_nhwc(r.dx.float().to(dev)),
        dw=_nhwc(r.dw.float().to(dev)), pre=_nhwc(r.pre.float().to(dev)), dw_acc=_nhwc((r.pre + r.dw).float().to(dev)),
        dw_absmax=(r.dw.abs().max().item() + r.amp), co=co)


def _krsc_flat(t):
    """[Co, Ci, R, S] -> flat [Co][R][S][Ci] (the memory order of a weight-gradient slot)."""
    return t.permute(0, 2, 3, 1).contiguous().reshape(-1)


_DECLINED = object()


def _call(fn):
    """``fn()``, or _DECLINED when the launcher refused the (variant, shape) by its contract (status -3)."""
    from tony_amd.ops import _lib

    try:
        return fn()
    except _lib.KernelError as e:
        if str(e).endswith("code -3"):
            return _DECLINED
        raise


# (pass, variant) -> shapes that ran (were not declined); every (pass, variant, shape) tried this session
_RAN: dict = {}
_TRIED: set = set()


def _ran(pas, v, shape):
    _RAN.setdefault((pas, v), set()).add(shape)


# --------------------------------------------------------------------------- A: pinned variants --
def _fwd_case(shape, v, record=True):
    from tony_amd.ops import _lib
    from tony_amd.ops.conv import conv_fwd

    c = _gpu(shape)
    st, pad, co = shape[6], shape[7], shape[4]
    if record:
        _TRIED.add(("fwd", v, shape))
    stats = torch.zeros(_lib.stat_floats(co), device=c.x.device)
    y = _call(lambda: conv_fwd(c.x, c.w, st, pad, stats, vflags=v << 8))
    if y is _DECLINED:
        return False
    assert y.is_contiguous(memory_format=torch.channels_last)
    _assert_equal(y, c.y, f"fwd v={v} y (n, c, oy, ox)")
    folded = _lib.fold_stats(stats, co)
    _assert_equal(folded[:co], c.ysum, f"fwd v={v} sum(y) per channel")
    _assert_equal(folded[co:], c.ysq, f"fwd v={v} sum(y^2) per channel")
    if record:
        _ran("fwd", v, shape)
    return True


def _dgrad_case(shape, v, record=True, amp=2):
    from tony_amd.ops import _lib
    from tony_amd.ops.conv import conv_dgrad

    c = _gpu(shape, amp)
    st, pad = shape[6], shape[7]
    xs = tuple(c.x.shape)
    if record:
        _TRIED.add(("dgrad", v, shape))
    L = _lib.lib()
    prev = L.tony_dgrad_one_launch(-1)
    try:
        for k, one in enumerate((1, 0) if st > 1 else (prev,)):
            L.tony_dgrad_one_launch(one)
            dx = _call(lambda: conv_dgrad(c.dy, c.w, xs, st, pad, vflags=v << 8))
            if dx is _DECLINED:
                # the first launch decides: a decline that depends on the one-launch setting is a failure
                assert k == 0, f"dgrad v={v}: declined with one_launch={one} after it ran with the other setting"
                return False
            _assert_equal(dx, c.dx, f"dgrad v={v} one_launch={one} dX (n, c, y, x)")
            # (9, 10 and 40 have no accumulating store: conv_dgrad hands the add to the built-in NT tile)
            g = c.g.clone()
            out = _call(lambda: conv_dgrad(c.dy, c.w, xs, st, pad, vflags=v << 8, accum=g))
            assert out is not _DECLINED, "accum= declined a shape the plain call takes"
            assert out.data_ptr() == g.data_ptr()
            _assert_equal(out, c.dx_acc, f"dgrad v={v} one_launch={one} bf16(g + dX) (n, c, y, x)")
    finally:
        L.tony_dgrad_one_launch(prev)
    if record:
        _ran("dgrad", v, shape)
    return True


@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_conv_fwd_exact(cuda, shape, v):
    """conv_fwd at a pinned tile variant: y bit-equal to bf16(float64 conv), statistics the exact sums."""
    if not _fwd_case(shape, v):
        pytest.skip("the launcher declines this (variant, shape): status -3")


@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_conv_dgrad_exact(cuda, shape, v):
    """conv_dgrad at a pinned tile variant, stride 1 and strided (both settings of the one-launch form),
    plain and accumulating: dX = bf16(float64 dX), accum = bf16(g + dX) with ONE rounding."""
    if not _dgrad_case(shape, v):
        pytest.skip("the launcher declines this (variant, shape): status -3")


# the halo (9), direct (10) and band (40) variants inside their documented contracts
SPECIAL = [(9, (1, 64, 9, 9, 32, (3, 3), 1, (0, 0))), (9, (2, 32, 19, 21, 64, (3, 3), 1, (1, 1))),
           (9, (3, 32, 24, 16, 64, (3, 3), 1, (1, 1))),
           (10, (3, 32, 37, 45, 32, (3, 3), 1, (0, 0))), (10, (2, 64, 24, 20, 64, (3, 3), 1, (1, 1))),
           (10, (2, 64, 29, 35, 32, (3, 3), 1, (1, 1))),
           (40, (2, 64, 9, 20, 96, (1, 7), 1, (0, 3))), (40, (2, 192, 11, 13, 128, (3, 1), 1, (1, 0))),
           (40, (3, 96, 17, 17, 64, (1, 7), 1, (0, 0)))]


@pytest.mark.parametrize("v,shape", SPECIAL, ids=[f"v{v}-{_sid(s)}" for v, s in SPECIAL])
def test_conv_exact_halo_direct_band(cuda, v, shape):
    """Forward + statistics, and the backward-data (plain and accum=) where the kernel has one for the shape
    (halo: Cout of 32 / 64, it runs with Cin' = Cout; band: "same" padding), as the variants' own tests
    select them."""
    _, _, _, _, co, (r, s), _, (ph, pw) = shape
    rec = v in OWN_CONTRACT  # (40 is no variant of the 0-31 matrix)
    assert _fwd_case(shape, v, record=rec), "a shape inside the variant's contract was declined"
    if (v == 9 and co in (32, 64)) or v == 10 or (v == 40 and (2 * ph + 1, 2 * pw + 1) == (r, s)):
        assert _dgrad_case(shape, v, record=rec), "a shape inside the variant's contract was declined"


# With {-2..2} the dX of these kernels' shapes stays below 256, where bf16 holds every integer and one or two
# roundings cannot differ.  Wider integers (still exact: the preconditions of _ref hold) push |dX| past 256,
# where rounding dX to bf16 before adding g lands one ulp off at ties.
ACCUM_TIES = [(9, (1, 64, 9, 9, 32, (3, 3), 1, (0, 0)), 4), (10, (1, 64, 9, 9, 64, (3, 3), 1, (1, 1)), 4),
              (40, (2, 64, 9, 20, 96, (1, 7), 1, (0, 3)), 3)]


@pytest.mark.parametrize("v,shape,amp", ACCUM_TIES, ids=[f"v{v}-{_sid(s)}" for v, s, _ in ACCUM_TIES])
def test_conv_dgrad_accum_rounds_once_whatever_the_variant(cuda, v, shape, amp):
    """conv_dgrad(accum=g) pinned to the halo / direct / band kernel, which has no accumulating store: the
    result is still bf16(g + dX) with one rounding, on operands where two roundings give another result."""
    r = _ref(shape, amp)
    twice = (r.dx.to(_BF16).double() + r.g).to(_BF16)
    assert not torch.equal(twice, (r.dx + r.g).to(_BF16)), "these operands cannot tell one rounding from two"
    assert _dgrad_case(shape, v, record=False, amp=amp), "a shape inside the variant's contract was declined"


def _wgrad_impls(shape):
    from tony_amd.ops import gemm
    from tony_amd.ops.conv import wgrad_direct_supported

    _, ci, _, _, co, (r, s), st, _ = shape
    impls = []
    for occ in (*gemm.WGRAD_OCC, *gemm.WGRAD_OCC_BIG, 1):
        if occ not in impls:
            impls.append(occ)
    if wgrad_direct_supported(ci, co, r, s, st, st):
        impls.append("direct")
    return impls


@pytest.mark.parametrize("shape", ALL_SHAPES + TINY_SHAPES, ids=_sid)
def test_conv_wgrad_exact(cuda, shape):
    """conv_wgrad at every shipped split plan (gemm.WGRAD_OCC, WGRAD_OCC_BIG, 1, and "direct" where it is
    supported), both settings of the fragment prefetch: returned fp32, added into an fp32 slot and into a
    bf16 slot, all exact."""
    from tony_amd.ops import _lib
    from tony_amd.ops.conv import conv_wgrad

    amp = 2 if _gpu(shape).dw_absmax <= 256 else 1  # a bf16 slot that is added into stays exact up to 256
    c = _gpu(shape, amp)
    assert c.dw_absmax <= 256, "every value of the bf16 slot must be an integer of magnitude <= 256"
    st, pad, ws = shape[6], shape[7], tuple(c.w.shape)
    L = _lib.lib()
    prev = L.tony_wgrad_pf(-1)
    try:
        for impl in _wgrad_impls(shape):
            for pf in (0, 1):
                L.tony_wgrad_pf(pf)
                dw = conv_wgrad(c.dy, c.x, ws, st, pad, impl=impl)
                assert dw.dtype == torch.float32
                _assert_equal(dw, c.dw, f"wgrad impl={impl} pf={pf} dW (co, ci, r, s)")
                for dt in (torch.float32, _BF16):
                    slot = _krsc_flat(c.pre).to(dt, copy=True)
                    assert conv_wgrad(c.dy, c.x, ws, st, pad, dst=slot, impl=impl) is None
                    _assert_equal(slot, _krsc_flat(c.dw_acc).to(dt),
                                  f"wgrad impl={impl} pf={pf} {dt} slot [co][r][s][ci]")
    finally:
        L.tony_wgrad_pf(prev)


# (the fourth: K a multiple of 64 with a partial row tile, which the 64-deep interleaved variant 22 needs)
GEMM_MNK = [(286, 88, 360), (49, 64, 576), (210, 224, 672), (150, 96, 320)]


@functools.lru_cache(maxsize=None)
def _gemm_ref(mnk):
    m, n, k = mnk
    gen = torch.Generator().manual_seed(m + n + k)
    a, b = _ints(gen, (m, k), 2), _ints(gen, (n, k), 2)
    c = a @ b.t()
    assert (a.abs() @ b.abs().t()).max().item() < _EXACT
    assert c.abs().sum(0).max().item() < _EXACT and (c * c).sum(0).max().item() < _EXACT
    dev = torch.device("cuda", 0)
    return types.SimpleNamespace(a=a.to(dev).to(_BF16), b=b.to(dev).to(_BF16), c=c.to(dev).to(_BF16),
                                 csum=c.sum(0).float().to(dev), csq=(c * c).sum(0).float().to(dev))


def _gemm_case(mnk, v):
    from tony_amd.ops.gemm import gemm_nt

    r = _gemm_ref(mnk)
    n = mnk[1]
    stats = torch.empty(2 * n, device=r.a.device)
    _TRIED.add(("gemm", v, mnk))
    c = _call(lambda: gemm_nt(r.a, r.b, stats=stats, vflags=v << 8))
    if c is _DECLINED:
        return False
    _assert_equal(c, r.c, f"gemm_nt v={v} C (row, col)")
    _assert_equal(stats[:n], r.csum, f"gemm_nt v={v} column sums")
    _assert_equal(stats[n:], r.csq, f"gemm_nt v={v} column sums of squares")
    _ran("gemm", v, mnk)
    return True


@pytest.mark.parametrize("v", NT_VARIANTS)
@pytest.mark.parametrize("mnk", GEMM_MNK, ids=lambda t: "x".join(map(str, t)))
def test_gemm_nt_exact(cuda, mnk, v):
    if not _gemm_case(mnk, v):
        pytest.skip("the launcher declines this (variant, shape): status -3")


@pytest.mark.parametrize("mn", [(286, 40, 88), (37, 8, 16)], ids=lambda t: "x".join(map(str, t)))
def test_gemm_tn_exact(cuda, mn):
    from tony_amd.ops.gemm import gemm_tn

    m, n1, n2 = mn
    gen = torch.Generator().manual_seed(m)
    a, b = _ints(gen, (m, n1), 2), _ints(gen, (m, n2), 2)
    got = gemm_tn(a.to(cuda).to(_BF16), b.to(cuda).to(_BF16))
    _assert_equal(got, (a.t() @ b).float().to(cuda), "gemm_tn A^T B (n1, n2)")


@pytest.mark.parametrize("co", [32, 64])
@pytest.mark.parametrize("pad", [(0, 0), (1, 1)], ids=["p0", "p1"])
def test_stem_exact(cuda, pad, co):
    """csrc/stem.hip on a 3-channel 19 x 17 image, 3x3 stride 2: forward + statistics and the weight
    gradient (returned, and added into fp32 / bf16 slots), all exact."""
    from tony_amd.ops import _lib
    from tony_amd.ops.conv import stem_fwd, stem_supported, stem_wgrad

    shape = (2, 3, 19, 17, co, (3, 3), 2, pad)
    c = _gpu(shape)
    assert c.dw_absmax <= 256
    assert stem_supported(c.x, c.w, 2, pad)
    stats = torch.zeros(_lib.stat_floats(co), device=cuda)
    y = stem_fwd(c.x, c.w, 2, pad, stats)
    _assert_equal(y, c.y, "stem y (n, c, oy, ox)")
    folded = _lib.fold_stats(stats, co)
    _assert_equal(folded[:co], c.ysum, "stem sum(y)")
    _assert_equal(folded[co:], c.ysq, "stem sum(y^2)")
    dw = stem_wgrad(c.dy, c.x, tuple(c.w.shape), 2, pad)
    _assert_equal(dw, c.dw, "stem dW (co, ci, r, s)")
    for dt in (torch.float32, _BF16):
        slot = _krsc_flat(c.pre).to(dt, copy=True)
        assert stem_wgrad(c.dy, c.x, tuple(c.w.shape), 2, pad, dst=slot) is None
        _assert_equal(slot, _krsc_flat(c.dw_acc).to(dt), f"stem {dt} slot [co][r][s][ci]")


X3_SHAPES = [S1_SHAPES[0], S1_SHAPES[1], STRIDED_SHAPES[0]]


@pytest.mark.parametrize("code", [0, 2, 12, 16, 32, 33, 34, 35, 36, 37])
@pytest.mark.parametrize("shape", X3_SHAPES, ids=_sid)
def test_x3_exact(cuda, shape, code, monkeypatch):
    """The fp32 path (ops/x3.py): integer operands have zero lo planes, so the fp32 forward (+ statistics),
    backward-data (plain and accumulating) and weight gradient equal the float64 reference exactly -- on
    pinned plain tiles and on the fused-plane tile codes 32-37."""
    from tony_amd.ops import _lib, tune, x3

    n, ci, h, w, co, k, st, pad = shape
    if code >= 32:
        kb = 64 if code == 35 else 32  # the fused tile's K-step: the plane width must be a multiple of it
        if ci % kb or (st == 1 and co % kb):
            pytest.skip(f"code {code}: {kb}-deep K-steps need plane widths that are multiples of {kb}")
    c = _gpu(shape)
    xf, wf, dyf = c.x.float(), c.w.float(), c.dy.float()
    xp, cp = x3.split_act(xf)
    dp, _ = x3.split_act(dyf)

    def pick(key, launch, variants=None):
        rc = launch(code << 8)
        assert rc == 0, f"code {code} refused for {key[0]}: status {rc}"  # (the pre-check above took the shape)
        return code << 8

    monkeypatch.setattr(tune, "_CACHE", {})
    monkeypatch.setattr(tune, "pick", pick)
    stats = torch.zeros(_lib.stat_floats(co), device=cuda)
    z = x3.conv_fwd(xp, cp, x3.split_weight(wf), tuple(wf.shape), st, pad, stats)
    _assert_equal(z, c.y32, f"x3 fwd code={code} (n, c, oy, ox)")
    folded = _lib.fold_stats(stats, co)
    _assert_equal(folded[:co], c.ysum, f"x3 fwd code={code} sum(y)")
    _assert_equal(folded[co:], c.ysq, f"x3 fwd code={code} sum(y^2)")
    if st == 1 or code < 32:  # (the strided dgrad has no fused-plane form)
        wt3 = x3.split_weight_t(wf)
        dx = x3.conv_dgrad(dp, wt3, co, tuple(xf.shape), tuple(wf.shape), st, pad)
        _assert_equal(dx, c.dx32, f"x3 dgrad code={code} (n, c, y, x)")
        acc = c.g.float()
        out = x3.conv_dgrad(dp, wt3, co, tuple(xf.shape), tuple(wf.shape), st, pad, accum=acc)
        _assert_equal(out, c.g.float() + c.dx32, f"x3 dgrad code={code} accumulating (n, c, y, x)")
    if code == 0:  # the weight gradient has no tile codes: once per shape
        dw = x3.conv_wgrad(dp, xp, cp, tuple(wf.shape), st, pad)
        _assert_equal(dw, c.dw, "x3 wgrad (co, ci, r, s)")


# --------------------------------------------------- B: poisoned operands, guarded destinations --
def _stats_slab(co, device):
    from tony_amd.ops import _lib

    s = _Slab(1, _lib.stat_floats(co), 0, torch.float32, _SENT, device, guard_ld=2 * co)
    s.view.zero_()  # accumulated into: zero on entry
    return s


B_SHAPES = [S1_SHAPES[0], S1_SHAPES[1], S1_SHAPES[2], STRIDED_SHAPES[0]]


def _geom(shape):
    n, ci, h, w, co, (r, s), st, (ph, pw) = shape
    return n, ci, h, w, co, r, s, st, ph, pw, (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1


@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("shape", B_SHAPES, ids=_sid)
def test_conv_fwd_poisoned_surroundings(cuda, shape, v):
    """tony_conv_fwd on an x that is a channel slice of a NaN buffer, a w between NaN guards, into a y that
    is a channel slice of a sentinel buffer, statistics between sentinel guards."""
    from tony_amd.ops import _lib

    c = _gpu(shape)
    n, ci, h, w, co, r, s, st, ph, pw, oh, ow = _geom(shape)
    X = _poisoned(_pix_rows(c.x), 16)
    W = _poisoned(c.w.permute(0, 2, 3, 1).reshape(co, -1), 0)
    Y = _Slab(n * oh * ow, co, 8, _BF16, _SENT, cuda)
    ST = _stats_slab(co, cuda)
    rc = _lib.lib().tony_conv_fwd(X.ptr(), n, h, w, ci, X.ld, W.ptr(), co, r, s, st, st, ph, pw, Y.ptr(), oh, ow,
                                  Y.ld, 1 | (v << 8), ST.ptr(), 2 * co, _lib.stream_ptr(cuda))
    if rc == -3:
        pytest.skip("the launcher declines this (variant, shape): status -3")
    assert rc == 0, f"tony_conv_fwd status {rc}"
    torch.cuda.synchronize()
    y, stats = Y.view, _lib.fold_stats(ST.view.reshape(-1), co)
    assert not torch.isnan(y.float()).any() and not torch.isnan(ST.view).any(), "a NaN outside the operands was read"
    _assert_equal(y.contiguous(), _pix_rows(c.y).contiguous(), f"fwd v={v} y (pixel row, channel)")
    _assert_equal(stats[:co], c.ysum, f"fwd v={v} sum(y)")
    _assert_equal(stats[co:], c.ysq, f"fwd v={v} sum(y^2)")
    Y.assert_surroundings_intact("y")
    ST.assert_surroundings_intact("statistics")


_B_DGRAD = [(s, v) for s in B_SHAPES for v in (VARIANTS if s[6] == 1 else NT_VARIANTS)]


@pytest.mark.parametrize("shape,v", _B_DGRAD, ids=[f"{_sid(s)}-{v}" for s, v in _B_DGRAD])
def test_conv_dgrad_poisoned_surroundings(cuda, shape, v):
    """tony_conv_dgrad / tony_conv_dgrad_strided on a dy slice of a NaN buffer and a transposed filter
    between NaN guards, into a dX slice of a sentinel buffer."""
    from tony_amd.ops import _lib

    c = _gpu(shape)
    n, ci, h, w, co, r, s, st, ph, pw, oh, ow = _geom(shape)
    DY = _poisoned(_pix_rows(c.dy), 16)
    WT = _poisoned(c.w.permute(1, 2, 3, 0).reshape(ci, -1), 0)  # [C][R][S][Co]
    DX = _Slab(n * h * w, ci, 8, _BF16, _SENT, cuda)
    L, stream = _lib.lib(), _lib.stream_ptr(cuda)
    if st == 1:
        rc = L.tony_conv_dgrad(DY.ptr(), n, oh, ow, co, DY.ld, WT.ptr(), ci, r, s, ph, pw, DX.ptr(), h, w, DX.ld,
                               v << 8, None, stream)
    else:
        rc = L.tony_conv_dgrad_strided(DY.ptr(), n, oh, ow, co, DY.ld, WT.ptr(), ci, r, s, st, st, ph, pw, DX.ptr(),
                                       h, w, DX.ld, v << 8, None, stream)
    if rc == -3:
        pytest.skip("the launcher declines this (variant, shape): status -3")
    assert rc == 0, f"dgrad status {rc}"
    torch.cuda.synchronize()
    assert not torch.isnan(DX.view.float()).any(), "a NaN outside the operands was read"
    _assert_equal(DX.view.contiguous(), _pix_rows(c.dx).contiguous(), f"dgrad v={v} dX (pixel row, channel)")
    DX.assert_surroundings_intact("dX")


@pytest.mark.parametrize("shape", B_SHAPES, ids=_sid)
def test_conv_wgrad_poisoned_surroundings(cuda, shape):
    """tony_conv_wgrad (through splitk_combine, the default plans) on x / dy slices of NaN buffers, dW added
    into a sub-range of a sentinel buffer."""
    from tony_amd.ops import _lib
    from tony_amd.ops.gemm import occ_choices, splitk_combine, wgrad_cus

    c = _gpu(shape)
    n, ci, h, w, co, r, s, st, ph, pw, oh, ow = _geom(shape)
    X = _poisoned(_pix_rows(c.x), 16)
    DY = _poisoned(_pix_rows(c.dy), 8)
    L = _lib.lib()
    tbm = 32 if co <= 32 else 64 if co <= 64 else 128
    ntiles = -(-co // tbm) * -(-(r * s * ci) // 128)
    nel = co * r * s * ci
    for occ in occ_choices(n * oh * ow):
        DW = _Slab(1, nel, 0, torch.float32, _SENT, cuda, guard_ld=r * s * ci)  # a dW row: [r][s][ci] of one co
        out = splitk_combine(
            lambda slab, cap, sp, fc, fd, ff: L.tony_conv_wgrad(
                DY.ptr(), DY.ld, X.ptr(), n, h, w, ci, X.ld, co, r, s, st, st, ph, pw, oh, ow, 0, slab, cap, sp,
                wgrad_cus(cuda, occ), fc, fd, ff, _lib.stream_ptr(cuda)),
            nel, ntiles, cuda, DW.view.reshape(-1), occ)
        assert out is None
        torch.cuda.synchronize()
        got = DW.view.reshape(-1)
        assert not torch.isnan(got).any(), "a NaN outside the operands was read"
        _assert_equal(got, _krsc_flat(c.dw) + _SENT, f"wgrad occ={occ} sentinel + dW [co][r][s][ci]")
        DW.assert_surroundings_intact("dW")


@pytest.mark.parametrize("v", NT_VARIANTS)
@pytest.mark.parametrize("mnk", GEMM_MNK, ids=lambda t: "x".join(map(str, t)))
def test_gemm_poisoned_surroundings(cuda, mnk, v):
    """tony_gemm_bf16 on an A that is a column slice of a NaN buffer, B between NaN guards, C a column
    slice of a sentinel buffer, statistics between sentinel guards."""
    from tony_amd.ops import _lib

    r = _gemm_ref(mnk)
    m, n, k = mnk
    A, B = _poisoned(r.a, 16), _poisoned(r.b, 0)
    C = _Slab(m, n, 8, _BF16, _SENT, cuda)
    ST = _stats_slab(n, cuda)
    rc = _lib.lib().tony_gemm_bf16(A.ptr(), B.ptr(), C.ptr(), m, n, k, A.ld, B.ld, C.ld, 1 | (v << 8), ST.ptr(), 2 * n,
                                   _lib.stream_ptr(cuda))
    if rc == -3:
        pytest.skip("the launcher declines this (variant, shape): status -3")
    assert rc == 0, f"tony_gemm_bf16 status {rc}"
    torch.cuda.synchronize()
    assert not torch.isnan(C.view.float()).any(), "a NaN outside the operands was read"
    assert not torch.isnan(ST.view).any(), "a NaN outside the operands reached the statistics"
    _assert_equal(C.view.contiguous(), r.c, f"gemm v={v} C (row, col)")
    stats = _lib.fold_stats(ST.view.reshape(-1), n)
    _assert_equal(stats[:n], r.csum, f"gemm v={v} column sums")
    _assert_equal(stats[n:], r.csq, f"gemm v={v} column sums of squares")
    C.assert_surroundings_intact("C")
    ST.assert_surroundings_intact("statistics")


# ------------------------------------------------------ C: slice producers and consumers --
_WIDTHS = (32, 40, 24)


def _concat3(like, h=9, w=7):
    from tony_amd.ops import concat

    buf = concat.concat_buffer(2, sum(_WIDTHS), h, w, like)
    buf.fill_(_SENT)
    return buf


def _assert_neighbours(buf, what):
    lo, hi = buf[:, :_WIDTHS[0]], buf[:, _WIDTHS[0] + _WIDTHS[1]:]
    assert torch.equal(lo, torch.full_like(lo, _SENT)) and torch.equal(hi, torch.full_like(hi, _SENT)), \
        f"{what}: a neighbour slice of the concat buffer changed"


@pytest.mark.parametrize("relu", [True, False])
def test_conv_bn_act_training_slot_keeps_neighbours(cuda, relu):
    """conv_bn_act(training, slot=) writes the middle slice of a three-slice concat buffer: bit-equal to the
    unslotted call (integer inputs: exact statistics), the neighbour slices untouched."""
    from tony_amd.ops import concat
    from tony_amd.ops.conv import conv_bn_act

    shape = (2, 32, 9, 7, _WIDTHS[1], (3, 3), 1, (1, 1))
    c = _gpu(shape)
    co = _WIDTHS[1]
    gen = torch.Generator().manual_seed(3)
    gamma = (torch.rand(co, generator=gen) + 0.5).to(cuda)
    beta = (torch.randn(co, generator=gen) * 0.1).to(cuda)

    def run(slot):
        rm, rv = torch.zeros(co, device=cuda), torch.ones(co, device=cuda)
        with torch.no_grad():
            y = conv_bn_act(c.x, c.w, gamma, beta, rm, rv, 1, 1, True, 0.1, 1e-3, relu, slot=slot)
        return y, rm, rv

    plain, rm0, rv0 = run(None)
    buf = _concat3(c.x)
    y, rm1, rv1 = run(concat.Slot(buf, _WIDTHS[0]))
    torch.cuda.synchronize()
    mid = buf[:, _WIDTHS[0]:_WIDTHS[0] + co]
    assert y.data_ptr() == mid.data_ptr(), "the slot was not written in place"
    assert torch.isfinite(plain.float()).all()
    _assert_equal(mid, plain, "slotted vs unslotted conv_bn_act (n, c, y, x)")
    _assert_equal(rm1, rm0, "running mean")
    _assert_equal(rv1, rv0, "running var")
    _assert_neighbours(buf, "conv_bn_act slot")


def test_max_pool_slot_keeps_neighbours(cuda):
    from tony_amd.ops import concat
    from tony_amd.ops.pool import max_pool

    gen = torch.Generator().manual_seed(4)
    x = _nhwc(_ints(gen, (2, _WIDTHS[1], 19, 15), 2).to(cuda)).to(_BF16)
    plain = max_pool(x, 3, 2)
    buf = _concat3(x)
    y = max_pool(x, 3, 2, slot=concat.Slot(buf, _WIDTHS[0]))
    torch.cuda.synchronize()
    mid = buf[:, _WIDTHS[0]:_WIDTHS[0] + _WIDTHS[1]]
    assert y.data_ptr() == mid.data_ptr(), "the slot was not written in place"
    _assert_equal(plain, _nhwc(F.max_pool2d(x.float(), 3, 2)).to(_BF16), "max_pool vs reference")
    _assert_equal(mid, plain, "slotted vs unslotted max_pool (n, c, y, x)")
    _assert_neighbours(buf, "max_pool slot")


def _close(a, b, rtol, atol, what, max_bad_frac=0.0):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    assert bad <= max_bad_frac * a.numel(), f"{what}: {bad}/{a.numel()} outside tol, max err {err.max().item():.4g}"


@pytest.mark.parametrize("relu", [True, False])
def test_bn_act_backward_on_slices_of_nan_buffers(cuda, relu):
    """bn_act forward + backward with x and dy the middle channel slices of wider buffers whose other
    channels are NaN: dx / dgamma / dbeta against float64 at test_bn_act_train_fwd_bwd's tolerances, no NaN."""
    from tony_amd.ops.bn import bn_act

    c0, c = _WIDTHS[0], _WIDTHS[1]
    gen = torch.Generator().manual_seed(5)
    shape = (2, c, 9, 7)
    xs = (torch.randn(shape, generator=gen) * 2 + 0.5).to(_BF16)
    dys = torch.randn(shape, generator=gen).to(_BF16)
    gamma = (torch.rand(c, generator=gen) + 0.5).to(_BF16)
    beta = (torch.randn(c, generator=gen) * 0.1).to(_BF16)

    def wide(t):
        big = _nhwc(torch.full((2, sum(_WIDTHS), 9, 7), float("nan"), dtype=_BF16, device=cuda))
        big[:, c0:c0 + c] = t.to(cuda)
        return big[:, c0:c0 + c]

    xr, gr, br = (t.double().requires_grad_(True) for t in (xs, gamma, beta))
    yr = F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-3)
    yr = torch.relu(yr) if relu else yr
    yr.backward(dys.double())
    xk = wide(xs).detach().requires_grad_(True)
    gk, bk = gamma.to(cuda).requires_grad_(True), beta.to(cuda).requires_grad_(True)
    rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
    yk = bn_act(xk, gk, bk, rm, rv, True, 0.1, 1e-3, relu)
    yk.backward(wide(dys))
    torch.cuda.synchronize()
    for t, what in ((yk, "y"), (xk.grad, "dx"), (gk.grad, "dgamma"), (bk.grad, "dbeta"), (rm, "running mean")):
        assert torch.isfinite(t.float()).all(), f"{what}: a NaN of a neighbour channel was read"
    _close(yk, yr.detach(), 2e-2, 2e-2, "bn fwd")
    _close(xk.grad, xr.grad, 3e-2, 3e-2, "bn dx", max_bad_frac=1e-3)
    _close(gk.grad, gr.grad, 3e-2, 0.05 * gr.grad.abs().max().item() + 1e-2, "bn dgamma")
    _close(bk.grad, br.grad, 3e-2, 0.05 * br.grad.abs().max().item() + 1e-2, "bn dbeta")


@pytest.mark.parametrize("k,pad", [((3, 3), (1, 1)), ((1, 1), (0, 0))], ids=["3x3", "1x1"])
def test_conv_bn_act_infer_slot_keeps_neighbours(cuda, k, pad):
    """conv_bn_act_infer(slot=): the conv and the 1x1 GEMM epilogues write only their channel slice."""
    from tony_amd.ops import concat
    from tony_amd.ops.conv import conv_bn_act_infer

    shape = (2, 32, 9, 7, _WIDTHS[1], k, 1, pad)
    c = _gpu(shape)
    co = _WIDTHS[1]
    gen = torch.Generator().manual_seed(6)
    g, b = (torch.rand(co, generator=gen) + 0.5).to(cuda), (torch.randn(co, generator=gen) * 0.1).to(cuda)
    rm, rv = (torch.randn(co, generator=gen) * 0.1).to(cuda), (torch.rand(co, generator=gen) + 0.5).to(cuda)
    with torch.no_grad():
        plain = conv_bn_act_infer(c.x, c.w, g, b, rm, rv, 1, pad, 1e-3, True)
        buf = _concat3(c.x)
        conv_bn_act_infer(c.x, c.w, g, b, rm, rv, 1, pad, 1e-3, True, slot=concat.Slot(buf, _WIDTHS[0]))
    torch.cuda.synchronize()
    _assert_equal(buf[:, _WIDTHS[0]:_WIDTHS[0] + co], plain, "slotted vs unslotted conv_bn_act_infer (n, c, y, x)")
    _assert_neighbours(buf, "conv_bn_act_infer slot")


# ------------------------------------------------------------------- coverage of the matrix --
def test_zz_every_variant_ran(cuda):
    """Every variant 0-31 ran (was not declined) on at least two stride-1 shapes per pass, one of them with
    a partial row tile (M % 64 != 0: partial for the 64-, 128- and 256-row tiles alike), and on at least
    one strided shape -- so a silent decline cannot empty the matrix.  The halo and direct kernels (9, 10)
    are stride-1 only by contract and have tiles of their own: at least two stride-1 shapes per pass, which
    the shapes of SPECIAL supply (all with partial edge tiles).  Cases this session has not tried yet (a
    filtered run) are run here first."""
    for v in VARIANTS:
        for shape in ALL_SHAPES + [s for sv, s in SPECIAL if sv == v]:
            if ("fwd", v, shape) not in _TRIED:
                _fwd_case(shape, v)
            if ("dgrad", v, shape) not in _TRIED:
                _dgrad_case(shape, v)
    for v in NT_VARIANTS:
        for mnk in GEMM_MNK:
            if ("gemm", v, mnk) not in _TRIED:
                _gemm_case(mnk, v)
    short = []
    for v in NT_VARIANTS:  # gemm_nt: two shapes, one of them with a partial row tile
        ran = _RAN.get(("gemm", v), set())
        if len(ran) < 2 or not any(m[0] % 64 for m in ran):
            short.append(("gemm", v, sorted(ran)))
    for pas in ("fwd", "dgrad"):
        for v in VARIANTS:
            ran = _RAN.get((pas, v), set())
            s1 = [s for s in ran if s[6] == 1]
            if v in OWN_CONTRACT:
                ok = len(s1) >= 2
            else:
                ok = len(s1) >= 2 and any(_rows_of(s) % 64 for s in s1) and any(s[6] > 1 for s in ran)
            if not ok:
                short.append((pas, v, sorted(_sid(s) for s in ran)))
    assert not short, f"variants short of coverage (pass, variant, shapes that ran): {short}"
