"""Exact tests of the split-K combine (csrc/splitk.hip), the batched weight transpose (csrc/transpose.hip through
ops/wt_cache.TransposedWeights) and the MFMA linear layer (ops/linear.py).  Everything here is ``torch.equal``:
the operands leave a correct kernel no freedom.

Split-K combine (``tony_splitk_reduce``).  Slab entries are integers in [-8, 8], the pre-fill of an accumulating
destination integers in [-64, 64]: every partial sum, in any group / chunk / pass order, is an exact fp32
integer (|sum| <= 512 * 8 + 64 < 2^24, asserted on the reference), so dst must equal the float64 sum (+ the
pre-fill) rounded ONCE to the destination dtype.  The (512, 5120) bf16 case holds sums above 256 that really
round (asserted).  ``_plan`` mirrors the launcher: with fewer column blocks than CUs and >= 32 splits the first
pass sums chunks in place; at 256 CUs (3, 4), (4, 260), (31, 1024), (7, 65540) take one pass -- the last because
its 257 column blocks are no fewer than the CUs -- and (32, 1024), (33, 1028), (37, 9216), (100, 252),
(512, 5120) two; (100, 252) has a short last chunk (5 x 17 + 15) and n / 4 = 63 columns, (512, 5120) a short
last chunk of 12.  Both paths must have been taken at the device's CU count.  The slab sits between NaN guards,
dst in a sentinel slab; a one-pass case leaves the slab itself untouched.  n % 4 != 0, a misaligned dst and
splits = 0 are refused on the host and write nothing.
Mutants (test_cpu_splitk_*): one split row dropped, one doubled, the final row of the last chunk dropped: each
breaks equality in both dtypes at every case.  What the old tolerance (atol 1e-4 sqrt(splits) fp32, 1e-2
sqrt(splits) + rtol 1e-2 bf16, on randn) sees of a doubled row at (512, 5120): as a whole row it does notice
it (fp32: all but ~10 of 5120 elements exceed it), so the issue's expectation that the whole-row mutant stays
below it does not hold; but ~30 % of the elements of a bf16 destination stay inside it individually, so a row
doubled in a few columns only (one lane's float4, an edge column) passes it with that probability per element,
while equality on integers flags every element where the row is non-zero.  Asserted as measured.

Transpose (``tony_transpose_batch``).  One work list, every branch of the kernel:
    (32, 3, 3, 3)    the stem: Ci = 3, rows unaligned, the load falls back to scalars throughout
    (40, 24, 1, 1)   Co % 8 == 0, less than a tile; 16-byte loads and stores
    (64, 64, 1, 1)   exactly one full tile
    (72, 136, 3, 1)  partial tiles in both directions, several taps
    (200, 8, 1, 7)   four co tiles of one 8-wide ci column
    (12, 20, 1, 1)   Co % 8 != 0: the store falls back (rows of 24 bytes: every other row unaligned, and the
                     last 4 of 12 never fill a vector); Ci = 20: the load's last vector of a row falls back
    (16, 8, 1, 1)    Ci % 8 == 0 but the weight starts 8 bytes into its storage: unaligned rows, scalar loads
Every element of a weight has its own bf16 bit pattern (so a swapped pair shows; compared as bits), the
destinations are registered by hand inside sentinel slabs, and after ``refresh()`` on changed weights every
descriptor -- the first and the last: both ends of the binary search -- equals ``permute(1, 2, 3, 0)``.

Linear.  x, w in {-2..2}, bias in {-4..4}, dy in {-2..2}: y = x w^T + b (|y| <= 4 * 768 + 4), dx (<= 4000), dW and
db (<= 4 * 37) are exact fp32 integers, stored rounded once.  dW / db: returned, and summed into a bf16 slot
pre-filled with integers in [-64, 64] (|pre + dW| < 256: exact in bf16); dW also summed into an fp32 slot through
``wgrad_tn`` -- the layer itself only ever sees a slot of the parameter's dtype (``_lib.grad_slot``), so an fp32
slot of a bf16 Linear, and with it an fp32 db slot, does not exist.
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from exact_helpers import SENT, Slab, assert_equal

gpu = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

_CALLED = set()


def _L():
    from tony_amd.ops import _lib

    return _lib


def _k(name, *args, rc=0):
    lib = _L()
    if rc == 0:
        _CALLED.add(name)
    got = getattr(lib.lib(), name)(*args)
    assert got == rc, f"{name} returned {got}, expected {rc}"


# ------------------------------------------------------------------------------------- split-K combine --
SPLITK = [(3, 4), (4, 260), (31, 1024), (32, 1024), (33, 1028), (37, 9216), (100, 252), (512, 5120), (7, 65540)]


def _plan(splits, n, cus):
    """The launcher's decision (csrc/splitk.hip tony_splitk_reduce): (two passes?, chunk, chunks)."""
    grid = (n // 4 + 63) // 64
    if grid < cus and splits >= 32:
        want = min((2 * cus + grid - 1) // grid, splits // 16)
        chunk = (splits + want - 1) // want
        return True, chunk, (splits + chunk - 1) // chunk
    return False, splits, 1


@functools.lru_cache(maxsize=None)
def _sk_case(splits, n):
    g = torch.Generator().manual_seed(splits * 100003 + n)
    slab = torch.randint(-8, 9, (splits, n), generator=g).double()
    pre = torch.randint(-64, 65, (n,), generator=g).double()
    tot = slab.sum(0)
    assert float(slab.abs().sum(0).max()) + 64 < 2 ** 24
    return slab, pre, tot


def _sk_want(tot, pre, acc, dtype):
    return (tot + (pre if acc else 0)).to(dtype)  # float64 -> dtype: rounded once


def test_cpu_splitk_plan_and_rounding():
    """At 256 CUs both paths are taken, (100, 252) / (512, 5120) have a short last chunk, and the bf16 cases hold
    values that actually round."""
    plans = {c: _plan(*c, 256) for c in SPLITK}
    assert [c for c, p in plans.items() if p[0]] == [(32, 1024), (33, 1028), (37, 9216), (100, 252), (512, 5120)]
    assert plans[(100, 252)][1:] == (17, 6) and 100 - 5 * 17 == 15
    assert plans[(512, 5120)][1:] == (20, 26) and 512 - 25 * 20 == 12
    rounds = 0
    for c in SPLITK:
        slab, pre, tot = _sk_case(*c)
        for acc in (0, 1):
            v = tot + (pre if acc else 0)
            rounds += int((v.to(BF16).double() != v).sum())
            assert torch.equal(v.float().double(), v)
    slab, pre, tot = _sk_case(512, 5120)
    assert int((tot.to(BF16).double() != tot).sum()) > 20 and rounds > 50


@pytest.mark.parametrize("case", SPLITK, ids=lambda c: f"{c[0]}x{c[1]}")
def test_cpu_splitk_mutants_break_equality(case):
    splits, n = case
    slab, pre, tot = _sk_case(splits, n)
    _, chunk, groups = _plan(splits, n, 256)
    muts = {"row dropped": (splits // 2, 0.0), "row doubled": (splits // 3, 2.0),
            "last chunk's final row dropped": (splits - 1, 0.0)}
    for name, (row, w) in muts.items():
        m = tot + (w - 1.0) * slab[row]
        for dtype in (F32, BF16):
            for acc in (0, 1):
                assert not torch.equal(_sk_want(m, pre, acc, dtype), _sk_want(tot, pre, acc, dtype)), (name, dtype, acc)


def test_cpu_splitk_doubled_row_against_the_old_tolerance():
    """(512, 5120), one row doubled, on the OLD test's operands (randn) and tolerance; see the module docstring."""
    splits, n = 512, 5120
    torch.manual_seed(0)
    slab = torch.randn(splits, n)
    ref = slab.double().sum(0)
    inside = {}
    for dtype, atol, rtol in ((F32, 1e-4 * splits ** 0.5, 1e-5), (BF16, 1e-2 * splits ** 0.5, 1e-2)):
        got = (ref + slab[splits // 3].double()).to(dtype).double()
        want = ref.to(dtype).double()
        inside[dtype] = int(((got - want).abs() <= atol + rtol * want.abs()).sum())
    assert inside[F32] < 0.01 * n, "fp32: the old tolerance notices a whole doubled row"
    assert 0.2 * n < inside[BF16] < 0.4 * n, "bf16: about 30 % of the row's elements stay inside it"
    islab, pre, tot = _sk_case(splits, n)
    row = islab[splits // 3]
    for dtype in (F32, BF16):
        same = _sk_want(tot + row, pre, 0, dtype) == _sk_want(tot, pre, 0, dtype)
        # equality on integers: every element where the row is non-zero differs (bf16: unless both round alike)
        assert int(same.sum()) == int((row == 0).sum()) if dtype == F32 else int(same.sum()) < 0.1 * n


def _nan_guards_intact(s):
    return bool(torch.isnan(s.alloc[:s.guard]).all() and torch.isnan(s.alloc[s.guard + s.rows * s.ld:]).all())


_PATHS = set()


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", SPLITK, ids=lambda c: f"{c[0]}x{c[1]}")
def test_splitk_reduce_is_the_exact_sum(cuda, case, dtype):
    splits, n = case
    slab64, pre, tot = _sk_case(splits, n)
    lib = _L()
    cus = lib.num_cus(cuda)
    two, _, _ = _plan(splits, n, cus)
    _PATHS.add(two)
    for acc in (0, 1):
        src = Slab(splits, n, 0, F32, float("nan"), cuda, vector_rows=False)
        src.view.copy_(slab64.float().to(cuda))
        dst = Slab(1, n, 8, dtype, SENT, cuda, vector_rows=False)
        if acc:
            dst.view[0].copy_(pre.to(dtype).to(cuda))
        assert src.ptr() % 16 == 0 and dst.ptr() % 16 == 0
        _k("tony_splitk_reduce", src.ptr(), splits, n, dst.ptr(), int(dtype == BF16), acc, cus, lib.stream_ptr(cuda))
        torch.cuda.synchronize()
        dst.assert_surroundings_intact("dst")
        assert _nan_guards_intact(src), "the slab's guards"
        assert_equal(dst.view[0].cpu(), _sk_want(tot, pre, acc, dtype), f"{splits}x{n} acc={acc}")
        if not two:
            assert_equal(src.view.cpu(), slab64.float(), "one pass: the slab is only read")


@gpu
def test_splitk_reduce_refusals_write_nothing(cuda):
    lib = _L()
    st, cus = lib.stream_ptr(cuda), lib.num_cus(cuda)
    src = torch.ones(4, 64, device=cuda)
    for dtype, step in ((F32, 4), (BF16, 2)):
        dst = Slab(1, 64, 8, dtype, SENT, cuda, vector_rows=False)
        bf = int(dtype == BF16)
        _k("tony_splitk_reduce", src.data_ptr(), 4, 62, dst.ptr(), bf, 0, cus, st, rc=-1)       # n % 4
        _k("tony_splitk_reduce", src.data_ptr(), 4, 60, dst.ptr() + step, bf, 0, cus, st, rc=-1)  # misaligned dst
        _k("tony_splitk_reduce", src.data_ptr(), 0, 64, dst.ptr(), bf, 0, cus, st, rc=-1)       # no splits
        _k("tony_splitk_reduce", src.data_ptr() + 4, 4, 60, dst.ptr(), bf, 0, cus, st, rc=-1)   # misaligned slab
        torch.cuda.synchronize()
        assert_equal(dst.alloc.cpu(), torch.full_like(dst.alloc, SENT).cpu(), "nothing written")


# ------------------------------------------------------------------------------------------- transpose --
T_SHAPES = [(32, 3, 3, 3), (40, 24, 1, 1), (64, 64, 1, 1), (72, 136, 3, 1), (200, 8, 1, 7), (12, 20, 1, 1),
            (16, 8, 1, 1)]
_FINITE = 0x7F80  # bf16 bit patterns 0 .. 0x7F7F: the non-negative finite numbers


def _t_bits(shape, index, salt):
    """[Co, R, S, Ci]-ordered int16 bit patterns, all distinct within the weight."""
    co, ci, r, s = shape
    n = co * ci * r * s
    assert n < _FINITE
    return ((torch.arange(n, dtype=torch.int64) * 7 + 977 * index + salt) % _FINITE).to(torch.int16).view(co, r, s, ci)


def _t_weight(shape, index, dev):
    """A channels_last bf16 Parameter [Co, Ci, R, S]; the last one starts 8 bytes into its storage."""
    co, ci, r, s = shape
    n = co * ci * r * s
    off = 4 if index == len(T_SHAPES) - 1 else 0
    store = torch.zeros(n + 8, dtype=BF16, device=dev)
    w = nn.Parameter(store[off:off + n].view(co, r, s, ci).permute(0, 3, 1, 2), requires_grad=False)
    assert w.is_contiguous(memory_format=torch.channels_last) and w.data_ptr() % 16 == 2 * off
    return w


def _t_set(w, shape, index, salt):
    co, ci, r, s = shape
    w.data.permute(0, 2, 3, 1).view(torch.int16).copy_(_t_bits(shape, index, salt).to(w.device))


def test_cpu_transpose_swapped_pair_shows():
    for i, shape in enumerate(T_SHAPES):
        b = _t_bits(shape, i, 0).reshape(-1)
        assert b.unique().numel() == b.numel() and not torch.equal(_t_bits(shape, i, 0), _t_bits(shape, i, 5))
        assert not torch.equal(_t_bits(shape, i, 0), _t_bits(shape, (i + 1), 0))


@gpu
def test_transpose_batch_every_branch(cuda):
    from tony_amd.ops.wt_cache import TransposedWeights

    c = TransposedWeights(cuda)
    c.enabled = True
    ws, dsts = [], []
    for i, shape in enumerate(T_SHAPES):
        co, ci, r, s = shape
        w = _t_weight(shape, i, cuda)
        _t_set(w, shape, i, 0)
        d = Slab(1, w.numel(), 8, BF16, SENT, cuda, vector_rows=False)
        assert d.ptr() % 16 == 0
        buf = d.view[0].view(ci, r, s, co)
        c.entries[id(w)] = (w, buf, w.data_ptr())  # registered by hand: get() allocates its own buffer
        ws.append(w)
        dsts.append((d, buf))
    c._build()
    assert c.n_desc == len(T_SHAPES)
    _CALLED.add("tony_transpose_desc_bytes")
    for salt in (0, 5):  # the second round: the weights changed, refresh() again
        for i, (w, shape) in enumerate(zip(ws, T_SHAPES)):
            _t_set(w, shape, i, salt)
        c.refresh()
        _CALLED.add("tony_transpose_batch")
        torch.cuda.synchronize()
        for i, (w, (d, buf)) in enumerate(zip(ws, dsts)):
            d.assert_surroundings_intact(f"transposed {T_SHAPES[i]}")
            want = w.data.permute(1, 2, 3, 0).contiguous()
            assert_equal(buf.view(torch.int16).cpu(), want.view(torch.int16).cpu(), f"{T_SHAPES[i]} salt {salt}")
            assert c.get(w) is buf  # the public lookup serves the registered copy
    # a weight get() has not seen: copied on the spot, joins the batch, refreshed with the rest
    extra = _t_weight((24, 16, 1, 1), 1, cuda)
    _t_set(extra, (24, 16, 1, 1), 1, 0)
    got = c.get(extra)
    assert torch.equal(got, extra.data.permute(1, 2, 3, 0).contiguous()) and c.n_desc == len(T_SHAPES) + 1
    _t_set(extra, (24, 16, 1, 1), 1, 9)
    c.refresh()
    torch.cuda.synchronize()
    assert torch.equal(c.get(extra).view(torch.int16), extra.data.permute(1, 2, 3, 0).contiguous().view(torch.int16))
    _k("tony_transpose_batch", 0, 1, 1, _L().stream_ptr(cuda), rc=-1)  # no work list: refused


# ---------------------------------------------------------------------------------------------- linear --
LIN = [(1, 64, 16), (5, 64, 16), (37, 768, 1000)]


@functools.lru_cache(maxsize=None)
def _lin_case(m, k, n):
    g = torch.Generator().manual_seed(m * 1009 + k + n)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()  # noqa: E731
    x, w, b, dy = ri(-2, 2, (m, k)), ri(-2, 2, (n, k)), ri(-4, 4, (n,)), ri(-2, 2, (m, n))
    prew, preb = ri(-64, 64, (n, k)), ri(-64, 64, (n,))
    if k >= 768:  # aligned rows: y[0, 0] = |w_0|^2 ~ 1500 and its neighbours, so that the bf16 store of y rounds
        x[0] = w[0]
        w[1], w[2] = w[0], -w[0]
        w[2, ::5] = 0
    y, dx, dw, db = x @ w.t() + b, dy @ w, dy.t() @ x, dy.sum(0)
    for t in (y, dx, dw, db):
        assert float(t.abs().max()) < 2 ** 24
    assert float((prew + dw).abs().max()) < 256 and float((preb + db).abs().max()) < 256 and float(db.abs().max()) < 256
    return dict(x=x, w=w, b=b, dy=dy, prew=prew, preb=preb, y=y, dx=dx, dw=dw, db=db)


def test_cpu_linear_mutants_break_equality():
    """One row of x dropped from dW / db, one k-slice dropped from y: integers differ, also after the bf16 store."""
    for mkn in LIN:
        c = _lin_case(*mkn)
        x, w, dy = c["x"], c["w"], c["dy"]
        assert not torch.equal((dy[1:].t() @ x[1:]).to(BF16), c["dw"].to(BF16)) or mkn[0] == 1
        assert not torch.equal((x[:, 8:] @ w[:, 8:].t() + c["b"]).to(BF16), c["y"].to(BF16))
        assert not torch.equal((x @ w.t()).to(BF16), c["y"].to(BF16))  # the bias left out
        assert int((c["y"].to(BF16).double() != c["y"]).sum()) > 0 or mkn[1] < 768  # y really rounds at k = 768


def _linear_pass(dev, c, slot, strided=False):
    from tony_amd.ops.linear import Linear, supported

    m, k = c["x"].shape
    n = c["w"].shape[0]
    lin = Linear(k, n).to(dev, BF16)
    with torch.no_grad():
        lin.weight.copy_(c["w"])
        lin.bias.copy_(c["b"])
    if slot:
        lin.weight.grad = c["prew"].to(BF16).to(dev)
        lin.bias.grad = c["preb"].to(BF16).to(dev)
    if strided:
        big = torch.full((m, k + 4), float("nan"), dtype=BF16, device=dev)
        big[:, :k] = c["x"].to(BF16).to(dev)
        x = big[:, :k]
        assert x.stride(0) % 8 != 0
    else:
        x = c["x"].to(BF16).to(dev)
    x.requires_grad_(True)
    assert supported(x, lin.weight)
    y = lin(x)
    y.backward(c["dy"].to(BF16).to(dev))
    _CALLED.add("ops.linear")
    return y.detach().cpu(), x.grad.cpu(), lin.weight.grad.cpu(), lin.bias.grad.cpu()


def _check_linear(c, got, slot, what):
    y, dx, dw, db = got
    assert_equal(y, c["y"].to(BF16), f"{what} y")
    assert_equal(dx, c["dx"].to(BF16), f"{what} dx")
    assert_equal(dw, (c["dw"] + (c["prew"] if slot else 0)).to(BF16), f"{what} dW")
    assert_equal(db, (c["db"] + (c["preb"] if slot else 0)).to(BF16), f"{what} db")


@gpu
@pytest.mark.parametrize("slot", [False, True], ids=["returned", "bf16-slot"])
@pytest.mark.parametrize("mkn", LIN, ids=lambda s: "x".join(map(str, s)))
def test_linear_is_exact_on_integers(cuda, monkeypatch, mkn, slot):
    from tony_amd.ops import linear

    monkeypatch.setattr(linear, "TUNE", False)
    c = _lin_case(*mkn)
    _check_linear(c, _linear_pass(cuda, c, slot), slot, f"{mkn} slot={slot}")


@gpu
def test_linear_tuned_and_strided_input(cuda, monkeypatch):
    """The smallest shape with the per-shape tile choice on, and an x whose row stride is no multiple of 8 (the
    copy path): the same exact results."""
    from tony_amd.ops import linear

    c = _lin_case(5, 64, 16)
    monkeypatch.setattr(linear, "TUNE", True)
    _check_linear(c, _linear_pass(cuda, c, False), False, "tuned")
    monkeypatch.setattr(linear, "TUNE", False)
    _check_linear(c, _linear_pass(cuda, c, True, strided=True), True, "strided x")


@gpu
@pytest.mark.parametrize("mkn", LIN, ids=lambda s: "x".join(map(str, s)))
def test_linear_dw_into_an_fp32_slot(cuda, mkn):
    """dW = dy^T x summed into an fp32 slot (ops/gemm.py wgrad_tn with dst, the form FlatParams' fp32 gradients
    take) and returned as a new fp32 tensor."""
    from tony_amd.ops.gemm import wgrad_tn

    c = _lin_case(*mkn)
    m, k = c["x"].shape
    n = c["w"].shape[0]
    x, dy = c["x"].to(BF16).to(cuda), c["dy"].to(BF16).to(cuda)
    slot = c["prew"].float().to(cuda)
    assert wgrad_tn(dy.data_ptr(), n, x.data_ptr(), k, m, n, k, cuda, dst=slot) is None
    assert_equal(slot.cpu(), (c["prew"] + c["dw"]).float(), "fp32 slot")
    assert_equal(wgrad_tn(dy.data_ptr(), n, x.data_ptr(), k, m, n, k, cuda).cpu(), c["dw"].float(), "returned fp32")
    _CALLED.add("ops.gemm.wgrad_tn")


@gpu
def test_linear_unsupported_shape_falls_back(cuda):
    from tony_amd.ops.linear import linear, supported

    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (5, 60), generator=g).to(BF16).to(cuda)
    w = torch.randint(-2, 3, (16, 60), generator=g).to(BF16).to(cuda)
    b = torch.randint(-4, 5, (16,), generator=g).to(BF16).to(cuda)
    assert not supported(x, w) and supported(x[:, :56].contiguous(), w[:, :56].contiguous())
    assert_equal(linear(x, w, b), F.linear(x, w, b), "k % 8 != 0: F.linear")
    assert_equal(linear(x, w, b).cpu(), (x.double() @ w.double().t() + b.double()).to(BF16).cpu(), "and exact")


@gpu
def test_zz_every_glue_entry_point_ran(cuda):
    """The combine took both of its paths at this device's CU count, and every entry point of this module ran
    (the module run as a whole)."""
    assert _PATHS == {True, False}, f"split-K paths taken at {_L().num_cus(cuda)} CUs: {_PATHS}"
    names = {"tony_splitk_reduce", "tony_transpose_batch", "tony_transpose_desc_bytes", "ops.linear",
             "ops.gemm.wgrad_tn"}
    missing = sorted(names - _CALLED)
    assert not missing, f"entry points no case of this module called: {missing}"
