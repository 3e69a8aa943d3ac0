"""The MNIST HIP kernels (csrc/conv1.hip, conv1_pool.hip, conv2.hip, dense.hip, dense_xent.hip) where their value
tests (test_conv1_gpu.py, test_conv1_pool_gpu.py, test_conv2_gpu.py, test_dense_gpu.py, test_dense_xent_gpu.py) do
not look: around the buffers, at non-finite values, at refused calls, and in ``dense_xent``'s ``gout`` branches.

A  Every one of the 19 entry points is called directly, the way ops/*.py call it, with each input inside a NaN-filled
   allocation (labels: an out-of-range integer, idx: 255) and each destination, the partials included, inside a
   sentinel-filled one (exact_helpers.Slab).  The destination equals float64 on small integers bit for bit (the
   ``dense_xent`` floats: the public wrapper's bits on plain tensors), holds no NaN (a clamped load zeroed by a
   multiplication instead of a select would leak one), and nothing outside it has changed.  The partials have exactly
   the size the wrappers allocate.
B  NaN, +inf and -inf planted in x, w, bias or dy / gout, through the public ops, against the float64 CPU composition
   (F.conv2d, F.relu, F.max_pool2d, F.linear, F.cross_entropy and autograd): identical NaN / +inf / -inf masks, equal
   values where the reference is finite, and the pooled ops' idx equal to ``return_indices`` in every window that
   holds a NaN (torch: the LAST NaN of a window wins).
   What this found: all four backward kernels masked dy with ``y > 0``, which sends 0 through a NaN activation where
   torch's threshold_backward (``y <= 0 ? 0 : dy``) sends dy: with a NaN in x, w or bias the bias gradient (and parts
   of dW / dX) came out finite where the composition's is NaN.  The kernels now mask with ``!(y <= 0)``.
   Two documented differences are pinned rather than matched (see test_b_conv2 and test_b_dense_xent).
C  Every ``return -n`` that small arguments can reach, per entry point: the code, and no byte of any destination
   written.  Each of these calls returns before any launch (read in the source; a misaligned pointer that WAS
   launched would fault).  And the Python predicates on GPU tensors: off the native form the ops are the composition,
   to the bit.
D  ``dense_xent`` with ``reduction="sum"`` (gout read with stride 0), ``"mean"``, a float64 and a stride-2 gout (the
   recast branch) and M = 1.  Worst error / bound on an MI355X at 33x10x36 with three ignored rows (printed; a record
   beside test_dense_xent_gpu.py's, not a knob): see the figures in test_d_sum_and_mean's docstring.
E  test_zz_every_entry_point_ran: all 19 names ran in A, and every one that takes a pointer was refused in C.

tests/test_mnist_exact_cpu.py holds the sensitivity half: the comparison functions used here fail on a model of each
fault they are for.
"""
import pytest
import torch
import torch.nn.functional as F
from exact_helpers import (SENT, assert_clean, assert_equal, assert_nan_windows_idx, assert_same_specials, flat_slab,
                           guarded, window_positions)

pytestmark = pytest.mark.gpu

F32, U8, I64 = torch.float32, torch.uint8, torch.int64
NAN, INF = float("nan"), float("inf")
IDX_SENT = 0xA5
_RAN, _REFUSED = set(), set()


def _L():
    from tony_amd.ops import _lib
    return _lib


def _call(dev, name, *args, rc=0, stream=True):
    """Entry point ``name`` with slabs passed as their interior's address; asserts and records the return code."""
    lib = _L()
    raw = [a.ptr() if hasattr(a, "assert_surroundings_intact") else a for a in args]
    with torch.cuda.device(dev):
        got = getattr(lib.lib(), name)(*raw, *([lib.stream_ptr(dev)] if stream else []))
    if not stream:  # a *_grid / splits query: the value is the result
        _RAN.add(name)
        return got
    assert got == rc, f"{name} returned {got}, expected {rc}"
    (_RAN if rc == 0 else _REFUSED).add(name)
    return got


def _out(numel, dev, ld=1, dtype=F32):
    return flat_slab(numel, dtype, IDX_SENT if dtype == U8 else SENT, dev, ld)


def _idx_in(t, dev):
    return guarded(t, dev, fill=255)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _finite_inside(slab, what):
    torch.cuda.synchronize()
    assert not bool(slab.view.isnan().any()), f"{what}: NaN in the destination"
    slab.assert_surroundings_intact(what)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def _conv_inputs(cin, cout, k, p, nhw, pool):
    n, h, w = nhw
    g = torch.Generator().manual_seed(cin * 7919 + k * 1000 + 10 * p + sum(nhw) + int(pool))
    oh, ow = h + 2 * p - k + 1, w + 2 * p - k + 1
    ys = (n, cout, oh // 2, ow // 2) if pool else (n, cout, oh, ow)
    return (_ints(g, (n, cin, h, w), 0, 3), _ints(g, (cout, cin, k, k), -2, 2), _ints(g, (cout,), -4, 4),
            _ints(g, ys, -2, 2))


def conv_reference(x, wt, b, p, pool, dy, x_grad):
    """float64 CPU composition: dict of y, pos (window positions, pooled only), full (the ReLU output at full
    resolution), dfull (the gradient at the conv output), dx (or None), dw, db."""
    xr, wr, br = (t.double().requires_grad_() for t in (x, wt, b))
    conv = F.conv2d(xr, wr, br, padding=p)
    full = F.relu(conv)
    pos = None
    if pool:
        y, flat = F.max_pool2d(full, 2, return_indices=True)
        pos = window_positions(flat, full.shape[-1])
    else:
        y = full
    wanted = (wr, br, conv) + ((xr,) if x_grad else ())
    grads = torch.autograd.grad(y, wanted, dy.double())
    return {"y": y.detach(), "pos": pos, "full": full.detach(), "dw": grads[0], "db": grads[1], "dfull": grads[2],
            "dx": grads[3] if x_grad else None}


def dense_dgrad_model(dfull, wt, k, p):
    """conv2's data gradient as the kernel forms it: a correlation of dY' INCLUDING its halo of k - 1 - p zeros with
    the reversed taps, so a non-finite weight meets the halo's zeros (0 * NaN) at the border pixels."""
    q = k - 1 - p
    return F.conv2d(F.pad(dfull.double(), (q, q, q, q)), wt.double().flip(2, 3).transpose(0, 1))


def dense_reference(x, w, b, relu, dy):
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    y = F.linear(xr, wr, br)
    y = F.relu(y) if relu else y
    return [y.detach(), *torch.autograd.grad(y, (xr, wr, br), dy.double())]


def xent_reference(x, w, b, labels, gout, explicit_d=False):
    """float64 (loss, logits, dx, dw, db) of cross_entropy(linear(x)), every label live.  ``explicit_d``: the
    gradients from d = gout (softmax - onehot), the line the kernel states, instead of torch's autograd."""
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    z = F.linear(xr, wr, br)
    loss = F.cross_entropy(z, labels, reduction="none")
    if explicit_d:
        zd = z.detach()
        d = gout.double()[:, None] * ((zd - torch.logsumexp(zd, 1, keepdim=True)).exp()
                                      - F.one_hot(labels, w.shape[0]).double())
        grads = (d @ w.double(), d.t() @ x.double(), d.sum(0))
    else:
        grads = torch.autograd.grad(loss, (xr, wr, br), gout.double())
    return [loss.detach(), z.detach(), *grads]


# ---------------------------------------------------------------------------------------------------------------------
# A: direct calls on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------

KP = [(k, p) for k in (3, 5) for p in (0, (k - 1) // 2)]
CONV1_CASES = [(k, p, nhw) for k, p in KP for nhw in ((1, k, k), (3, 9, 8), (1, 6, 300))]
CONV1_POOL_CASES = [(k, p, nhw) for k, p in KP for nhw in ((1, k + 1, k + 1), (3, 9, 8), (1, 6, 600))]
CONV2_CASES = [(k, p, nhw) for k, p in KP for nhw in ((1, k + 1, k + 1), (3, 9, 11), (1, 40, 12), (1, 8, 64 - 2 * p))]
DENSE_CASES = [(relu, mnk) for relu in (False, True) for mnk in ((1, 1, 4), (33, 10, 36), (3, 33, 2500), (130, 10, 128))]
XENT_SHAPES = [(1, 1, 4), (33, 10, 36), (130, 10, 128), (5, 32, 36)]


def _conv1_backward(dev, pool, dy, r, xs, nhw, k, p):
    """The weight / bias gradient launches of conv1 (pooled or not) on guarded buffers, against the reference."""
    n, h, w = nhw
    fam = "tony_conv1_pool_" if pool else "tony_conv1_"
    grid = _call(dev, fam + "bwd_grid", n, stream=False)
    assert grid == -(-n // 2)
    part = _out(grid * 32 * 32, dev, ld=32)  # ops/conv1.py: grid * COUT * 32
    saved = [guarded(dy, dev), guarded(r["y"].float(), dev)] + ([_idx_in(r["pos"], dev)] if pool else [])
    _call(dev, fam + "bwd", *saved, xs, part, n, h, w, k, p)
    _finite_inside(part, "partials")
    dws, dbs = _out(32 * k * k, dev, ld=k * k), _out(32, dev)
    _call(dev, "tony_conv1_fold", part, grid, k, dws, dbs)
    assert_clean(dws, r["dw"].float(), "dW")
    assert_clean(dbs, r["db"].float(), "db")
    part.assert_surroundings_intact("partials after the fold")


@pytest.mark.parametrize("k,p,nhw", CONV1_CASES)
def test_a_conv1(cuda, k, p, nhw):
    n, h, w = nhw
    x, wt, b, dy = _conv_inputs(1, 32, k, p, nhw, False)
    r = conv_reference(x, wt, b, p, False, dy, False)
    xs, ws, bs = guarded(x, cuda, ld=w), guarded(wt, cuda, ld=k * k), guarded(b, cuda)
    ys = _out(r["y"].numel(), cuda, ld=r["y"].shape[-1])
    _call(cuda, "tony_conv1_fwd", xs, ws, bs, ys, n, h, w, k, p)
    assert_clean(ys, r["y"].float(), "y")
    _conv1_backward(cuda, False, dy, r, xs, nhw, k, p)


@pytest.mark.parametrize("k,p,nhw", CONV1_POOL_CASES)
def test_a_conv1_pool(cuda, k, p, nhw):
    n, h, w = nhw
    x, wt, b, dy = _conv_inputs(1, 32, k, p, nhw, True)
    r = conv_reference(x, wt, b, p, True, dy, False)
    xs, ws, bs = guarded(x, cuda, ld=w), guarded(wt, cuda, ld=k * k), guarded(b, cuda)
    ys = _out(r["y"].numel(), cuda, ld=r["y"].shape[-1])
    ids = _out(r["y"].numel(), cuda, ld=r["y"].shape[-1], dtype=U8)
    _call(cuda, "tony_conv1_pool_fwd", xs, ws, bs, ys, ids, n, h, w, k, p)
    assert_clean(ys, r["y"].float(), "y")
    assert_clean(ids, r["pos"], "idx")
    _conv1_backward(cuda, True, dy, r, xs, nhw, k, p)


@pytest.mark.parametrize("k,p,nhw", CONV2_CASES)
def test_a_conv2(cuda, k, p, nhw):
    n, h, w = nhw
    x, wt, b, dy = _conv_inputs(32, 64, k, p, nhw, True)
    r = conv_reference(x, wt, b, p, True, dy, True)
    xs, ws, bs = guarded(x, cuda, ld=w), guarded(wt, cuda, ld=32 * k * k), guarded(b, cuda)
    pw = r["y"].shape[-1]
    ys, ids = _out(r["y"].numel(), cuda, ld=pw), _out(r["y"].numel(), cuda, ld=pw, dtype=U8)
    _call(cuda, "tony_conv2_fwd", xs, ws, bs, ys, ids, n, h, w, k, p)
    assert_clean(ys, r["y"].float(), "y")
    assert_clean(ids, r["pos"], "idx")
    saved = [guarded(dy, cuda, ld=pw), guarded(r["y"].float(), cuda, ld=pw), _idx_in(r["pos"], cuda)]
    dxs = _out(x.numel(), cuda, ld=w)
    _call(cuda, "tony_conv2_dgrad", *saved, ws, dxs, n, h, w, k, p)
    assert_clean(dxs, r["dx"].float(), "dX")
    grid = _call(cuda, "tony_conv2_wgrad_grid", n, stream=False)
    assert grid == -(-n // 2)
    part = _out(grid * (k * k * 64 * 32 + 64), cuda, ld=32)  # ops/conv2.py: grid * (k * k * COUT * CIN + COUT)
    _call(cuda, "tony_conv2_wgrad", *saved, xs, part, n, h, w, k, p)
    _finite_inside(part, "partials")
    assert not bool((part.view == SENT).any()), "partials: an element the kernel did not write"
    dws, dbs = _out(wt.numel(), cuda, ld=k * k), _out(64, cuda)
    _call(cuda, "tony_conv2_fold", part, grid, k, dws, dbs)
    assert_clean(dws, r["dw"].float(), "dW")
    assert_clean(dbs, r["db"].float(), "db")
    part.assert_surroundings_intact("partials after the fold")


@pytest.mark.parametrize("relu,mnk", DENSE_CASES)
def test_a_dense(cuda, relu, mnk):
    m, n, k = mnk
    g = torch.Generator().manual_seed(m * 1000003 + n * 1009 + k)
    x, w, b, dy = _ints(g, (m, k), 0, 3), _ints(g, (n, k), -2, 2), _ints(g, (n,), -4, 4), _ints(g, (m, n), -2, 2)
    yr, dxr, dwr, dbr = dense_reference(x, w, b, relu, dy)
    xs, ws, bs = guarded(x, cuda, ld=k), guarded(w, cuda, ld=k), guarded(b, cuda)
    assert xs.ptr() % 16 == 0 and ws.ptr() % 16 == 0
    splits = _call(cuda, "tony_dense_splits", m, n, k, stream=False)
    assert (splits > 1) == (mnk == (3, 33, 2500))
    ys = _out(m * n, cuda, ld=n)
    if splits > 1:
        part = _out(splits * m * n, cuda, ld=n)  # ops/dense.py: splits * m * n
        _call(cuda, "tony_dense_fwd", xs, ws, bs, ys, part, m, n, k, int(relu))
        _finite_inside(part, "partials")
        assert not bool((part.view == SENT).any()), "partials: an element the kernel did not write"
        assert bool((ys.alloc == SENT).all()), "y written by the split forward"
        _call(cuda, "tony_dense_fold", part, bs, ys, splits, m, n, int(relu))
        part.assert_surroundings_intact("partials after the fold")
    else:
        _call(cuda, "tony_dense_fwd", xs, ws, bs, ys, None, m, n, k, int(relu))
        # the fold on its own: one guarded partial holding x w^T gives the same y
        part, y2 = guarded((x.double() @ w.double().t()).float(), cuda, fill=NAN, ld=n), _out(m * n, cuda, ld=n)
        _call(cuda, "tony_dense_fold", part, bs, y2, 1, m, n, int(relu))
        assert_clean(y2, yr.float(), "y of the fold")
    assert_clean(ys, yr.float(), "y")
    dys, ysaved = guarded(dy, cuda, ld=n), guarded(yr.float(), cuda, ld=n)
    dxs, dws, dbs = _out(m * k, cuda, ld=k), _out(n * k, cuda, ld=k), _out(n, cuda)
    _call(cuda, "tony_dense_dgrad", dys, ysaved, ws, dxs, m, n, k, int(relu))
    assert_clean(dxs, dxr.float(), "dx")
    _call(cuda, "tony_dense_wgrad", dys, ysaved, xs, dws, dbs, m, n, k, int(relu))
    assert_clean(dws, dwr.float(), "dw")
    assert_clean(dbs, dbr.float(), "db")


def _xent_inputs(mnk):
    m, n, k = mnk
    g = torch.Generator().manual_seed(m * 1000003 + n * 1009 + k + 1)
    x, w, b = _ints(g, (m, k), 0, 3), _ints(g, (n, k), -2, 2), _ints(g, (n,), -4, 4)
    labels = torch.randint(0, n, (m,), generator=g)
    if mnk == (33, 10, 36):
        labels[[0, 7, 32]] = torch.tensor([-100, n, -100])
    return x, w, b, labels, _ints(g, (m,), -2, 2)


@pytest.mark.parametrize("gs", [1, 0])
@pytest.mark.parametrize("want_dx", [True, False])
@pytest.mark.parametrize("mnk", XENT_SHAPES)
def test_a_dense_xent(cuda, mnk, want_dx, gs):
    from tony_amd.ops.dense_xent import _DenseXent, dense_xent

    m, n, k = mnk
    x, w, b, labels, gout = _xent_inputs(mnk)
    if gs == 0:
        gout = torch.full((m,), -2.0)
    # the public wrapper on plain tensors (held to its bound by test_dense_xent_gpu.py), a contiguous gout
    xp, wp, bp = x.to(cuda).requires_grad_(want_dx), w.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    loss, logits = dense_xent(xp, wp, bp, labels.to(cuda), reduction="none", return_logits=True)
    assert isinstance(loss.grad_fn, _DenseXent._backward_cls)
    lse = loss.grad_fn.saved_tensors[4]
    loss.backward(gout.to(cuda))
    assert_equal(logits.cpu().double(), F.linear(x.double(), w.double(), b.double()), "the wrapper's logits")

    xs, ws, bs = guarded(x, cuda, ld=k), guarded(w, cuda, ld=k), guarded(b, cuda)
    assert xs.ptr() % 16 == 0 and ws.ptr() % 16 == 0
    labs = guarded(labels, cuda, fill=2 ** 62 if gs else -1)
    lgs, lss, los = _out(m * n, cuda, ld=n), _out(m, cuda), _out(m, cuda)
    _call(cuda, "tony_dense_xent_fwd", xs, ws, bs, labs, lgs, lss, los, m, n, k)
    assert_clean(lgs, logits.detach().cpu(), "logits")
    assert_clean(lss, lse.cpu(), "lse")
    assert_clean(los, loss.detach().cpu(), "loss")
    gos = guarded(gout if gs else gout[:1], cuda)  # stride 0: ONE element, NaN on both sides of it
    dxs = _out(m * k, cuda, ld=k) if want_dx else None
    dws, dbs = _out(n * k, cuda, ld=k), _out(n, cuda)
    _call(cuda, "tony_dense_xent_bwd", gos, gs, guarded(logits.detach(), cuda, ld=n), guarded(lse, cuda), labs, xs, ws,
          dxs, dws, dbs, m, n, k)
    if want_dx:
        assert_clean(dxs, xp.grad.cpu(), "dx")
    assert_clean(dws, wp.grad.cpu(), "dw")
    assert_clean(dbs, bp.grad.cpu(), "db")


# ---------------------------------------------------------------------------------------------------------------------
# B: non-finite values through the public ops
# ---------------------------------------------------------------------------------------------------------------------

KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF}
B_CASES = [(kind, where) for kind in KINDS for where in ("x", "w", "b", "dy")]
# fixed positions; x: image 0 at an even conv column (a window whose only NaN is position 0, windows with several),
# image 1 at an odd one (a window whose only NaN is position 1), both clear of a dropped odd last row / column
CONV_SPOTS = {"x": [(0, 0, 3, 3), (1, 0, 3, 4)], "w": [(5, 0, 0, 0), (9, 0, 2, 1)], "b": [(7,)],
              "dy": [(0, 4, 1, 2), (1, 20, 2, 3)]}


def _plant(tensors, where, spots, value):
    t = tensors[("x", "w", "b", "dy").index(where)]
    for s in spots:
        t[s] = value
    return tensors


def windows(full, ph, pw):
    """[N, C, 2 ph.., 2 pw..] -> [N, C, ph, pw, 4]: the 2x2 windows in position order."""
    return full[..., :2 * ph, :2 * pw].unflatten(-2, (ph, 2)).unflatten(-1, (pw, 2)).permute(0, 1, 2, 4, 3, 5).flatten(-2)


def _assert_window_kinds(full, ph, pw):
    win = windows(full, ph, pw)
    m = win.isnan()
    assert bool((m[..., 0] & ~m[..., 1:].any(-1)).any()), "no window whose only NaN is position 0"
    later = torch.maximum(win[..., 2], win[..., 3])
    assert bool((~m[..., 0] & m[..., 1] & ~m[..., 2] & ~m[..., 3] & (later > win[..., 0])).any()), \
        "no window with its NaN at position 1 and a larger finite value later"
    assert bool((m.sum(-1) > 1).any()), "no window with several NaNs"


@pytest.mark.parametrize("kind,where", B_CASES)
@pytest.mark.parametrize("pool", [False, True])
def test_b_conv1(cuda, pool, kind, where):
    from tony_amd.ops.conv1 import _Conv1BiasReLU, _Conv1BiasReLUPool, _forward_pool, conv1_bias_relu

    k, p, nhw = 3, 1, (2, 8, 11) if pool else (2, 7, 9)
    x, wt, b, dy = _plant(list(_conv_inputs(1, 32, k, p, nhw, pool)), where, CONV_SPOTS[where], KINDS[kind])
    r = conv_reference(x, wt, b, p, pool, dy, False)
    xg, wg, bg = x.to(cuda), wt.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    y = conv1_bias_relu(xg, wg, bg, p, pool)
    assert isinstance(y.grad_fn, (_Conv1BiasReLUPool if pool else _Conv1BiasReLU)._backward_cls)
    dw, db = torch.autograd.grad(y, (wg, bg), dy.to(cuda))
    assert_same_specials(y.detach().cpu(), r["y"], "y")
    if pool:
        idx = _forward_pool(xg, wg.detach(), bg.detach(), p)[1].cpu()
        nanwin = assert_nan_windows_idx(idx, r["pos"], r["full"], "idx in the windows that hold a NaN")
        if kind == "nan":
            assert bool(nanwin.any()) == (where != "dy")
        if (kind, where) == ("nan", "x"):
            _assert_window_kinds(r["full"], *idx.shape[-2:])
    assert_same_specials(dw.cpu(), r["dw"], "dW")
    assert_same_specials(db.cpu(), r["db"], "db")


@pytest.mark.parametrize("kind,where", B_CASES)
def test_b_conv2(cuda, kind, where):
    """Pinned difference, dX with a non-finite WEIGHT: the kernel's data gradient is a dense correlation over dY'
    with its halo of k - 1 - p zeros, so at the border pixels the special weight meets a zero of the halo and
    0 * NaN (0 * inf) = NaN; torch's col2im never forms those products and leaves them finite there.  No defect (an
    infinite weight has no meaningful gradient either way), so dX is held to dense_dgrad_model, the float64
    correlation WITH the halo, and the composition's NaNs must be a subset of it."""
    from tony_amd.ops.conv2 import _Conv2BiasReLUPool, _forward, conv2_bias_relu_pool

    k, p, nhw = 3, 1, (2, 9, 11)
    spots = dict(CONV_SPOTS, x=[(0, 3, 3, 3), (1, 30, 3, 4)], w=[(5, 2, 0, 0), (9, 17, 2, 1)])[where]
    x, wt, b, dy = _plant(list(_conv_inputs(32, 64, k, p, nhw, True)), where, spots, KINDS[kind])
    r = conv_reference(x, wt, b, p, True, dy, True)
    xg, wg, bg = (t.to(cuda).requires_grad_() for t in (x, wt, b))
    y = conv2_bias_relu_pool(xg, wg, bg, p)
    assert isinstance(y.grad_fn, _Conv2BiasReLUPool._backward_cls)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.to(cuda))
    assert_same_specials(y.detach().cpu(), r["y"], "y")
    idx = _forward(xg.detach(), wg.detach(), bg.detach(), p)[1].cpu()
    assert_nan_windows_idx(idx, r["pos"], r["full"], "idx in the windows that hold a NaN")
    if (kind, where) == ("nan", "x"):
        _assert_window_kinds(r["full"], *idx.shape[-2:])
    want_dx = r["dx"]
    if where == "w":
        want_dx = dense_dgrad_model(r["dfull"], wt, k, p)
        assert bool((want_dx.isnan() | ~r["dx"].isnan()).all())  # the composition's NaNs are among the model's
        both = want_dx.isfinite() & r["dx"].isfinite()
        assert torch.equal(want_dx[both], r["dx"][both])
    assert_same_specials(dx.cpu(), want_dx, "dX")
    assert_same_specials(dw.cpu(), r["dw"], "dW")
    assert_same_specials(db.cpu(), r["db"], "db")


DENSE_SPOTS = {"x": [(4, 5), (20, 6)], "w": [(3, 5), (8, 30)], "b": [(7,)], "dy": [(6, 2), (32, 9)]}


@pytest.mark.parametrize("kind,where", B_CASES)
@pytest.mark.parametrize("relu", [False, True])
def test_b_dense(cuda, relu, kind, where):
    from tony_amd.ops.dense import _Dense, dense

    m, n, k = 33, 10, 36
    g = torch.Generator().manual_seed(33 * 1000003 + 10 * 1009 + 36)
    ins = [_ints(g, (m, k), 0, 3), _ints(g, (n, k), -2, 2), _ints(g, (n,), -4, 4), _ints(g, (m, n), -2, 2)]
    x, w, b, dy = _plant(ins, where, DENSE_SPOTS[where], KINDS[kind])
    want = dense_reference(x, w, b, relu, dy)
    xg, wg, bg = (t.to(cuda).requires_grad_() for t in (x, w, b))
    y = dense(xg, wg, bg, relu)
    assert isinstance(y.grad_fn, _Dense._backward_cls)
    got = [y.detach(), *torch.autograd.grad(y, (xg, wg, bg), dy.to(cuda))]
    for name, a, r in zip(("y", "dx", "dw", "db"), got, want):
        assert_same_specials(a.cpu(), r, name)


XENT_J = 5  # the planted column: weight +1 in every class, x >= 1 in every row


def xent_b_inputs(kind, where):
    """33 x 10 x 36 integers with one kind of special planted; every label live and off the classes 3 and 7 that a
    -inf in w / bias removes.  Rows of logits that occur: a +inf (x +inf: all +inf; w / bias +inf), only -inf (x -inf
    through the all-ones column), one -inf among finite values (w / bias -inf), a NaN (any NaN; x +-inf through a
    column of mixed signs).  The rows whose gout is special have x = 0, so their logits are the bias and no softmax
    term rounds to 0 or 1 in fp32 (0 * inf would differ from float64's tiny * inf)."""
    m, n, k = 33, 10, 36
    g = torch.Generator().manual_seed(20250101)
    x, w, b = _ints(g, (m, k), 0, 3), _ints(g, (n, k), -2, 2), _ints(g, (n,), -4, 4)
    labels = torch.randint(0, n, (m,), generator=g)
    labels[(labels == 3) | (labels == 7)] = 1
    gout = _ints(g, (m,), -2, 2)
    w[:, XENT_J], x[:, XENT_J] = 1.0, x[:, XENT_J].clamp_min(1.0)
    w[0, XENT_J + 1], w[1, XENT_J + 1], w[2, XENT_J + 1] = 1.0, -1.0, 0.0
    x[6], x[31] = 0.0, 0.0
    x[6, XENT_J], x[31, XENT_J] = 1.0, 1.0  # the all-ones column shifts every class alike
    v = KINDS[kind]
    if where == "x":
        x[4, XENT_J], x[20, XENT_J + 1] = v, v
    elif where == "w":
        w[3, XENT_J] = v
    elif where == "b":
        b[7] = v
    else:
        gout[6], gout[31] = v, v
    return x, w, b, labels, gout


def xent_b_bounds(x, w, b, labels, gout):
    """test_dense_xent_gpu.py's bounds for the finite outputs: a class whose logit is -inf in every row adds exactly 0
    to every sum and never holds the maximum, so the bounds are those of the problem without it (its dw row and db
    entry are exactly 0); a special in one row of x or gout leaves the other rows' bounds as they are, so they are
    computed with that special set to 0.  Outputs that are not finite in the reference have no bound."""
    from test_dense_xent_gpu import _reference

    n = w.shape[0]
    gone = ((w == -INF).any(1) | (b == -INF)).nonzero().flatten().tolist()
    keep = [c for c in range(n) if c not in gone]
    fin = lambda t: torch.where(t.isfinite(), t, torch.zeros_like(t))  # noqa: E731
    remap = torch.full((n,), -1, dtype=I64)
    remap[keep] = torch.arange(len(keep))
    assert bool((remap[labels] >= 0).all())
    _, bounds = _reference(fin(x), fin(w)[keep], fin(b)[keep], remap[labels], fin(gout))
    e_dw, e_db = torch.zeros(n, x.shape[1], dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    e_dw[keep], e_db[keep] = bounds[3], bounds[4]
    return [bounds[0], None, bounds[2], e_dw, e_db]


def _row_kinds(z):
    return {"+inf": bool((z == INF).any(1).any()), "only -inf": bool((z == -INF).all(1).any()),
            "one -inf": bool((((z == -INF).sum(1) == 1) & (z.isfinite().sum(1) == z.shape[1] - 1)).any()),
            "nan": bool(z.isnan().any(1).any())}


@pytest.mark.parametrize("kind,where", B_CASES)
def test_b_dense_xent(cuda, kind, where):
    """Pinned difference, an INFINITE gout: torch's log_softmax backward forms grad - exp(logp) * sum(grad), which at
    the label's class is -inf + inf = NaN; the kernel forms gout * (p - onehot), the line both dense_xent.hip and
    ops.cross_entropy state, which is -inf * (1 - p) = an infinity there.  No defect: for those two cases the
    reference is that line in float64 (xent_reference(explicit_d=True)); every other case is torch's autograd."""
    from tony_amd.ops.dense_xent import _DenseXent, dense_xent

    x, w, b, labels, gout = xent_b_inputs(kind, where)
    want = xent_reference(x, w, b, labels, gout, explicit_d=(where == "dy" and kind != "nan"))
    seen = _row_kinds(want[1])
    expect = {("nan", "x"): "nan", ("+inf", "x"): "+inf", ("-inf", "x"): "only -inf", ("-inf", "w"): "one -inf",
              ("-inf", "b"): "one -inf", ("+inf", "w"): "+inf", ("+inf", "b"): "+inf", ("nan", "w"): "nan",
              ("nan", "b"): "nan"}.get((kind, where))
    assert expect is None or seen[expect], (expect, seen)
    bounds = xent_b_bounds(x, w, b, labels, gout)
    xg, wg, bg = (t.to(cuda).requires_grad_() for t in (x, w, b))
    loss, logits = dense_xent(xg, wg, bg, labels.to(cuda), reduction="none", return_logits=True)
    assert isinstance(loss.grad_fn, _DenseXent._backward_cls)
    loss.backward(gout.to(cuda))
    got = [loss.detach(), logits, xg.grad, wg.grad, bg.grad]
    for name, a, r, bound in zip(("loss", "logits", "dx", "dw", "db"), got, want, bounds):
        assert_same_specials(a.cpu(), r, name, bound)


# ---------------------------------------------------------------------------------------------------------------------
# C: refusals write nothing; the Python predicates on the GPU
# ---------------------------------------------------------------------------------------------------------------------

BIG = 2 ** 31


def _conv_base(dev, cin, cout, pooled):
    """Valid guarded buffers of one small case (k = 3, p = 1, 2 x 6 x 6): inputs dict, destinations dict."""
    n, h, w, k = 2, 6, 6, 3
    ph = 3 if pooled else 6
    f = lambda *s: torch.zeros(*s)  # noqa: E731
    ins = {"x": guarded(f(n, cin, h, w), dev), "w": guarded(f(cout, cin, k, k), dev), "b": guarded(f(cout), dev),
           "dy": guarded(f(n, cout, ph, ph), dev), "ysaved": guarded(f(n, cout, ph, ph), dev),
           "idxsaved": _idx_in(torch.zeros(n, cout, ph, ph, dtype=U8), dev),
           "part_in": guarded(f(1 * (k * k * cout * cin + cout) if cin > 1 else 32 * 32), dev)}
    outs = {"y": _out(n * cout * ph * ph, dev), "idx": _out(n * cout * ph * ph, dev, dtype=U8),
            "dx": _out(n * cin * h * w, dev), "part": _out(k * k * cout * cin + cout if cin > 1 else 32 * 32, dev),
            "dw": _out(cout * cin * k * k, dev), "db": _out(cout, dev)}
    return ins, outs, [n, h, w, k, 1]


# geometry mutations of (N, H, W, k, pad) and their codes, read from each make_geo
GEO_COMMON = [((2, 6, 6, 4, 1), -2), ((2, 6, 6, 3, 2), -3), ((0, 6, 6, 3, 1), -4)]
GEO = {
    "conv1": GEO_COMMON + [((2, 2, 6, 3, 1), -4), ((2, 6, 2, 3, 1), -4), ((BIG, 3, 3, 3, 0), -5)],
    "conv1_pool": GEO_COMMON + [((2, 2, 6, 3, 1), -4), ((2, 3, 6, 3, 0), -4), ((2, 6, 3, 3, 0), -4),
                                ((BIG, 4, 4, 3, 0), -5)],
    "conv2": GEO_COMMON + [((2, 3, 6, 3, 0), -4), ((2, 6, 3, 3, 0), -4), ((2, 6, 63, 3, 1), -4), ((2, 6, 65, 3, 0), -4),
                           ((2, 0, 6, 3, 1), -4), ((BIG, 4, 4, 3, 0), -5)],
}


def _refusals(dev, name, args, outs, cases, nullable=()):
    """Every pointer of ``args`` nulled in turn (-1) and every (position, value, code) of ``cases``: the code, and
    all of ``outs`` untouched."""
    todo = [(i, None, -1) for i, a in enumerate(args) if hasattr(a, "ptr") and i not in nullable] + list(cases)
    for pos, value, rc in todo:
        changed = list(args)
        if isinstance(pos, tuple):
            for q, v in zip(pos, value):
                changed[q] = v
        else:
            changed[pos] = value
        _call(dev, name, *changed, rc=rc)
    torch.cuda.synchronize()
    for what, s in outs.items():
        assert bool((s.alloc == s.fill).all()), f"{name}: a refused call wrote to {what}"


def _geo_cases(fam, first):
    pos = tuple(range(first, first + 5))
    return [(pos, geo, rc) for geo, rc in GEO[fam]]


CONV_ENTRIES = {
    "tony_conv1_fwd": ("conv1", 1, 32, False, ["x", "w", "b", "y"]),
    "tony_conv1_bwd": ("conv1", 1, 32, False, ["dy", "ysaved", "x", "part"]),
    "tony_conv1_pool_fwd": ("conv1_pool", 1, 32, True, ["x", "w", "b", "y", "idx"]),
    "tony_conv1_pool_bwd": ("conv1_pool", 1, 32, True, ["dy", "ysaved", "idxsaved", "x", "part"]),
    "tony_conv2_fwd": ("conv2", 32, 64, True, ["x", "w", "b", "y", "idx"]),
    "tony_conv2_dgrad": ("conv2", 32, 64, True, ["dy", "ysaved", "idxsaved", "w", "dx"]),
    "tony_conv2_wgrad": ("conv2", 32, 64, True, ["dy", "ysaved", "idxsaved", "x", "part"]),
}


@pytest.mark.parametrize("name", sorted(CONV_ENTRIES))
def test_c_conv_refusals(cuda, name):
    fam, cin, cout, pooled, ptrs = CONV_ENTRIES[name]
    ins, outs, geo = _conv_base(cuda, cin, cout, pooled)
    args = [ins.get(q, outs.get(q)) for q in ptrs] + geo
    _refusals(cuda, name, args, outs, _geo_cases(fam, len(ptrs)))


@pytest.mark.parametrize("name,cin,cout", [("tony_conv1_fold", 1, 32), ("tony_conv2_fold", 32, 64)])
def test_c_fold_refusals(cuda, name, cin, cout):
    ins, outs, _ = _conv_base(cuda, cin, cout, True)
    _refusals(cuda, name, [ins["part_in"], 1, 3, outs["dw"], outs["db"]], outs, [(1, 0, -1), (2, 4, -2)])


def _dense_base(dev, m=4, n=3, k=8):
    f = lambda *s: torch.zeros(*s)  # noqa: E731
    ins = {"x": guarded(f(m, k), dev), "w": guarded(f(n, k), dev), "b": guarded(f(n), dev), "dy": guarded(f(m, n), dev),
           "ysaved": guarded(f(m, n), dev), "part_in": guarded(f(2 * m * n), dev),
           "labels": guarded(torch.zeros(m, dtype=I64), dev, fill=-1), "gout": guarded(f(m), dev),
           "logits_in": guarded(f(m, n), dev), "lse_in": guarded(f(m), dev)}
    outs = {"y": _out(m * n, dev), "part": _out(2 * m * n, dev), "dx": _out(m * k, dev), "dw": _out(n * k, dev),
            "db": _out(n, dev), "logits": _out(m * n, dev), "lse": _out(m, dev), "loss": _out(m, dev)}
    assert ins["x"].ptr() % 16 == 0 and ins["w"].ptr() % 16 == 0
    return ins, outs


# (M, N, K) outside dense.hip's make_shape: -2 the form, -3 a product of two of them at 2^31
DENSE_SHAPES_BAD = [((0, 3, 8), -2), ((4, 0, 8), -2), ((4, 3, 0), -2), ((4, 3, 6), -2), ((BIG, 3, 8), -3),
                    ((2 ** 29, 3, 8), -3), ((4, 2 ** 29, 8), -3)]


def test_c_dense_fwd_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["x"], ins["w"], ins["b"], outs["y"], outs["part"], 4, 3, 8, 1]
    cases = [((5, 6, 7), mnk, rc) for mnk, rc in DENSE_SHAPES_BAD]
    cases += [(0, ins["x"].ptr() + 4, -4), (1, ins["w"].ptr() + 4, -4)]  # checked before the launch (dense.hip:326)
    _refusals(cuda, "tony_dense_fwd", args, outs, cases, nullable=(4,))
    # a split shape without its partials: -1, after the shape and the alignment passed and before the launch
    m, n, k = 3, 33, 2500
    x, w, y = guarded(torch.zeros(m, k), cuda), guarded(torch.zeros(n, k), cuda), _out(m * n, cuda)
    assert _L().lib().tony_dense_splits(m, n, k) > 1
    _call(cuda, "tony_dense_fwd", x, w, guarded(torch.zeros(n), cuda), y, None, m, n, k, 1, rc=-1)
    torch.cuda.synchronize()
    assert bool((y.alloc == SENT).all())


def test_c_dense_fold_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["part_in"], ins["b"], outs["y"], 2, 4, 3, 1]
    cases = [(3, 0, -2), (4, 0, -2), (5, 0, -2), ((4, 5), (2 ** 16, 2 ** 15), -2)]
    _refusals(cuda, "tony_dense_fold", args, outs, cases)


def test_c_dense_dgrad_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["dy"], ins["ysaved"], ins["w"], outs["dx"], 4, 3, 8, 1]  # relu = 1: y may not be null
    _refusals(cuda, "tony_dense_dgrad", args, outs, [((4, 5, 6), mnk, rc) for mnk, rc in DENSE_SHAPES_BAD])


def test_c_dense_wgrad_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["dy"], ins["ysaved"], ins["x"], outs["dw"], outs["db"], 4, 3, 8, 1]
    _refusals(cuda, "tony_dense_wgrad", args, outs, [((5, 6, 7), mnk, rc) for mnk, rc in DENSE_SHAPES_BAD])


# (M, N, K) outside dense_xent.hip's check_form
XENT_SHAPES_BAD = [((4, 33, 8), -2), ((4, 3, 6), -2), ((4, 3, 0), -2), ((0, 3, 8), -2), ((4, 0, 8), -2),
                   ((2 ** 28, 3, 8), -3)]


def test_c_dense_xent_fwd_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["x"], ins["w"], ins["b"], ins["labels"], outs["logits"], outs["lse"], outs["loss"], 4, 3, 8]
    cases = [((7, 8, 9), mnk, rc) for mnk, rc in XENT_SHAPES_BAD]
    cases += [(0, ins["x"].ptr() + 4, -4), (1, ins["w"].ptr() + 4, -4)]  # check_form precedes the launch
    _refusals(cuda, "tony_dense_xent_fwd", args, outs, cases)


def test_c_dense_xent_bwd_refusals(cuda):
    ins, outs = _dense_base(cuda)
    args = [ins["gout"], 1, ins["logits_in"], ins["lse_in"], ins["labels"], ins["x"], ins["w"], outs["dx"], outs["dw"],
            outs["db"], 4, 3, 8]
    cases = [((10, 11, 12), mnk, rc) for mnk, rc in XENT_SHAPES_BAD]
    cases += [(1, 2, -2), (1, -1, -2), (5, ins["x"].ptr() + 4, -4), (6, ins["w"].ptr() + 4, -4)]
    _refusals(cuda, "tony_dense_xent_bwd", args, outs, cases, nullable=(7,))  # a null dx means: not asked for


def test_c_queries_refuse_with_zero(cuda):
    for name in ("tony_conv1_bwd_grid", "tony_conv1_pool_bwd_grid", "tony_conv2_wgrad_grid"):
        assert getattr(_L().lib(), name)(0) == 0 and getattr(_L().lib(), name)(BIG) == 0
    assert _L().lib().tony_dense_splits(4, 3, 6) == 0 and _L().lib().tony_dense_splits(0, 3, 8) == 0


def _composition_dense(x, w, b, relu):
    y = F.linear(x, w, b)
    return F.relu(y) if relu else y


def _off_form_dense(dev):
    """(what, x, w) off dense's native form: 4-byte-offset contiguous views, a non-contiguous x, K % 4 != 0."""
    g = torch.Generator().manual_seed(5)
    m, n, k = 33, 10, 36
    x, w = torch.randn(m, k, generator=g).to(dev), torch.randn(n, k, generator=g).to(dev)
    xbuf, wbuf = torch.zeros(m * k + 8, device=dev), torch.zeros(n * k + 8, device=dev)
    xo, wo = xbuf[1:1 + m * k].view(m, k), wbuf[1:1 + n * k].view(n, k)
    xo.copy_(x), wo.copy_(w)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4 and wo.data_ptr() % 16 == 4
    xt = torch.randn(k, m, generator=g).to(dev).t()
    return [("x at +4 bytes", xo, w), ("w at +4 bytes", x, wo), ("a non-contiguous x", xt, w),
            ("K % 4 != 0", x[:, :34].contiguous(), w[:, :34].contiguous())]


def test_c_dense_predicate_on_gpu(cuda):
    from tony_amd.ops.dense import _Dense, dense

    b = torch.randn(10, generator=torch.Generator().manual_seed(6)).to(cuda).requires_grad_()
    for what, x, w in _off_form_dense(cuda):
        for relu in (False, True):
            y = dense(x, w, b, relu)
            assert not isinstance(y.grad_fn, _Dense._backward_cls), what
            assert_equal(y.detach().cpu(), _composition_dense(x, w, b, relu).detach().cpu(), what)
    _, x, w = _off_form_dense(cuda)[0]
    x = x.clone()  # aligned: only autocast keeps it off the kernels
    assert isinstance(dense(x, w.clone(), b).grad_fn, _Dense._backward_cls)
    with torch.autocast("cuda", torch.bfloat16):
        y, want = dense(x, w.clone(), b, True), _composition_dense(x, w.clone(), b, True)
    assert not isinstance(y.grad_fn, _Dense._backward_cls) and y.dtype == torch.bfloat16
    assert_equal(y.detach().cpu(), want.detach().cpu(), "under autocast")


def test_c_dense_xent_predicate_on_gpu(cuda):
    from tony_amd.ops.dense import dense
    from tony_amd.ops.dense_xent import _DenseXent, dense_xent
    from tony_amd.ops.loss import cross_entropy

    g = torch.Generator().manual_seed(7)
    b = torch.randn(10, generator=g).to(cuda).requires_grad_()
    labels = torch.randint(0, 10, (33,), generator=g).to(cuda)

    def check(what, x, w, b, autocast=False):
        with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
            loss, logits = dense_xent(x, w, b, labels, reduction="none", return_logits=True)
            z = dense(x, w, b)
            want = cross_entropy(z, labels, reduction="none")
        assert not isinstance(loss.grad_fn, _DenseXent._backward_cls), what
        assert_equal(loss.detach().cpu(), want.detach().cpu(), what + ": loss")
        assert_equal(logits.cpu(), z.detach().cpu(), what + ": logits")

    for what, x, w in _off_form_dense(cuda):
        check(what, x, w, b)
    x = torch.randn(33, 36, generator=g).to(cuda)
    w33 = torch.randn(33, 36, generator=g).to(cuda).requires_grad_()
    check("N = 33", x, w33, torch.randn(33, generator=g).to(cuda))
    w = torch.randn(10, 36, generator=g).to(cuda).requires_grad_()
    assert isinstance(dense_xent(x, w, b, labels, "none").grad_fn, _DenseXent._backward_cls)
    check("under autocast", x, w, b, autocast=True)


def test_c_conv_predicates_on_gpu(cuda):
    from tony_amd.ops.conv1 import _Conv1BiasReLU, _Conv1BiasReLUPool, conv1_bias_relu
    from tony_amd.ops.conv2 import _Conv2BiasReLUPool, conv2_bias_relu_pool

    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g).to(cuda)  # noqa: E731
    x1, w3, w5, b1 = r(2, 1, 8, 9), r(32, 1, 3, 3).requires_grad_(), r(32, 1, 5, 5).requires_grad_(), r(32).requires_grad_()
    for pool, cls in ((False, _Conv1BiasReLU), (True, _Conv1BiasReLUPool)):
        comp = lambda x, w, p: (F.max_pool2d(F.relu(F.conv2d(x, w, b1, padding=p)), 2) if pool  # noqa: E731
                                else F.relu(F.conv2d(x, w, b1, padding=p)))
        assert isinstance(conv1_bias_relu(x1, w3, b1, 1, pool).grad_fn, cls._backward_cls)
        for what, x, w, p in (("an image that requires grad", x1.clone().requires_grad_(), w3, 1),
                              ("padding 1 with k = 5", x1, w5, 1)):
            y = conv1_bias_relu(x, w, b1, p, pool)
            assert not isinstance(y.grad_fn, cls._backward_cls), what
            assert_equal(y.detach().cpu(), comp(x, w, p).detach().cpu(), what)
        with torch.autocast("cuda", torch.bfloat16):
            y, want = conv1_bias_relu(x1, w3, b1, 1, pool), comp(x1, w3, 1)
        # conv1 does not consult autocast today: the kernels and fp32 where the composition gives bf16
        assert isinstance(y.grad_fn, cls._backward_cls) and y.dtype == F32 and want.dtype == torch.bfloat16
    w2, b2 = r(64, 32, 3, 3).requires_grad_(), r(64).requires_grad_()
    comp2 = lambda x: F.max_pool2d(F.relu(F.conv2d(x, w2, b2, padding=1)), 2)  # noqa: E731
    x2, wide = r(1, 32, 6, 62), r(1, 32, 6, 63)
    assert isinstance(conv2_bias_relu_pool(x2, w2, b2, 1).grad_fn, _Conv2BiasReLUPool._backward_cls)
    y = conv2_bias_relu_pool(wide, w2, b2, 1)
    assert not isinstance(y.grad_fn, _Conv2BiasReLUPool._backward_cls)
    assert_equal(y.detach().cpu(), comp2(wide).detach().cpu(), "W + 2p = 65")
    with torch.autocast("cuda", torch.bfloat16):
        y, want = conv2_bias_relu_pool(x2, w2, b2, 1), comp2(x2)
    # conv2 does not consult autocast today either
    assert isinstance(y.grad_fn, _Conv2BiasReLUPool._backward_cls) and y.dtype == F32 and want.dtype == torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# D: dense_xent's gout branches
# ---------------------------------------------------------------------------------------------------------------------

def _d_inputs():
    from test_dense_xent_gpu import _inputs

    x, w, b, y, gout = _inputs((33, 10, 36), False)
    y[[0, 7, 32]] = torch.tensor([-100, 10, -100])
    return x, w, b, y, gout


def _xent_grads(dev, x, w, b, y, backward):
    """(dx, dw, db) on the GPU after ``backward(per-row loss or reduced loss, op)``."""
    from tony_amd.ops.dense_xent import dense_xent

    xg, wg, bg = (t.to(dev).requires_grad_() for t in (x, w, b))
    backward(lambda reduction: dense_xent(xg, wg, bg, y.to(dev), reduction=reduction))
    return [t.grad.cpu() for t in (xg, wg, bg)]


def _native_node(loss):
    from tony_amd.ops.dense_xent import _DenseXent

    node = loss.grad_fn
    while node is not None and not isinstance(node, _DenseXent._backward_cls):
        node = node.next_functions[0][0] if node.next_functions else None
    return node is not None


def within_bounds(got, want, bounds, what):
    """Each of (dx, dw, db) within its bound of the float64 reference; prints the worst error / bound."""
    for name, a, r, bound in zip(("dx", "dw", "db"), got, want, bounds):
        e = (a.double() - r).abs()
        print(f"{what} {name}: worst error / bound {float((e / bound.clamp_min(1e-300)).max()):.3f}")
        assert a.shape == r.shape and bool((e <= bound).all()), f"{what} {name}"


def test_d_sum_and_mean(cuda):
    """reduction="sum": SumBackward expands one value, which _DenseXent.backward hands to the kernel with stride 0;
    "mean": a stride-1 gout of 1/33 rounded to fp32.  Worst error / bound on an MI355X, 33x10x36 with rows 0, 7, 32
    ignored: sum dx 0.019, dw 0.012, db 0.003; mean dx 0.055, dw 0.008, db 0.002 (test_d_one_row_sum, 1x10x36: dx
    0.004, dw 0.016, db 0.016)."""
    from test_dense_xent_gpu import _reference

    x, w, b, y, _ = _d_inputs()

    def run(reduction):
        def go(op):
            loss = op(reduction)
            assert _native_node(loss)
            loss.backward()
        return _xent_grads(cuda, x, w, b, y, go)

    ones = torch.ones(33)
    want, bounds = _reference(x, w, b, y, ones)
    got = run("sum")
    within_bounds(got, want[2:], bounds[2:], "sum")
    per_row = _xent_grads(cuda, x, w, b, y, lambda op: op("none").backward(ones.to(cuda)))
    for name, a, r in zip(("dx", "dw", "db"), got, per_row):
        assert_equal(a, r, f"sum against none + ones: {name}")
    third = (torch.ones((), dtype=F32) / 33).expand(33)
    want, bounds = _reference(x, w, b, y, third)
    within_bounds(run("mean"), want[2:], bounds[2:], "mean")


def test_d_recast_gout(cuda):
    """A float64 gout and a stride-2 fp32 gout give the bits of the contiguous fp32 gout of the same values."""
    x, w, b, y, gout = _d_inputs()
    plain = _xent_grads(cuda, x, w, b, y, lambda op: op("none").backward(gout.to(cuda)))
    g64 = gout.double().to(cuda)
    as64 = _xent_grads(cuda, x, w, b, y, lambda op: (op("none").double() * g64).sum().backward())
    buf = torch.zeros(66)
    buf[::2] = gout

    class Strided(torch.autograd.Function):
        @staticmethod
        def forward(ctx, loss):
            return loss.sum()

        @staticmethod
        def backward(ctx, g):
            out = buf.to(cuda)[::2]
            assert out.stride(0) == 2
            return out

    strided = _xent_grads(cuda, x, w, b, y, lambda op: Strided.apply(op("none")).backward())
    for name, p, a, s in zip(("dx", "dw", "db"), plain, as64, strided):
        assert_equal(a, p, f"float64 gout: {name}")
        assert_equal(s, p, f"stride-2 gout: {name}")


def test_d_one_row_sum(cuda):
    """M = 1: an expanded gout of one row has stride 0 or 1 at torch's whim; the wrapper passes stride 1."""
    from test_dense_xent_gpu import _inputs, _reference

    x, w, b, y, _ = _inputs((1, 10, 36), False)
    want, bounds = _reference(x, w, b, y, torch.ones(1))
    got = _xent_grads(cuda, x, w, b, y, lambda op: op("sum").backward())
    within_bounds(got, want[2:], bounds[2:], "M = 1 sum")
    per_row = _xent_grads(cuda, x, w, b, y, lambda op: op("none").backward(torch.ones(1, device=cuda)))
    for name, a, r in zip(("dx", "dw", "db"), got, per_row):
        assert_equal(a, r, f"M = 1: {name}")


# ---------------------------------------------------------------------------------------------------------------------
# E
# ---------------------------------------------------------------------------------------------------------------------

def test_zz_every_entry_point_ran(cuda):
    """Every tony_conv1_* / tony_conv2_* / tony_dense_* entry point of _lib._SIGNATURES ran with code 0 in part A and,
    if it takes a pointer, was refused in part C (the module run as a whole): a later one cannot arrive untested."""
    import ctypes

    sigs = _L()._SIGNATURES
    names = sorted(n for n in sigs if n.startswith(("tony_conv1_", "tony_conv2_", "tony_dense_")))
    assert len(names) == 19
    missing = [n for n in names if n not in _RAN]
    assert not missing, f"entry points no case of part A ran: {missing}"
    unrefused = [n for n in names if ctypes.c_void_p in sigs[n][:-1] and n not in _REFUSED]
    assert not unrefused, f"entry points no case of part C refused: {unrefused}"
