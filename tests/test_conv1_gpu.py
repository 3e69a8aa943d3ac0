"""ops.conv1 on the GPU (csrc/conv1.hip) against float64: exact on integers, within counted roundings on normal
inputs, and the same bits on every backward.

Shapes: one output pixel at padding 0; odd, non-square sizes; a pixel count that is no multiple of the 32-pixel MFMA
tile; 131 images, more than a backward workgroup's slice of 2 and not a multiple of it (130 would be); and a plane
wider than a 256-pixel tile, so the column chunks run.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [(k, p, nhw) for k in (3, 5) for p in (0, (k - 1) // 2)
         for nhw in ((1, k, k), (2, 7, 9), (3, 28, 28), (131, 28, 28), (1, 6, 300))]
U = 2.0 ** -24


def _inputs(k, p, nhw, integers, dev):
    g = torch.Generator().manual_seed(k * 1000 + sum(nhw))
    n, h, w = nhw
    shapes = [(n, 1, h, w), (32, 1, k, k), (32,), (n, 32, h + 2 * p - k + 1, w + 2 * p - k + 1)]
    if integers:
        ts = [torch.randint(lo, hi + 1, s, generator=g).float() for s, (lo, hi) in
              zip(shapes, ((0, 3), (-2, 2), (-4, 4), (-2, 2)))]
    else:
        ts = [torch.randn(s, generator=g) for s in shapes]
    x, wt, b, dy = (t.to(dev) for t in ts)
    return x, wt.requires_grad_(), b.requires_grad_(), dy


def _run(x, wt, b, p, dy):
    from tony_amd.ops.conv1 import _Conv1BiasReLU, conv1_bias_relu

    y = conv1_bias_relu(x, wt, b, p)
    assert isinstance(y.grad_fn, _Conv1BiasReLU._backward_cls)  # the kernels, not the composition
    dw, db = torch.autograd.grad(y, (wt, b), dy)
    return y.detach(), dw, db


def _ref_bwd(x, mask, dy, k, p):
    """float64 dW, db and the sums of magnitudes behind them, through the given ReLU mask."""
    d = (dy.double() * mask).flatten(2)                             # [N, 32, L]
    cols = F.unfold(x.double(), k, padding=p)                       # [N, k*k, L]
    dw, mag = torch.einsum("ncl,ntl->ct", d, cols), torch.einsum("ncl,ntl->ct", d.abs(), cols.abs())
    return dw.view(32, 1, k, k), d.sum((0, 2)), mag.view(32, 1, k, k), d.abs().sum((0, 2))


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_exact_on_integers(cuda, k, p, nhw):
    x, wt, b, dy = _inputs(k, p, nhw, True, cuda)
    y, dw, db = _run(x, wt, b, p, dy)
    yr = F.relu(F.conv2d(x.double(), wt.detach().double(), b.detach().double(), padding=p))
    assert y.shape == yr.shape and torch.equal(y.double(), yr)
    dwr, dbr, _, _ = _ref_bwd(x, yr > 0, dy, k, p)
    assert torch.equal(dw.double(), dwr) and torch.equal(db.double(), dbr)


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_rounding_on_normals(cuda, k, p, nhw):
    x, wt, b, dy = _inputs(k, p, nhw, False, cuda)
    y, dw, db = _run(x, wt, b, p, dy)
    xd, wd, bd = x.double(), wt.detach().double(), b.detach().double()
    mag = bd.abs().view(1, 32, 1, 1) + F.conv2d(xd.abs(), wd.abs(), padding=p)
    err = (y.double() - F.relu(F.conv2d(xd, wd, bd, padding=p))).abs()
    print(f"forward: worst error / bound {float((err / ((k * k + 3) * U * mag)).max()):.3f}")
    assert bool((err <= (k * k + 3) * U * mag).all())
    # the mask of the kernel's own y: a sign flipped at 0 by rounding is the forward's matter, checked above
    dwr, dbr, mw, mb = _ref_bwd(x, y > 0, dy, k, p)
    L = y.numel() // 32
    ew, eb = (dw.double() - dwr).abs(), (db.double() - dbr).abs()
    print(f"backward: worst error / bound dW {float((ew / ((L + 2) * U * mw).clamp_min(1e-300)).max()):.3f} "
          f"db {float((eb / ((L + 2) * U * mb).clamp_min(1e-300)).max()):.3f}")
    assert bool((ew <= (L + 2) * U * mw).all()) and bool((eb <= (L + 2) * U * mb).all())


@pytest.mark.parametrize("k,p", [(3, 0), (5, 2)])
def test_backward_same_bits(cuda, k, p):
    from tony_amd.ops.conv1 import conv1_bias_relu

    x, wt, b, dy = _inputs(k, p, (131, 28, 28), False, cuda)
    y = conv1_bias_relu(x, wt, b, p)
    first = torch.autograd.grad(y, (wt, b), dy, retain_graph=True)
    again = torch.autograd.grad(y, (wt, b), dy)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
