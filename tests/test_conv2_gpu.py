"""ops.conv2 on the GPU (csrc/conv2.hip) against float64: exact on integers, within counted roundings on normal
inputs, and the same bits on every backward.

Shapes per (k, p): one pooled pixel (p = 0) or a one-band plane; odd, non-square sizes whose last conv row and / or
column is dropped; deepnn's 14x14 (49 pooled pixels, no multiple of the 32-pixel tile); hvd_cnn's 26x26 (several
bands); a tall plane (many bands sharing halo rows); the widest plane of the form; and 5 images of 14x14, more than a
weight-gradient workgroup's slice of 2 images (kWgImages) and not a multiple of it.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

M = 5
CASES = [(k, p, nhw) for k in (3, 5) for p in (0, (k - 1) // 2)
         for nhw in ((1, k + 1, k + 1), (2, 9, 11), (3, 14, 14), (2, 26, 26), (1, 40, 12), (1, 8, 64 - 2 * p),
                     (M, 14, 14))]
U = 2.0 ** -24


def _inputs(k, p, nhw, integers):
    g = torch.Generator().manual_seed(k * 1000 + 10 * p + sum(nhw))
    n, h, w = nhw
    shapes = [(n, 32, h, w), (64, 32, k, k), (64,), (n, 64, (h + 2 * p - k + 1) // 2, (w + 2 * p - k + 1) // 2)]
    if integers:
        return [torch.randint(lo, hi + 1, s, generator=g).float() for s, (lo, hi) in
                zip(shapes, ((0, 3), (-2, 2), (-4, 4), (-2, 2)))]
    return [torch.randn(s, generator=g) for s in shapes]


def _run(x, wt, b, p, dy, dev):
    from tony_amd.ops.conv2 import _Conv2BiasReLUPool, conv2_bias_relu_pool

    x, wt, b = (t.to(dev).requires_grad_() for t in (x, wt, b))
    y = conv2_bias_relu_pool(x, wt, b, p)
    assert isinstance(y.grad_fn, _Conv2BiasReLUPool._backward_cls)  # the kernels, not the composition
    return [t.detach().cpu().double() for t in (y, *torch.autograd.grad(y, (x, wt, b), dy.to(dev)))]


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_exact_on_integers(cuda, k, p, nhw):
    x, wt, b, dy = _inputs(k, p, nhw, True)
    y, dx, dw, db = _run(x, wt, b, p, dy, cuda)
    xr, wr, br = (t.double().requires_grad_() for t in (x, wt, b))
    yr = F.max_pool2d(F.relu(F.conv2d(xr, wr, br, padding=p)), 2)
    assert y.shape == yr.shape and torch.equal(y, yr.detach())
    for got, want in zip((dx, dw, db), torch.autograd.grad(yr, (xr, wr, br), dy.double())):
        assert torch.equal(got, want)


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_rounding_on_normals(cuda, k, p, nhw):
    from tony_amd.ops.conv2 import _forward

    x, wt, b, dy = _inputs(k, p, nhw, False)
    y, dx, dw, db = _run(x, wt, b, p, dy, cuda)
    xd, wd, bd = x.double(), wt.double(), b.double()
    K = 32 * k * k
    bound = F.max_pool2d((K + 3) * U * (bd.abs().view(1, 64, 1, 1) + F.conv2d(xd.abs(), wd.abs(), padding=p)), 2)
    err = (y - F.max_pool2d(F.relu(F.conv2d(xd, wd, bd, padding=p)), 2)).abs()
    print(f"forward: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # dY' through the kernel's own y > 0 and idx: a maximum or a sign flipped by rounding is the forward's matter
    yk, idx = (t.cpu() for t in _forward(x.to(cuda), wt.to(cuda), b.to(cuda), p))
    assert torch.equal(yk.double(), y) and int(idx.max()) <= 3
    n, _, ph, pw = y.shape
    oh, ow = x.shape[2] + 2 * p - k + 1, x.shape[3] + 2 * p - k + 1
    dyp = torch.zeros(n, 64, oh, ow, dtype=torch.float64)
    for pos in range(4):
        dyp[:, :, pos // 2:2 * ph:2, pos % 2:2 * pw:2] = torch.where((idx == pos) & (yk > 0), dy.double(), 0.0)
    cols, d = F.unfold(xd, k, padding=p), dyp.flatten(2)                     # [N, 32*k*k, L], [N, 64, L]
    L = n * oh * ow
    checks = [("dX", dx, F.conv_transpose2d(dyp, wd, padding=p), F.conv_transpose2d(dyp.abs(), wd.abs(), padding=p),
               64 * k * k + 2),
              ("dW", dw, torch.einsum("ncl,ntl->ct", d, cols).view_as(wd),
               torch.einsum("ncl,ntl->ct", d.abs(), cols.abs()).view_as(wd), L + 2),
              ("db", db, d.sum((0, 2)), d.abs().sum((0, 2)), L + 2)]
    for name, got, ref, mag, count in checks:
        e = (got - ref).abs()
        print(f"{name}: worst error / bound {float((e / (count * U * mag).clamp_min(1e-300)).max()):.3f}")
        assert bool((e <= count * U * mag).all()), name


@pytest.mark.parametrize("k,p", [(3, 0), (5, 2)])
def test_backward_same_bits(cuda, k, p):
    from tony_amd.ops.conv2 import conv2_bias_relu_pool

    x, wt, b, dy = (t.to(cuda) for t in _inputs(k, p, (M, 14, 14), False))
    x, wt, b = x.requires_grad_(), wt.requires_grad_(), b.requires_grad_()
    y = conv2_bias_relu_pool(x, wt, b, p)
    first = torch.autograd.grad(y, (x, wt, b), dy, retain_graph=True)
    again = torch.autograd.grad(y, (x, wt, b), dy)
    assert all(torch.equal(f, a) for f, a in zip(first, again))
