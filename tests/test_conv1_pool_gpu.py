"""ops.conv1 with pool=True on the GPU (csrc/conv1_pool.hip) against float64: exact on integers, within counted
roundings on normal inputs, and the same bits on every backward.

Shapes per (k, p): one pooled pixel at padding 0; odd conv sizes whose last column (2, 8, 11) or row (2, 9, 8) is
dropped; deepnn's 28x28 (196 pooled pixels in two tiles of 98, no multiple of the 32-pixel MFMA tile); 131 images,
more than a backward workgroup's slice of 2 and not a multiple of it; and a pooled row of 298 / 299 pixels, wider than
a 128-pixel tile, so the column chunks run.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [(k, p, nhw) for k in (3, 5) for p in (0, (k - 1) // 2)
         for nhw in ((1, k + 1, k + 1), (2, 8, 11), (2, 9, 8), (3, 28, 28), (131, 28, 28), (1, 6, 600))]
U = 2.0 ** -24


def _inputs(k, p, nhw, integers, dev):
    g = torch.Generator().manual_seed(k * 1000 + 10 * p + sum(nhw))
    n, h, w = nhw
    shapes = [(n, 1, h, w), (32, 1, k, k), (32,), (n, 32, (h + 2 * p - k + 1) // 2, (w + 2 * p - k + 1) // 2)]
    if integers:
        ts = [torch.randint(lo, hi + 1, s, generator=g).float() for s, (lo, hi) in
              zip(shapes, ((0, 3), (-2, 2), (-4, 4), (-2, 2)))]
    else:
        ts = [torch.randn(s, generator=g) for s in shapes]
    x, wt, b, dy = (t.to(dev) for t in ts)
    return x, wt.requires_grad_(), b.requires_grad_(), dy


def _run(x, wt, b, p, dy):
    from tony_amd.ops.conv1 import _Conv1BiasReLUPool, conv1_bias_relu

    y = conv1_bias_relu(x, wt, b, p, pool=True)
    assert isinstance(y.grad_fn, _Conv1BiasReLUPool._backward_cls)  # the kernels, not the composition
    dw, db = torch.autograd.grad(y, (wt, b), dy)
    return y.detach(), dw, db


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_exact_on_integers(cuda, k, p, nhw):
    x, wt, b, dy = _inputs(k, p, nhw, True, cuda)
    y, dw, db = _run(x, wt, b, p, dy)
    wr, br = wt.detach().double().requires_grad_(), b.detach().double().requires_grad_()
    yr = F.max_pool2d(F.relu(F.conv2d(x.double(), wr, br, padding=p)), 2)
    assert y.shape == yr.shape and torch.equal(y.double(), yr.detach())
    dwr, dbr = torch.autograd.grad(yr, (wr, br), dy.double())  # ties: torch's first maximum too
    assert torch.equal(dw.double(), dwr) and torch.equal(db.double(), dbr)


@pytest.mark.parametrize("k,p,nhw", CASES)
def test_rounding_on_normals(cuda, k, p, nhw):
    from tony_amd.ops.conv1 import _forward_pool

    x, wt, b, dy = _inputs(k, p, nhw, False, cuda)
    y, dw, db = _run(x, wt, b, p, dy)
    xd, wd, bd = x.double(), wt.detach().double(), b.detach().double()
    bound = F.max_pool2d((k * k + 3) * U * (bd.abs().view(1, 32, 1, 1) + F.conv2d(xd.abs(), wd.abs(), padding=p)), 2)
    err = (y.double() - F.max_pool2d(F.relu(F.conv2d(xd, wd, bd, padding=p)), 2)).abs()
    print(f"forward: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # dY' through the kernel's own y > 0 and idx: a maximum or a sign flipped by rounding is the forward's matter
    yk, idx = _forward_pool(x, wt.detach(), b.detach(), p)
    assert torch.equal(yk, y) and int(idx.max()) <= 3
    n, _, ph, pw = y.shape
    oh, ow = x.shape[2] + 2 * p - k + 1, x.shape[3] + 2 * p - k + 1
    dyp = torch.zeros(n, 32, oh, ow, dtype=torch.float64, device=cuda)
    for pos in range(4):
        dyp[:, :, pos // 2:2 * ph:2, pos % 2:2 * pw:2] = torch.where((idx == pos) & (yk > 0), dy.double(), 0.0)
    cols, d = F.unfold(xd, k, padding=p), dyp.flatten(2)                     # [N, k*k, L], [N, 32, L]
    # The count.  An element of dW is a sum of at most L = N * OH * OW products, each entering by a fused multiply-add
    # (one rounding), the chains of the four window positions, the four waves and the partials then added pairwise.
    # An addition rounds only when both operands are non-zero, so every rounding on a term's path brings at least one
    # further term in: a term passes at most as many roundings as there are terms, L, and L + 2 holds whatever the
    # order -- the count of test_conv1_gpu.py, which this kernel's shorter chains only undercut.
    L = n * oh * ow
    checks = [("dW", dw, torch.einsum("ncl,ntl->ct", d, cols), torch.einsum("ncl,ntl->ct", d.abs(), cols.abs())),
              ("db", db, d.sum((0, 2)), d.abs().sum((0, 2)))]
    for name, got, ref, mag in checks:
        e = (got.double().view_as(ref) - ref).abs()
        print(f"{name}: worst error / bound {float((e / ((L + 2) * U * mag).clamp_min(1e-300)).max()):.3f}")
        assert bool((e <= (L + 2) * U * mag).all()), name


@pytest.mark.parametrize("k,p", [(3, 0), (5, 2)])
def test_backward_same_bits(cuda, k, p):
    from tony_amd.ops.conv1 import conv1_bias_relu

    x, wt, b, dy = _inputs(k, p, (131, 28, 28), False, cuda)
    y = conv1_bias_relu(x, wt, b, p, pool=True)
    first = torch.autograd.grad(y, (wt, b), dy, retain_graph=True)
    again = torch.autograd.grad(y, (wt, b), dy)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
