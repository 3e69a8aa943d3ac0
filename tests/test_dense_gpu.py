"""ops.dense on the GPU (csrc/dense.hip) against float64: exact on integers, within counted roundings on normal
inputs, and the same bits on every run.

Shapes (M, N, K): the smallest form; ``linear``'s layer ragged in M and N; ``hvd_cnn``'s first dense layer at a few rows
(36 K slices); K = 4 x 625, ragged against the 64-wide chunk and the slices, N one past a tile (9 slices); more than
four row tiles plus a rest with one slice; and a K shorter than one chunk under N = 1024, the data gradient's
reduction over four of its 256-wide chunks.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4), (33, 10, 784), (5, 128, 9216), (3, 33, 2500), (130, 10, 128), (64, 1024, 36)]
CASES = [(relu, mnk) for relu in (False, True) for mnk in SHAPES]
U = 2.0 ** -24


def _g(n):
    return n * U / (1 - n * U)


def _inputs(mnk, integers):
    m, n, k = mnk
    g = torch.Generator().manual_seed(m * 1000003 + n * 1009 + k)
    shapes = [(m, k), (n, k), (n,), (m, n)]
    if integers:
        return [torch.randint(lo, hi + 1, s, generator=g).float() for s, (lo, hi) in
                zip(shapes, ((0, 3), (-2, 2), (-4, 4), (-2, 2)))]
    return [torch.randn(s, generator=g) for s in shapes]


def _run(x, w, b, relu, dy, dev, x_grad=True):
    from tony_amd.ops.dense import _Dense, dense

    x, w, b = x.to(dev).requires_grad_(x_grad), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = dense(x, w, b, relu)
    assert isinstance(y.grad_fn, _Dense._backward_cls)  # the kernels, not the composition
    y.backward(dy.to(dev))
    return [None if t is None else t.detach().cpu().double() for t in (y, x.grad, w.grad, b.grad)]


def _reference(x, w, b, relu, dy):
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    yr = F.linear(xr, wr, br)
    yr = F.relu(yr) if relu else yr
    return [yr.detach(), *torch.autograd.grad(yr, (xr, wr, br), dy.double())]


def test_split_k_is_covered(cuda):
    from tony_amd.ops import _lib

    assert _lib.lib().tony_dense_splits(5, 128, 9216) > 1 and _lib.lib().tony_dense_splits(3, 33, 2500) > 1
    assert _lib.lib().tony_dense_splits(130, 10, 128) == 1


@pytest.mark.parametrize("relu,mnk", CASES)
def test_exact_on_integers(cuda, relu, mnk):
    x, w, b, dy = _inputs(mnk, True)
    for name, got, want in zip(("y", "dx", "dw", "db"), _run(x, w, b, relu, dy, cuda), _reference(x, w, b, relu, dy)):
        assert got.shape == want.shape and torch.equal(got, want), name


@pytest.mark.parametrize("relu,mnk", CASES)
def test_rounding_on_normals(cuda, relu, mnk):
    m, n, k = mnk
    x, w, b, dy = _inputs(mnk, False)
    y, dx, dw, db = _run(x, w, b, relu, dy, cuda)
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = F.linear(xd, wd, bd)
    # dy' through the kernel's own y > 0: a sign flipped by rounding is the forward's matter
    d = torch.where(y > 0, dy.double(), 0.0) if relu else dy.double()
    checks = [("y", y, F.relu(ref) if relu else ref, _g(k + 2) * (bd.abs() + xd.abs() @ wd.abs().t())),
              ("dx", dx, d @ wd, _g(n + 1) * (d.abs() @ wd.abs())),
              ("dw", dw, d.t() @ xd, _g(m + 1) * (d.abs().t() @ xd.abs())),
              ("db", db, d.sum(0), _g(m) * d.abs().sum(0))]
    for name, got, want, bound in checks:
        e = (got - want).abs()
        print(f"{name}: worst error / bound {float((e / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((e <= bound).all()), name


def test_same_bits(cuda):
    from tony_amd.ops.dense import dense

    x, w, b, dy = (t.to(cuda) for t in _inputs((5, 128, 9216), False))
    x, w, b = x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    y = dense(x, w, b, True)
    assert torch.equal(y, dense(x, w, b, True))
    first = torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)
    again = torch.autograd.grad(y, (x, w, b), dy)
    assert all(torch.equal(f, a) for f, a in zip(first, again))


def test_no_dx_for_an_input_without_grad(cuda):
    x, w, b, dy = _inputs((33, 10, 784), True)
    y, dx, dw, db = _run(x, w, b, True, dy, cuda, x_grad=False)
    yr, _, dwr, dbr = _reference(x, w, b, True, dy)
    assert dx is None and torch.equal(y, yr) and torch.equal(dw, dwr) and torch.equal(db, dbr)
