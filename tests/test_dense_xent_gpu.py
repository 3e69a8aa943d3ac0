"""ops.dense_xent on the GPU (csrc/dense_xent.hip) against float64: logits exact on integers, loss / dx / dw / db within
counted roundings on normal inputs, ignored rows, the same bits on every run.

Shapes (M, N, K): the smallest form with one class (loss 0, d = 0); one row past a tile with K ragged against the
64-wide forward chunk and the 32-wide backward slice; more than four row tiles plus a rest, so the backward's
round-robin wraps; N at the cap with K shorter than a chunk; the longest head K with an N that is neither 10 nor a
power of two.

The bound is assembled from what the project states elsewhere, every magnitude in float64 next to the reference.
U = 2^-24, _g(n) = n U / (1 - n U) as in tests/test_dense_gpu.py; z the logits, p their softmax, H = lse - E_p[z].
  E_z    = _g(K + 2) (|b| + |x| |w|^T)                                  the logits (that module's bound on y)
  E_lse  = max_n E_z + U (2 + N + 3 H + 4 |lse - mx| + 2 |lse|)          lse is 1-Lipschitz in max |dz|; then the terms
           of tests/test_loss_dropout_exact_gpu.py (1 ulp assumed for the hardware exp2, 2 ulp for logf) with the N - 1
           serial additions of this kernel's sum counted as N in place of that kernel's 25
  E_loss = (1 + U) (E_lse + E_z[label]) + U |loss|                       one subtraction of two inexact operands
  E_d    = |gout| (p (expm1(E_lse + E_z + 3 U |z - lse|) + 2 U) + 2 U |p - onehot|) + 2^-125
           that docstring's E_d with the stored logits' own error in the exponent, expm1 itself for its 1.01 x (the
           exponent's error reaches 0.04 at K = 1024), and no target roundings: without smoothing the target is exact
  E_dx   = E_d |w| + _g(N + 1) ((|d| + E_d) |w|),  E_dw = E_d^T |x| + _g(M + 1) ((|d| + E_d)^T |x|),
  E_db   = sum_m E_d + _g(M) sum_m (|d| + E_d)

Worst error / bound on an MI355X (printed by test_rounding_on_normals; a record, not a knob): loss 0.007, dx 0.045,
dw 0.134, db 0.098, all at 5x32x36; below 0.01 at K = 784 and 1024, where the worst-case _g(K + 2) of the logits goes
through expm1 while the measured logits error grows like sqrt(K).  Under reduction="sum" / "mean" at 33x10x36 with three
ignored rows (tests/test_mnist_exact_gpu.py::test_d_sum_and_mean): dx 0.019 / 0.055, dw 0.012 / 0.008, db 0.003 / 0.002.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4), (33, 10, 784), (130, 10, 128), (5, 32, 36), (64, 17, 1024)]
U = 2.0 ** -24


def _g(n):
    return n * U / (1 - n * U)


def _inputs(mnk, integers):
    m, n, k = mnk
    g = torch.Generator().manual_seed(m * 1000003 + n * 1009 + k)
    shapes = [(m, k), (n, k), (n,)]
    if integers:
        x, w, b = (torch.randint(lo, hi + 1, s, generator=g).float() for s, (lo, hi) in
                   zip(shapes, ((0, 3), (-2, 2), (-4, 4))))
    else:
        x, w, b = (torch.randn(s, generator=g) for s in shapes)
    return x, w, b, torch.randint(0, n, (m,), generator=g), torch.randn(m, generator=g)


def _run(x, w, b, y, gout, dev, x_grad=True):
    from tony_amd.ops.dense_xent import _DenseXent, dense_xent

    x, w, b = x.to(dev).requires_grad_(x_grad), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    loss, logits = dense_xent(x, w, b, y.to(dev), reduction="none", return_logits=True)
    assert isinstance(loss.grad_fn, _DenseXent._backward_cls) and not logits.requires_grad  # the kernels
    loss.backward(gout.to(dev))
    return [None if t is None else t.detach().cpu().double() for t in (loss, logits, x.grad, w.grad, b.grad)]


def _reference(x, w, b, y, gout):
    """float64 (loss, logits, dx, dw, db) and their bounds; a row with a label outside [0, N) counts with gout 0."""
    (m, k), n = x.shape, w.shape[0]
    live = (y >= 0) & (y < n)
    y, gout = torch.where(live, y, 0), torch.where(live, gout, 0.0).double()
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    z = F.linear(xr, wr, br)
    loss = F.cross_entropy(z, y, reduction="none") * live
    dx, dw, db = torch.autograd.grad(loss, (xr, wr, br), gout)
    z, xa, wa = z.detach(), x.double().abs(), w.double().abs()
    lse, onehot = torch.logsumexp(z, 1, keepdim=True), F.one_hot(y, n).double()
    p = (z - lse).exp()
    e_z = _g(k + 2) * (b.double().abs() + xa @ wa.t())
    e_lse = e_z.max(1, keepdim=True).values + U * (2 + n + 3 * (lse - (p * z).sum(1, keepdim=True))
                                                   + 4 * (lse - z.max(1, keepdim=True).values) + 2 * lse.abs())
    e_loss = ((1 + U) * (e_lse + e_z.gather(1, y[:, None])) + U * (lse - z.gather(1, y[:, None])).abs())[:, 0]
    g = gout.abs()[:, None]
    e_p = p * (torch.expm1(e_lse + e_z + 3 * U * (z - lse).abs()) + 2 * U)
    e_d = g * (e_p + 2 * U * (p - onehot).abs()) + 2.0 ** -125
    d = g * (p - onehot).abs() + e_d
    bounds = [e_loss, None, e_d @ wa + _g(n + 1) * (d @ wa), e_d.t() @ xa + _g(m + 1) * (d.t() @ xa),
              e_d.sum(0) + _g(m) * d.sum(0)]
    return [loss.detach(), z, dx, dw, db], bounds


@pytest.mark.parametrize("mnk", SHAPES)
def test_logits_exact_on_integers(cuda, mnk):
    args = _inputs(mnk, True)
    got, (want, _) = _run(*args, cuda), _reference(*args)
    assert got[1].shape == want[1].shape and torch.equal(got[1], want[1])
    if mnk[1] == 1:  # one class: p = 1, so the loss and every gradient are zero to the bit
        assert all(not t.any() for t in (got[0], *got[2:]))


@pytest.mark.parametrize("mnk", SHAPES)
def test_rounding_on_normals(cuda, mnk):
    args = _inputs(mnk, False)
    want, bounds = _reference(*args)
    for name, got, ref, bound in zip(("loss", "logits", "dx", "dw", "db"), _run(*args, cuda), want, bounds):
        if bound is not None:
            e = (got - ref).abs()
            print(f"{name}: worst error / bound {float((e / bound.clamp_min(1e-300)).max()):.3f}")
            assert got.shape == ref.shape and bool((e <= bound).all()), name


def test_ignored_rows(cuda):
    from tony_amd.ops.dense_xent import dense_xent

    x, w, b, y, gout = _inputs((33, 10, 784), False)
    dead = [0, 7, 32]
    y[dead] = torch.tensor([-100, 10, -100])
    want, bounds = _reference(x, w, b, y, gout)
    got = _run(x, w, b, y, gout, cuda)
    assert not got[0][dead].any() and not got[2][dead].any()  # loss and dx rows exactly 0
    for name, g, ref, bound in zip(("loss", "logits", "dx", "dw", "db"), got, want, bounds):
        assert bound is None or bool(((g - ref).abs() <= bound).all()), name
    mean = dense_xent(x.to(cuda), w.to(cuda), b.to(cuda), y.to(cuda)).cpu().double()  # over all 33 rows, in fp32
    assert abs(mean - want[0].sum() / 33) <= (bounds[0].sum() + _g(33) * want[0].abs().sum()) / 33


def test_same_bits(cuda):
    from tony_amd.ops.dense_xent import dense_xent

    x, w, b, y, gout = (t.to(cuda) for t in _inputs((130, 10, 128), False))
    x, w, b = x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    loss, logits = dense_xent(x, w, b, y, reduction="none", return_logits=True)
    assert all(torch.equal(f, a) for f, a in zip((loss, logits), dense_xent(x, w, b, y, "none", True)))
    first = torch.autograd.grad(loss, (x, w, b), gout, retain_graph=True)
    again = torch.autograd.grad(loss, (x, w, b), gout)
    assert all(torch.equal(f, a) for f, a in zip(first, again))


def test_no_dx_for_an_input_without_grad(cuda):
    args = _inputs((33, 10, 784), False)
    with_dx, without = _run(*args, cuda), _run(*args, cuda, x_grad=False)
    assert without[2] is None and all(torch.equal(f, a) for f, a in zip(with_dx[3:], without[3:]))
