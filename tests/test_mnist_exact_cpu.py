"""The sensitivity half of test_mnist_exact_gpu.py, on the CPU: each comparison function the GPU results are held to
(exact_helpers.assert_clean, assert_same_specials, assert_nan_windows_idx) passes a tiny torch model of the kernel
line it guards and FAILS the model of the fault it is for -- a row stored past M, a column past N, an unclamped load
zeroed by a multiplication, an fmaxf ReLU, a pool with a plain ``>``, the backward mask ``y > 0``, a stride-0 gout read
with stride 1.  It also holds that module's references and inputs to what its docstrings say of them, so that a wrong
reference shows here and not as a puzzling GPU failure."""
import pytest
import torch
import torch.nn.functional as F
from exact_helpers import (SENT, assert_clean, assert_nan_windows_idx, assert_same_specials, flat_slab, guarded)
from test_mnist_exact_gpu import (B_CASES, CONV_SPOTS, DENSE_SPOTS, INF, KINDS, NAN, _assert_window_kinds, _conv_inputs,
                                  _ints, _plant, _row_kinds, conv_reference, dense_dgrad_model, dense_reference, windows,
                                  xent_b_bounds, xent_b_inputs, xent_reference)

FAILS = (AssertionError, pytest.fail.Exception)
CPU = torch.device("cpu")


def _dense_nan_case(where="x"):
    g = torch.Generator().manual_seed(33 * 1000003 + 10 * 1009 + 36)
    ins = [_ints(g, (33, 36), 0, 3), _ints(g, (10, 36), -2, 2), _ints(g, (10,), -4, 4), _ints(g, (33, 10), -2, 2)]
    return _plant(ins, where, DENSE_SPOTS[where], NAN)


def test_a_store_past_the_destination_is_seen():
    m, n = 4, 5
    want = torch.arange(m * n, dtype=torch.float32).view(m, n)

    def store(rows, cols):
        s = flat_slab(m * n, torch.float32, SENT, CPU, ld=n)
        flat = s.alloc[s.guard:]
        for r in range(rows):
            for c in range(cols):  # the kernel's address r * N + c with a wrong guard on r or c
                flat[r * n + c] = want[min(r, m - 1), min(c, n - 1)] if c < n else -1.0
        return s

    assert_clean(store(m, n), want, "the guarded store")
    for rows, cols in ((m + 1, n), (m, n + 1)):
        with pytest.raises(FAILS):
            assert_clean(store(rows, cols), want, "a store past the destination")


def test_a_multiplication_by_zero_next_to_nan_is_seen():
    """dense.hip's staging of a ragged row tile: rows past M load the last row (clamped) and are zeroed by a select."""
    m, k, tile = 3, 4, 8
    x = torch.arange(1, m * k + 1, dtype=torch.float32).view(m, k)
    xs = guarded(x, CPU, ld=k)
    flat = xs.alloc[xs.guard:]
    rows = torch.arange(tile)

    def column_sums(clamp, select):
        r = rows.clamp_max(m - 1) if clamp else rows
        v = flat[(r[:, None] * k + torch.arange(k)[None]).flatten()].view(tile, k)
        ok = (rows < m)[:, None]
        staged = torch.where(ok, v, torch.zeros(())) if select else v * ok
        out = flat_slab(k, torch.float32, SENT, CPU)
        out.view.copy_(staged.sum(0)[None])
        return out

    assert_clean(column_sums(True, True), x.sum(0), "clamped and selected")
    assert_clean(column_sums(False, True), x.sum(0), "selected")  # a stray load that a select masks costs nothing
    with pytest.raises(FAILS):
        assert_clean(column_sums(False, False), x.sum(0), "a stray load times zero")


def test_b_fmaxf_relu_is_seen():
    x, w, b, dy = _dense_nan_case()
    want = dense_reference(x, w, b, True, dy)[0]
    lin = F.linear(x.double(), w.double(), b.double())
    assert_same_specials(torch.where(lin < 0, torch.zeros(()).double(), lin), want, "relu_f")
    with pytest.raises(FAILS):
        assert_same_specials(torch.where(lin > 0, lin, torch.zeros(()).double()), want, "an fmaxf ReLU")


def _pool_model(full, ph, pw, nan_wins):
    win = windows(full, ph, pw)
    best, bi = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for pos in range(1, 4):
        v = win[..., pos]
        take = (v > best) | (v.isnan() if nan_wins else torch.zeros_like(v, dtype=torch.bool))
        best, bi = torch.where(take, v, best), torch.where(take, torch.full_like(bi, pos), bi)
    return best, bi


def test_b_pool_with_a_plain_greater_is_seen():
    k, p, nhw = 3, 1, (2, 8, 11)
    x, wt, b, dy = _plant(list(_conv_inputs(1, 32, k, p, nhw, True)), "x", CONV_SPOTS["x"], NAN)
    r = conv_reference(x, wt, b, p, True, dy, False)
    ph, pw = r["y"].shape[-2:]
    _assert_window_kinds(r["full"], ph, pw)
    y, idx = _pool_model(r["full"], ph, pw, True)
    assert_same_specials(y, r["y"], "the kernel's pool")
    assert_nan_windows_idx(idx, r["pos"], r["full"], "the kernel's idx")
    y, idx = _pool_model(r["full"], ph, pw, False)
    with pytest.raises(FAILS):
        assert_same_specials(y, r["y"], "a pool with a plain >")
    with pytest.raises(FAILS):
        assert_nan_windows_idx(idx, r["pos"], r["full"], "idx of a pool with a plain >")


def test_b_backward_mask_is_seen():
    x, w, b, dy = _dense_nan_case()
    y, dx, dw, db = dense_reference(x, w, b, True, dy)

    def grads(mask):
        d = torch.where(mask, dy.double(), torch.zeros(()).double())
        return d @ w.double(), d.t() @ x.double(), d.sum(0)

    for name, got, want in zip(("dx", "dw", "db"), grads(~(y <= 0)), (dx, dw, db)):
        assert_same_specials(got, want, name)
    with pytest.raises(FAILS):
        assert_same_specials(grads(y > 0)[2], db, "db under the mask y > 0")


def test_a_gout_stride_is_seen():
    x, w, b, labels, _ = xent_b_inputs("nan", "dy")
    gout = torch.full((33,), -2.0)
    want = xent_reference(x, w, b, labels, gout, explicit_d=True)
    gs = guarded(gout[:1], CPU)  # stride 0: one element, NaN on both sides
    flat = gs.alloc[gs.guard:]
    z = want[1]
    pmo = (z - torch.logsumexp(z, 1, keepdim=True)).exp() - F.one_hot(labels, 10).double()

    def db(stride):
        go = flat[torch.arange(33) * stride].double()
        return (go[:, None] * pmo).sum(0)

    assert_same_specials(db(0), want[4], "db", bound=torch.full((10,), 1e-12))
    with pytest.raises(FAILS):
        assert_same_specials(db(1), want[4], "db read with stride 1", bound=torch.full((10,), 1e-12))


def test_dense_dgrad_model_is_the_composition_plus_the_halo():
    k, p, nhw = 3, 1, (2, 9, 11)
    x, wt, b, dy = _conv_inputs(32, 64, k, p, nhw, True)
    r = conv_reference(x, wt, b, p, True, dy, True)
    assert torch.equal(dense_dgrad_model(r["dfull"], wt, k, p), r["dx"])
    wt[5, 2, 0, 0] = NAN
    r = conv_reference(x, wt, b, p, True, dy, True)
    model = dense_dgrad_model(r["dfull"], wt, k, p)
    assert bool(model[:, 2].isnan().all()) and bool((model.isnan() | ~r["dx"].isnan()).all())
    # torch's col2im never multiplies the corner tap into the last row and column: the documented difference
    assert bool(r["dx"][:, 2, :-1, :-1].isnan().all()) and bool(r["dx"][:, 2, -1].isfinite().all())


def test_xent_explicit_d_is_autograd_except_at_an_infinite_gout():
    x, w, b, labels, gout = xent_b_inputs("nan", "b")
    b[7] = 1.0
    for a, r in zip(xent_reference(x, w, b, labels, gout, True), xent_reference(x, w, b, labels, gout)):
        assert bool(((a - r).abs() <= 1e-12 * (1 + r.abs())).all())
    x, w, b, labels, gout = xent_b_inputs("+inf", "dy")
    auto, line = xent_reference(x, w, b, labels, gout), xent_reference(x, w, b, labels, gout, True)
    z = line[1]
    d6 = gout[6].double() * ((z[6] - torch.logsumexp(z[6], 0)).exp() - F.one_hot(labels[6], 10).double())
    assert bool(d6.isinf().all()) and d6[labels[6]] == -INF  # the stated line: infinities of the signs of p - onehot
    assert bool(auto[4].isnan()[labels[6]])                  # torch: -inf + inf at the label's class


@pytest.mark.parametrize("kind,where", B_CASES)
def test_xent_b_inputs_give_the_rows_they_promise(kind, where):
    x, w, b, labels, gout = xent_b_inputs(kind, where)
    want = xent_reference(x, w, b, labels, gout, explicit_d=(where == "dy" and kind != "nan"))
    seen = _row_kinds(want[1])
    if where == "dy":
        assert not any(seen.values()) and bool(want[0].isfinite().all())
    if (kind, where) in (("-inf", "w"), ("-inf", "b")):  # one -inf in every row: the loss stays finite
        assert seen == {"+inf": False, "only -inf": False, "one -inf": True, "nan": False}
        assert bool(want[0].isfinite().all()) and bool(want[4].isfinite().all())
    if kind == "+inf" and where != "dy":
        assert seen["+inf"] and bool(want[0].isnan().any())
    if (kind, where) == ("-inf", "x"):
        assert seen["only -inf"] and bool(want[0][4].isnan())
    bounds = xent_b_bounds(x, w, b, labels, gout)
    for r, bound in zip(want, bounds):
        assert bound is None or (bound.shape == r.shape and bool(bound[r.isfinite()].isfinite().all()))
    for r in want:  # the comparison accepts the reference itself
        assert_same_specials(r, r, "self")
    assert KINDS[kind] != 0
