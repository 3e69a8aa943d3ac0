"""Helpers shared by the bit-exact kernel tests (test_conv_exact_gpu.py, test_bn_pool_exact_gpu.py,
test_mnist_exact_gpu.py): whole-tensor equality with a readable failure, operands / destinations that live as
channel slices of poisoned allocations so an out-of-bounds read or write shows, and comparisons with a reference
that holds NaN and infinities."""
import pytest
import torch

SENT = 1.5  # the finite sentinel of every destination's surroundings (no integer: a result never equals it)


def assert_equal(got, want, what):
    """``torch.equal`` on the whole tensor; on failure the count and first coordinates of the differences."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    first = [tuple(i) for i in bad.nonzero()[:8].tolist()]
    detail = ", ".join(f"{i}: got {got[i].item()} want {want[i].item()}" for i in first)
    pytest.fail(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first {detail}")


def guard_elems(ld, dtype):
    """Elements of one guard: at least 2 x 256 rows of the operand's row stride, never less than 64 KB."""
    esz = torch.empty((), dtype=dtype).element_size()
    return -(-max(2 * 256 * ld, 65536 // esz) // 8) * 8


class Slab:
    """``rows`` x ``cols`` elements at channel offset ``c0`` of rows ``ld = cols + 2 * c0`` wide, inside one
    flat allocation filled with ``fill`` that extends a guard before the first and after the last row."""

    def __init__(self, rows, cols, c0, dtype, fill, device, guard_ld=None, vector_rows=True):
        self.rows, self.cols, self.c0, self.ld, self.fill = rows, cols, c0, cols + 2 * c0, fill
        # (a flat destination -- dW, statistics -- has no row stride: the guard is sized by ``guard_ld``)
        self.guard = guard_elems(guard_ld or self.ld, dtype)
        self.alloc = torch.full((2 * self.guard + rows * self.ld,), fill, dtype=dtype, device=device)
        self.view = self._inner(self.alloc)
        # (byte masks and per-channel vectors are not read as 16-byte row vectors: ``vector_rows=False``)
        assert not vector_rows or (self.view.data_ptr() % 16 == 0 and self.ld % 8 == 0)

    def _inner(self, alloc):
        body = alloc[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)
        return body[:, self.c0:self.c0 + self.cols]

    def ptr(self):
        return self.view.data_ptr()

    def assert_surroundings_intact(self, what):
        rest = self.alloc.clone()
        self._inner(rest).fill_(self.fill)
        assert torch.equal(rest, torch.full_like(rest, self.fill)), f"{what}: bytes outside the destination changed"


def poisoned(rows2d, c0):
    """The [rows, cols] operand as a channel slice of a NaN-filled allocation with NaN guards."""
    s = Slab(rows2d.shape[0], rows2d.shape[1], c0, rows2d.dtype, float("nan"), rows2d.device)
    s.view.copy_(rows2d)
    return s


def pix_rows(t):
    """[N, C, H, W] -> [N*H*W, C] rows (NHWC order)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def flat_slab(numel, dtype, fill, device, ld=1):
    """A contiguous tensor of ``numel`` elements inside a ``fill``-filled allocation, guards sized for rows of ``ld``."""
    return Slab(1, numel, 0, dtype, fill, device, guard_ld=ld, vector_rows=False)


def guarded(t, device, fill=float("nan"), ld=1):
    """The contiguous operand ``t`` inside an allocation filled with ``fill`` (NaN, or an out-of-range integer)."""
    s = flat_slab(t.numel(), t.dtype, fill, device, ld)
    s.view.copy_(t.reshape(1, -1))
    return s


def assert_clean(slab, want, what):
    """A destination slab against its reference: bit-equal inside, no NaN inside (a clamped load that leaked from
    the NaN around an operand), nothing changed outside."""
    got = slab.view.reshape(want.shape).cpu()
    if got.is_floating_point():
        assert not bool(got.isnan().any()), f"{what}: NaN in the destination"
    assert_equal(got, want, what)
    slab.assert_surroundings_intact(what)


def assert_same_specials(got, want, what, bound=None):
    """``got`` against a float64 reference that may hold NaN and infinities: the NaN, +inf and -inf masks are
    identical, and where the reference is finite the values are equal (within ``bound`` where one is given)."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    inf = float("inf")
    for name, g, w in (("NaN", got.isnan(), want.isnan()), ("+inf", got == inf, want == inf),
                       ("-inf", got == -inf, want == -inf)):
        if not torch.equal(g, w):
            first = [tuple(i) for i in (g != w).nonzero()[:8].tolist()]
            detail = ", ".join(f"{i}: got {got[i].item()} want {want[i].item()}" for i in first)
            pytest.fail(f"{what}: {name} mask differs at {int((g != w).sum())} of {got.numel()}; first {detail}")
    fin = want.isfinite()
    err = torch.where(fin, got - want, torch.zeros_like(want)).abs()
    bad = err > (0 if bound is None else torch.where(fin, bound.double(), torch.zeros_like(want)))
    if bool(bad.any()):
        first = [tuple(i) for i in bad.nonzero()[:8].tolist()]
        detail = ", ".join(f"{i}: got {got[i].item()} want {want[i].item()}" for i in first)
        pytest.fail(f"{what}: {int(bad.sum())} of {got.numel()} finite values differ; first {detail}")


def window_positions(flat_idx, ow):
    """``max_pool2d(..., 2, return_indices=True)``'s flat plane indices as 2x2 window positions 0..3."""
    return (2 * ((flat_idx // ow) % 2) + (flat_idx % ow) % 2).to(torch.uint8)


def assert_nan_windows_idx(idx, ref_pos, full, what):
    """``idx`` (window positions) equals the reference's in every 2x2 window of ``full`` that holds a NaN."""
    ph, pw = idx.shape[-2:]
    nanwin = full[..., :2 * ph, :2 * pw].isnan().unflatten(-2, (ph, 2)).unflatten(-1, (pw, 2)).any(-1).any(-2)
    assert_equal(torch.where(nanwin, idx, 0), torch.where(nanwin, ref_pos, 0), what)
    return nanwin
