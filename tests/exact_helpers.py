"""Helpers shared by the bit-exact kernel tests (test_conv_exact_gpu.py, test_bn_pool_exact_gpu.py):
whole-tensor equality with a readable failure, and operands / destinations that live as channel slices of
poisoned allocations so an out-of-bounds read or write shows."""
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
