"""``tony_kv_csr_dot`` / ``tony_kv_rows_segsum`` (csrc/kv_sparse_dot.hip) and ``kv.dot`` on the GPU, bit for bit
against the numpy contract (tests/kv_sparse_dot_ref.py), the kernels' outputs in guarded allocations."""
import numpy as np
import pytest
import torch

import kv_sparse_dot_ref as ref
import tony_amd.kv as kv
from exact_helpers import SENT, Slab
from kv_sparse_ref import bits, from_rows
from test_kv_sparse_dot_cpu import B, F, case, tensors, weight

pytestmark = pytest.mark.gpu
DIMS = [4, 36, 1028]  # one chunk, a group that does not fill its power of two, more than one pass of a wave
data_or_ones = pytest.mark.parametrize("with_data", [False, True], ids=["ones", "data"])


def _env():
    from tony_amd.ops import _lib
    dev = torch.device("cuda", 0)
    return _lib, _lib.lib(), dev, _lib.stream_ptr(dev)


def _same_bits(got, want, what):
    got = bits(got.detach().cpu().numpy().reshape(want.shape))
    assert np.array_equal(got, bits(want)), f"{what}: {int((got != bits(want)).sum())} of {want.size} differ"


@pytest.mark.parametrize("kind", ["rsp", "dense"])
@data_or_ones
@pytest.mark.parametrize("D", DIMS)
def test_csr_dot_bit_exact_in_guarded_surroundings(D, with_data, kind):
    _lib, L, dev, stream = _env()
    c = case(D, with_data)
    indptr, indices, data, w, _ = c
    ip, ix, dt, _, _ = tensors(c, dev)
    wv, w_ids, rows = weight(w, kind, dev)
    want = ref.dot(indptr, indices, data, w_ids, rows, D)
    assert not want[0].any() and want[1:].any()  # the empty sample is +0.0
    d_rows, d_ids = (wv, None) if w_ids is None else (wv.data, wv.indices.data_ptr())
    out = Slab(1, B * D, 4, torch.float32, SENT, dev, guard_ld=D, vector_rows=False)
    _lib.check(L.tony_kv_csr_dot(out.ptr(), ip.data_ptr(), ix.data_ptr(), _lib.ptr(dt) or None, d_ids,
                                 d_rows.data_ptr(), d_rows.shape[0], B, ix.numel(), D, stream), "tony_kv_csr_dot")
    _same_bits(out.view[0], want, "the kernel")
    out.assert_surroundings_intact("tony_kv_csr_dot")
    before = list(kv.dot_kernel_ops)
    _same_bits(kv.dot(kv.CSR(ip, ix, dt, shape=(B, F)), wv), want, "kv.dot")
    assert kv.dot_kernel_ops == [before[0] + 1, before[1]]


@data_or_ones
@pytest.mark.parametrize("D", DIMS)
def test_transposed_dot_bit_exact_in_guarded_surroundings(D, with_data):
    _lib, L, dev, stream = _env()
    c = case(D, with_data)
    indptr, indices, data, _, dy = c
    ip, ix, dt, _, tdy = tensors(c, dev)
    uniq, want = ref.dot_t(indptr, indices, data, dy)
    x = kv.CSR(ip, ix, dt, shape=(B, F))
    u, starts, order, rowof = x.plan()
    assert u.tolist() == uniq.tolist() and int((starts[1:] - starts[:-1]).max()) == 70
    out = Slab(1, uniq.size * D, 4, torch.float32, SENT, dev, guard_ld=D, vector_rows=False)
    _lib.check(L.tony_kv_rows_segsum(out.ptr(), tdy.data_ptr(), starts.data_ptr(), order.data_ptr(),
                                     rowof.data_ptr(), _lib.ptr(dt) or None, uniq.size, ix.numel(), B, D, stream),
               "tony_kv_rows_segsum")
    _same_bits(out.view[0], want, "the kernel")
    out.assert_surroundings_intact("tony_kv_rows_segsum")
    before = list(kv.dot_kernel_ops)
    g = kv.dot(x, tdy, transpose_a=True)
    assert g.shape == (F, D) and g.indices is u and x.plan()[0] is u  # the plan was built once
    _same_bits(g.data, want, "kv.dot")
    assert kv.dot_kernel_ops == [before[0], before[1] + 1]


def test_an_empty_csr_in_both_directions():
    dev = torch.device("cuda", 0)
    zero = torch.zeros(4, dtype=torch.int64, device=dev)
    x = kv.CSR(zero, zero[:0], shape=(3, F))
    h = kv.dot(x, torch.ones(F, 8, device=dev))
    assert h.shape == (3, 8) and h.dtype == torch.float32 and not h.any()
    g = kv.dot(x, torch.ones(3, 8, device=dev), transpose_a=True)
    assert g.nnz == 0 and g.data.shape == (0, 8) and g.shape == (F, 8)


@pytest.mark.parametrize("D", DIMS)
def test_from_rows_of_a_multiplicity_of_70_runs_the_kernel(D):
    dev = torch.device("cuda", 0)
    indptr, indices, _, _, dy = case(D, False)
    rows = dy[np.repeat(np.arange(B), np.diff(indptr))]
    uniq, want = from_rows(indices, rows)
    before = list(kv.dot_kernel_ops)
    got = kv.RowSparse.from_rows(torch.from_numpy(indices).to(dev), torch.from_numpy(rows).to(dev), (F, D))
    assert kv.dot_kernel_ops == [before[0], before[1] + 1] and got.indices.tolist() == uniq.tolist()
    _same_bits(got.data, want, f"from_rows D {D}")


def test_launchers_refuse_misaligned_pointers_and_odd_rows():
    _lib, L, dev, stream = _env()
    out, rows = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    o, r, i = out.data_ptr(), rows.data_ptr(), torch.zeros(8, dtype=torch.int64, device=dev).data_ptr()
    # (out, indptr | rows, indices | starts, data | order, w_ids | src, w_rows | val, ...): one fault each, for both
    for args in ((o + 4, i, i, r, None, r, 4, 2, 2, 8), (o, i, i, r, None, r + 2, 4, 2, 2, 8),
                 (o, i + 4, i, r, i, r, 4, 2, 2, 8), (o, i, i, r, None, r, 4, 2, 2, 5),  # (a row of 20 B)
                 (o, i, i, r, None, r, 4, -1, 2, 8), (None, i, i, r, None, r, 4, 2, 2, 8)):
        assert L.tony_kv_csr_dot(*args, stream) == -1, args
        assert L.tony_kv_rows_segsum(*args, stream) == -1, args
    assert L.tony_kv_csr_dot(o, i, i, r, None, r, 4, 0, 2, 8, stream) == 0  # no sample: nothing to launch
    assert not out.cpu().any()  # nothing was launched


def test_a_malformed_csr_is_a_value_error():
    dev = torch.device("cuda", 0)
    ip, ix, one = torch.tensor([0, 2, 3], device=dev), torch.tensor([1, 0, 3], device=dev), torch.ones(3, device=dev)
    kv.CSR(ip, ix, one, shape=(2, 4))
    for indptr, indices, data, shape in (
            (ip + 1, ix, None, (2, 4)), (torch.tensor([0, 3, 2], device=dev), ix, None, (2, 4)),  # start, decrease
            (torch.tensor([0, 2, 2], device=dev), ix, None, (2, 4)), (ip, ix, None, (3, 4)),      # end, length
            (ip, ix, None, (2, 3)), (ip, -ix, None, (2, 4)), (ip, ix.int(), None, (2, 4)),        # ids, their dtype
            (ip, ix, one[:2], (2, 4)), (ip, ix, one.double(), (2, 4)), (ip, ix, None, None),      # data, no shape
            (ip, ix.cpu(), None, (2, 4)), (ip, ix, one.cpu(), (2, 4))):                           # two devices
        with pytest.raises(ValueError):
            kv.CSR(indptr, indices, data, shape=shape)
