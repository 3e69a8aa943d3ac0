"""``kv.CSR`` / ``kv.dot`` on the CPU (the torch composition of the contract) bit for bit against the numpy contract
(tests/kv_sparse_dot_ref.py).  ``case`` is the one CSR the GPU tests (test_kv_sparse_dot_gpu.py) share."""
import numpy as np
import pytest
import torch

import kv_sparse_dot_ref as ref
import tony_amd.kv as kv
from kv_sparse_ref import bits

B, F = 37, 64
W_IDS = np.asarray([c for c in range(60) if c != 5] + [62], np.int64)  # column 5 missing, column 62 never asked for


def _values(rng, shape):  # magnitudes apart: the order of the adds shows in the bits
    scale = 10.0 ** rng.integers(-3, 4, (shape[0],) + (1,) * (len(shape) - 1))
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def case(D, with_data):
    """``(indptr, indices, data or None, w [F, D], dy [B, D])``, 37 samples over 64 columns: lengths 0, 1, 8 and 70
    (more than a turn of 64; it repeats columns), then 0..5; column 7 occurs exactly 70 times across the batch."""
    rng = np.random.default_rng(D)
    lens = [0, 1, 8, 70] + [int(k) for k in rng.integers(0, 6, B - 4)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    E = int(indptr[-1])
    indices = rng.integers(0, 60, E).astype(np.int64)
    indices[indices == 7] = 8
    indices[rng.choice(E, 70, replace=False)] = 7
    assert E > 70 + B and (indices == 5).any() and (indices[10:80] == 7).any()
    return indptr, indices, (_values(rng, (E,)) if with_data else None), _values(rng, (F, D)), _values(rng, (B, D))


def tensors(c, dev):
    return [None if a is None else torch.from_numpy(a).to(dev) for a in c]


def weight(w, kind, dev):  # w as kv.dot takes it and as the reference does: (kv value, w_ids or None, rows)
    if kind == "dense":
        return torch.from_numpy(w).to(dev), None, w
    rows = np.ascontiguousarray(w[W_IDS])
    return kv.RowSparse(torch.from_numpy(W_IDS).to(dev), torch.from_numpy(rows).to(dev), w.shape), W_IDS, rows


@pytest.mark.parametrize("kind", ["rsp", "dense"])
@pytest.mark.parametrize("with_data", [False, True], ids=["ones", "data"])
def test_cpu_dot_and_its_transpose_equal_the_contract(with_data, kind):
    c = case(6, with_data)
    indptr, indices, data, w, dy = c
    ip, ix, dt, _, tdy = tensors(c, "cpu")
    x = kv.CSR(ip, ix, dt, shape=(B, F))
    before = list(kv.dot_kernel_ops)
    wv, w_ids, rows = weight(w, kind, "cpu")
    got = kv.dot(x, wv)
    assert got.dtype == torch.float32 and got.shape == (B, 6)
    assert np.array_equal(bits(got.numpy()), bits(ref.dot(indptr, indices, data, w_ids, rows, 6)))
    g = kv.dot(x, tdy, transpose_a=True)
    uniq, grad = ref.dot_t(indptr, indices, data, dy)
    assert g.shape == (F, 6) and g.indices.tolist() == list(uniq) and np.array_equal(bits(g.data.numpy()), bits(grad))
    assert kv.dot_kernel_ops == before  # no kernel ran for CPU tensors
    assert x.plan() is x.plan() and x.plan()[0] is g.indices  # the plan is built once
    if not with_data:  # all ones: from_rows of dy expanded per occurrence
        want = kv.RowSparse.from_rows(ix, tdy.index_select(0, x.rowof()), (F, 6))
        assert torch.equal(g.indices, want.indices) and np.array_equal(bits(g.data.numpy()), bits(want.data.numpy()))
