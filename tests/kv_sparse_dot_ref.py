"""The kvstore's CSR x row-sparse dot contract (tony_amd/parallel/kvstore.py module docstring) in numpy: every fp32
operation one numpy float32 operation, the adds left to right.  ``data`` None: no multiply."""
import numpy as np


def dot(indptr, indices, data, w_ids, w_rows, D):
    """[B, D]: per sample the ordered sum of its entries' rows of ``w`` (``w_ids`` None: dense, row = column)."""
    pos = {int(c): k for k, c in enumerate(range(len(w_rows)) if w_ids is None else w_ids)}
    out = np.zeros((len(indptr) - 1, D), np.float32)
    for b in range(len(indptr) - 1):
        acc = None
        for e in range(indptr[b], indptr[b + 1]):
            if int(indices[e]) in pos:
                t = w_rows[pos[int(indices[e])]]
                t = t if data is None else (data[e] * t).astype(np.float32)
                acc = t.copy() if acc is None else (acc + t).astype(np.float32)
        if acc is not None:
            out[b] = acc
    return out


def dot_t(indptr, indices, data, dy):
    """(uniq, grad): per column the ordered sum over its entries, ascending, of ``dy`` of the entry's sample."""
    rowof = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    uniq = np.unique(indices)
    grad = np.zeros((uniq.size, dy.shape[1]), np.float32)
    for u, c in enumerate(uniq):
        acc = None
        for e in np.flatnonzero(indices == c):
            t = dy[rowof[e]] if data is None else (data[e] * dy[rowof[e]]).astype(np.float32)
            acc = t.copy() if acc is None else (acc + t).astype(np.float32)
        grad[u] = acc
    return uniq.astype(np.int64), grad
