"""Adasum: Horovod's adaptive summation of gradients, taken per parameter tensor (HIP kernels in csrc/adasum.hip).

The contract (tests/adasum_ref.py is the same in numpy).

Combining two gradients ``a`` and ``b`` of one parameter tensor::

    dot = sum a_i b_i      na = sum a_i^2      nb = sum b_i^2        (over that tensor alone)
    ca  = 1 - dot / (2 na)   if na >= sqrt(DBL_MIN), else 1
    cb  = 1 - dot / (2 nb)   if nb >= sqrt(DBL_MIN), else 1
    out_i = ca a_i + cb b_i

Orthogonal gradients add, equal gradients give that gradient, a zero side gives the other side.

Combining the gradients of ``N`` ranks, ``N`` a power of two: the ranks form a binary tree by rank bits; level
``d = 1, 2, 4, ...`` combines what rank ``r`` holds with what rank ``r ^ d`` holds, ``a`` always the side of the lower
rank, so for four ranks ``adasum(g0..g3) = combine(combine(g0, g1), combine(g2, g3))``.  The coefficients are taken per
parameter tensor, never over a bucket or a fused buffer: that is what makes it Horovod's Adasum and not a scaled sum.
``N = 1`` is the identity; an ``N`` that is not a power of two raises ``ValueError`` where the operator is requested
(Horovod requires the same).

Arithmetic, fixed so that ranks cannot drift apart: every product of the three sums is formed exactly in double (fp32
x fp32 and bf16 x bf16 both fit in 53 bits) and the sums are accumulated in double, in a fixed order; ``ca`` and ``cb``
are formed in double and rounded once to fp32; ``out_i = fl32(fl32(ca a_i) + fl32(cb b_i))`` with no fused
multiply-add; a bf16 buffer is read as bf16 and the fp32 result is rounded once to bf16, nearest-even.  The sum of the
two rounded products commutes and the sums use a fixed order, so the two partners of a level compute bit-identical
results from the same two vectors, and after the last level every rank holds the same bits.  A tensor's result does
not depend on which other tensors share its buffer: work items are cut from each tensor's own start and folded in an
order that depends on the tensor's own item count alone.

Two choices differ from ``horovod.torch``:

* Whole-buffer exchange.  Every level exchanges the whole buffer between the two partners (recursive doubling,
  ``parallel/collectives.py adasum_all_reduce_``), through ``torch.distributed`` point-to-point ops on the caller's
  process group.  Per rank that moves ``log2(N)`` times the buffer where a ring all-reduce moves ``2 (N-1)/N`` times
  it: 3 against 1.75 on 8 GPUs.  Horovod's vector-halving form, and an exchange through the xGMI peer-memory kernels
  (parallel/xgmi.py), are the follow-up.
* Gradients, not deltas.  ``hvd.DistributedOptimizer(op=hvd.Adasum)`` combines the gradients before the optimizer
  step, as Horovod's TensorFlow ``DistributedOptimizer`` does (the reference's Horovod examples are those);
  ``horovod.torch`` combines the optimizer's weight deltas instead.  The delta form is not provided.

``AdasumPlan`` is built once from a ``Segments`` table (ops/optim.py) and holds the work items, the per-tensor order /
start tables and the scratch buffers; ``combine_`` runs the three launches (dots, coef, combine) on the current stream.
CPU tensors, and dtypes the kernels do not take (fp16, fp64), are served by torch ops of the same contract: float64
dots, fp32 coefficients, fp32 products and sum (fp64 buffers: float64 products and sum).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .optim import Segments

ITEM_FLOATS = 4096   # longest work item of the kernels (csrc/adasum.hip kItemFloats; checked on use)
TINY = 1.4916681462400413e-154  # sqrt(DBL_MIN): a squared norm below it counts as zero
_NATIVE = (torch.float32, torch.bfloat16)


def check_world(n: int) -> None:
    """Adasum pairs ranks by rank bits: the number of ranks must be a power of two."""
    if n < 1 or n & (n - 1):
        raise ValueError(f"Adasum needs a power-of-two number of ranks, got {n}")


class AdasumPlan:
    """Where the parameter tensors lie in a flat buffer of ``dtype`` on ``device``, as the kernels' work list.

    ``segments`` covers the buffer (``Segments.validate``); the tensor ids may be sparse (a bucket of a larger flat
    buffer): they are renumbered densely in ascending order.  On the GPU, for fp32 and bf16, every segment must start on
    a 16-byte boundary (the flat buffers' slots do; ``hvd.grouped_allreduce`` packs its tensors that way)."""

    def __init__(self, segments: Segments, dtype: torch.dtype, device):
        if not dtype.is_floating_point:
            raise TypeError(f"Adasum combines floating-point gradients, got {dtype}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype
        self.numel = int(segments.starts[-1])
        segments.validate(self.numel)
        ids = sorted(set(segments.tensor))
        dense = {t: i for i, t in enumerate(ids)}
        self.tensor_ids = ids
        self.n_tensors = len(ids)
        # (lo, hi, dense tensor) of every segment, in elements
        self.segs = [(segments.starts[k], segments.starts[k + 1], dense[t]) for k, t in enumerate(segments.tensor)]
        self.native = self.device.type == "cuda" and dtype in _NATIVE
        self._recv: Optional[torch.Tensor] = None
        self._host = None
        if not self.native:
            self._by_tensor = [[] for _ in ids]
            for lo, hi, t in self.segs:
                self._by_tensor[t].append((lo, hi))
            return
        if _lib.lib().tony_adasum_item_floats() != ITEM_FLOATS:
            raise _lib.KernelError(f"{_lib.SO_PATH} is built for Adasum work items of "
                                   f"{_lib.lib().tony_adasum_item_floats()} elements, the Python side expects "
                                   f"{ITEM_FLOATS}: rebuild")
        vec = 16 // dtype.itemsize  # elements of one 16-byte vector
        if any(lo % vec for lo, _, _ in self.segs) or self.numel % vec:
            raise ValueError(f"Adasum segments of a {dtype} buffer must start and end on multiples of {vec} elements")
        items = []
        for lo, hi, t in self.segs:  # cut from the segment's own start
            items += [(a // vec, min(a + ITEM_FLOATS, hi) // vec, t, 0) for a in range(lo, hi, ITEM_FLOATS)]
        order = sorted(range(len(items)), key=lambda j: items[j][2])  # stable: a tensor's items in index order
        tstart = [0] * (self.n_tensors + 1)
        for it in items:
            tstart[it[2] + 1] += 1
        for t in range(self.n_tensors):
            tstart[t + 1] += tstart[t]
        i32 = dict(dtype=torch.int32, device=self.device)
        self.n_items = len(items)
        self.items = torch.tensor(items, **i32)
        self.order = torch.tensor(order, **i32)
        self.tstart = torch.tensor(tstart, **i32)
        self.partials = torch.zeros(len(items), 3, dtype=torch.float64, device=self.device)
        self.coef = torch.ones(self.n_tensors, 2, dtype=torch.float32, device=self.device)

    @classmethod
    def packed(cls, numels, dtype: torch.dtype, device) -> "AdasumPlan":
        """The plan of tensors of ``numels`` elements packed at 16-byte-aligned offsets (``offsets`` / ``numel`` of
        the packed buffer are kept on the plan): one segment per tensor, its zero padding included."""
        vec = max(1, 16 // dtype.itemsize)
        vec = vec * 4 // _gcd(vec, 4)  # Segments wants multiples of 4 as well
        starts, offsets = [0], []
        for n in numels:
            offsets.append(starts[-1])
            starts.append(starts[-1] + max(vec, (int(n) + vec - 1) // vec * vec))
        plan = cls(Segments(starts, list(range(len(offsets))), [True] * len(offsets)), dtype, device)
        plan.offsets = offsets
        return plan

    def recv_buffer(self) -> torch.Tensor:
        """The buffer a level receives the partner's side into: allocated once, reused by every level and step."""
        if self._recv is None:
            self._recv = torch.empty(self.numel, dtype=self.dtype, device=self.device)
        return self._recv

    def host_buffers(self):
        """Pinned host (send, receive) buffers, for a process group that cannot move device memory point to point."""
        if self._host is None:
            self._host = tuple(torch.empty(self.numel, dtype=self.dtype).pin_memory() for _ in range(2))
        return self._host

    def _check(self, dst: torch.Tensor, other: torch.Tensor):
        for t in (dst, other):
            if t.dim() != 1 or t.numel() != self.numel or t.dtype != self.dtype or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError(f"Adasum plan of {self.numel} {self.dtype} elements on {self.device} given a "
                                 f"{tuple(t.shape)} {t.dtype} tensor on {t.device}")
        if dst.data_ptr() == other.data_ptr():
            raise ValueError("Adasum combines two distinct buffers")


def _gcd(a: int, b: int) -> int:
    while b:
        a, b = b, a % b
    return a


def dots_(a: torch.Tensor, b: torch.Tensor, plan: AdasumPlan) -> torch.Tensor:
    """``plan.partials[i] = (a.b, a.a, b.b)`` of work item i, as doubles (GPU plans only)."""
    plan._check(a, b)
    rc = _lib.lib().tony_adasum_dots(a.data_ptr(), b.data_ptr(), int(plan.dtype == torch.bfloat16),
                                     plan.items.data_ptr(), plan.n_items, plan.partials.data_ptr(),
                                     _lib.stream_ptr(plan.device))
    _lib.check(rc, "tony_adasum_dots")
    return plan.partials


def coef_(plan: AdasumPlan) -> torch.Tensor:
    """``plan.coef[t] = (ca, cb)`` from ``plan.partials`` (GPU plans only)."""
    rc = _lib.lib().tony_adasum_coef(plan.partials.data_ptr(), plan.order.data_ptr(), plan.tstart.data_ptr(),
                                     plan.n_tensors, plan.coef.data_ptr(), _lib.stream_ptr(plan.device))
    _lib.check(rc, "tony_adasum_coef")
    return plan.coef


def apply_(dst: torch.Tensor, other: torch.Tensor, dst_is_a: bool, plan: AdasumPlan) -> torch.Tensor:
    """``dst = ca a + cb b`` in place with the coefficients in ``plan.coef`` (GPU plans only)."""
    plan._check(dst, other)
    rc = _lib.lib().tony_adasum_combine(dst.data_ptr(), other.data_ptr(), int(bool(dst_is_a)),
                                        int(plan.dtype == torch.bfloat16), plan.items.data_ptr(), plan.n_items,
                                        plan.coef.data_ptr(), _lib.stream_ptr(plan.device))
    _lib.check(rc, "tony_adasum_combine")
    return dst


def _combine_torch(dst, other, dst_is_a, plan):
    """The contract in torch ops, no host synchronisation: float64 dots, fp32 coefficients, fp32 products and sum."""
    a, b = (dst, other) if dst_is_a else (other, dst)
    wide = torch.float64 if plan.dtype == torch.float64 else torch.float32
    one = torch.ones((), dtype=torch.float64, device=dst.device)
    for pieces in plan._by_tensor:
        a64 = [a[lo:hi].double() for lo, hi in pieces]
        b64 = [b[lo:hi].double() for lo, hi in pieces]
        dot = sum(torch.dot(x, y) for x, y in zip(a64, b64))
        na = sum(torch.dot(x, x) for x in a64)
        nb = sum(torch.dot(y, y) for y in b64)
        ca = torch.where(na >= TINY, 1.0 - dot / (2.0 * na), one).float().to(wide)
        cb = torch.where(nb >= TINY, 1.0 - dot / (2.0 * nb), one).float().to(wide)
        for lo, hi in pieces:
            dst[lo:hi].copy_(a[lo:hi].to(wide) * ca + b[lo:hi].to(wide) * cb)
    return dst


def combine_(dst: torch.Tensor, other: torch.Tensor, dst_is_a: bool, plan: AdasumPlan) -> torch.Tensor:
    """``dst = adasum(a, b)`` in place, tensor by tensor of ``plan``; ``dst`` is the ``a`` side (the lower rank's)
    when ``dst_is_a``, else the ``b`` side.  Three launches on the current stream, nothing waits on the host."""
    if not plan.native:
        plan._check(dst, other)
        return _combine_torch(dst, other, dst_is_a, plan)
    a, b = (dst, other) if dst_is_a else (other, dst)
    dots_(a, b, plan)
    coef_(plan)
    return apply_(dst, other, dst_is_a, plan)
