"""Flat parameter / gradient buffers.

Every trainable tensor of a model becomes a view into one contiguous buffer
(and its ``.grad`` a view into a second one).  This is what lets the hot path
run ONE fused optimizer launch over a whole shard, ONE reduce-scatter /
all-gather / all-reduce per bucket, and a single memset to zero gradients —
instead of per-tensor launches.  The layout is padded so every shard of a
``world``-way split is a multiple of ``align`` elements (16-byte vector loads
in the HIP kernels need multiples of 8 bf16).
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass

import torch


@dataclass
class Slot:
    name: str
    offset: int
    numel: int
    shape: torch.Size
    channels_last: bool = False  # 4-D conv weight kept in [Co][R][S][Ci] memory order

    def view(self, buf: torch.Tensor) -> torch.Tensor:
        flat = buf[self.offset:self.offset + self.numel]
        if self.channels_last:
            co, ci, r, s = self.shape
            return flat.view(co, r, s, ci).permute(0, 3, 1, 2)
        return flat.view(self.shape)


class FlatParams:
    def __init__(self, module: torch.nn.Module, dtype=torch.bfloat16, device=None, world: int = 1,
                 align: int = 64, grad_dtype=None):
        params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
        if not params:
            raise ValueError("module has no trainable parameters")
        device = torch.device(device) if device is not None else params[0][1].device
        self.slots = []
        off = 0
        for name, p in params:
            # conv weights of a channels_last model stay channels_last: the implicit-GEMM convs read
            # them as [Co][R][S][Ci] and write dW in that order, with no per-step transposes
            cl = p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous()
            self.slots.append(Slot(name, off, p.numel(), p.shape, cl))
            off += (p.numel() + align - 1) // align * align  # keep every view 16B aligned
        self.numel_unpadded = off
        chunk = world * align
        self.numel = (off + chunk - 1) // chunk * chunk
        self.world = world
        self.dtype = dtype
        self.device = device
        self.data = torch.zeros(self.numel, dtype=dtype, device=device)
        self.grad = torch.zeros(self.numel, dtype=grad_dtype or dtype, device=device)
        self.params = []
        with torch.no_grad():
            for slot, (_, p) in zip(self.slots, params):
                view = slot.view(self.data)
                view.copy_(p.detach().to(device=device, dtype=dtype))
                p.data = view
                p.grad = slot.view(self.grad)
                self.params.append(p)

    @property
    def shard_numel(self) -> int:
        return self.numel // self.world

    def shard(self, buf: torch.Tensor, rank: int) -> torch.Tensor:
        n = self.shard_numel
        return buf[rank * n:(rank + 1) * n]

    def zero_grad(self):
        self.grad.zero_()

    def rebind_grads(self):
        """Re-point ``p.grad`` at the flat buffer (after user code replaced them)."""
        for slot, p in zip(self.slots, self.params):
            p.grad = slot.view(self.grad)

    def master_copy(self, rank: int = 0) -> torch.Tensor:
        return self.shard(self.data, rank).float().clone()


def build_segments(flat: FlatParams, ranges, adapt_filter=None):
    """The ``Segments`` table (ops/optim.py) of a master shard made of the flat ranges ``ranges`` -- ``(flat_lo,
    flat_hi)`` pairs laid end to end in master order: the whole buffer for Horovod, the one-rank PS and the async
    ps, the owned buckets of a dedicated ps task, rank r's piece of every bucket for the colocated PS.

    Tensor ids are slot indices, the same on every rank, so a tensor cut by a piece boundary gives segments on two
    ranks that carry one id.  A slot's alignment padding (and the buffer's tail padding) belongs to the slot before
    it: it is zero in the variables and in the gradient and stays zero.  Every range begins a new segment, so the
    ranges are also what ``norm_range`` / ``apply_range`` may be called with.

    ``adapt``: parameters with ``ndim <= 1`` (BatchNorm scale and shift, biases) take no trust ratio and no weight
    decay, the usual LARS / LAMB exclusion; ``adapt_filter(name, param) -> bool`` overrides the rule."""
    from ..ops.optim import Segments

    offs = [s.offset for s in flat.slots]
    ends = offs[1:] + [flat.numel]  # padding attributed to the slot before it
    starts, tensor, m = [0], [], 0
    for lo, hi in ranges:
        if not 0 <= lo < hi <= flat.numel or lo % 4 or hi % 4:
            raise ValueError(f"master range [{lo}, {hi}) is empty, outside the flat buffer or not 4-aligned")
        i = bisect.bisect_right(offs, lo) - 1
        while i < len(offs) and offs[i] < hi:
            a, b = max(lo, offs[i]), min(hi, ends[i])
            m += b - a
            starts.append(m)
            tensor.append(i)
            i += 1
    if adapt_filter is None:
        adapt = [len(s.shape) > 1 for s in flat.slots]
    else:
        adapt = [bool(adapt_filter(s.name, p)) for s, p in zip(flat.slots, flat.params)]
    return Segments(starts, tensor, adapt, [s.name for s in flat.slots])
