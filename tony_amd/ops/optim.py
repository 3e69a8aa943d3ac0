"""Fused optimizers over flat parameter shards (HIP kernels in csrc/optim.hip: one apply kernel,
``optim_apply_kernel``, instantiated per kind; the kinds' updates in csrc/optim_math.h).

``FlatSGD`` / ``FlatAdam`` / ``FlatAdagrad`` / ``FlatRMSProp`` / ``FlatLARS`` / ``FlatLAMB`` own an fp32 master
copy of a flat parameter shard plus its optimizer state, consume a flat gradient (bf16 or fp32) and write the
updated bf16 compute copy in the same pass.  The PS shard (``tony_amd.parallel.ps``)
and the data-parallel engine use them directly; on CPU tensors the same update
is computed with PyTorch ops (used by the CPU test-suite and local mode).

Hyper-parameters are kept in a device tensor that is refreshed (a 36-byte H2D
copy) before each step, so a captured HIP graph sees the current lr / step.

Every kind also takes ``clip_norm`` (clipping by the global gradient norm), ``skip_nonfinite`` and ``ema_decay`` /
``ema_warmup`` (an EMA of the variables beside the master): see ``_FlatOptimizer``.  The norm, the clip
coefficient and the skip decision stay on the device, so these too replay from a captured graph.

``FlatLARS`` / ``FlatLAMB`` also take ``segments``, the table of where each parameter tensor lies in the shard, and
scale every tensor's update by its own trust ratio (``_FlatLayerwise``, csrc/layerwise.hip).
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Tuple

import torch

from . import _lib


SUMSQ_BLOCKS = 1024  # floats of one partial block of tony_grad_sumsq (csrc/optim.hip kSumsqGrid; checked on use)
ITEM_FLOATS = 4096   # longest work item of the layer-wise kernels (csrc/layerwise.hip kItemFloats; checked on use)
N_XHP = 8            # xhp = [clip_norm, base_grad_scale, skip_nonfinite, ema_decay, 1 - ema_decay, 0, 0, 0]


def _f32(x: float) -> float:
    """``x`` rounded to fp32 (the CPU fallbacks form the clip coefficient in the kernels' precision)."""
    return torch.tensor(float(x), dtype=torch.float32).item()


class _Kind(NamedTuple):
    """What a flat optimizer class declares about its kind, once.

    ``entry``  the plain entry point (``(w, *state, grad, grad_bf16, w_bf16, n, hp, stream)``); None: no plain form;
    ``code``   the kind's number for ``tony_optim_apply_x`` and the PS data plane (csrc/optim_math.h ``OptKind``);
               None: not available there;
    ``state``  the ordered ``(checkpoint key, attribute)`` pairs of its state tensors, ``s0`` then ``s1``;
    ``name``   the ``kind`` string of its checkpoints."""

    entry: Optional[str]
    code: Optional[int]
    state: Tuple[Tuple[str, str], ...]
    name: str


class _FlatOptimizer:
    """Common part of the flat optimizers.  Beyond the update itself every kind takes

    ``clip_norm``       clip the averaged gradient by its global L2 norm (``tf.clip_by_global_norm``: the
                        gradient is scaled by ``clip_norm / max(norm, clip_norm)``, before weight decay is added);
    ``skip_nonfinite``  a step whose gradient holds an inf / nan (or whose sum of squares overflows fp32) changes
                        nothing; the skip is decided on the device, so the host's step counter still advances;
    ``ema_decay``       keep ``ema += (1 - d)(w - ema)`` beside the master (``tf.train.ExponentialMovingAverage``,
                        the shadow starts as a copy of the master); ``ema_warmup`` uses TF's ``num_updates`` form
                        ``d = min(ema_decay, (1 + t) / (10 + t))`` with t the step being applied.

    With all four at their defaults nothing is allocated and ``apply_range`` launches the plain kernel of its
    kind.  Otherwise the norm takes two small launches before the apply (``accumulate_sumsq`` once per bucket,
    ``finish_norm`` once per step: csrc/optim.hip tony_grad_sumsq / tony_clip_ctl) and the apply is
    ``tony_optim_apply_x``, which reads the coefficient and the skip flag on the device."""

    n_hp = 0
    kind: _Kind = None  # every concrete class declares its own

    def __init__(self, master: torch.Tensor, lr: float, weight_decay: float = 0.0, clip_norm=None,
                 skip_nonfinite: bool = False, ema_decay=None, ema_warmup: bool = False):
        if master.dtype != torch.float32 or master.dim() != 1:
            raise TypeError("master shard must be a flat fp32 tensor")
        if master.numel() % 4:
            raise ValueError("flat shard length must be a multiple of 4 (pad the buffer)")
        if clip_norm is not None and not float(clip_norm) > 0.0:
            raise ValueError(f"clip_norm must be positive (None: no clipping), got {clip_norm}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (None: no EMA), got {ema_decay}")
        if ema_warmup and ema_decay is None:
            raise ValueError("ema_warmup needs ema_decay")
        self.w = master
        self.lr = float(lr)
        self.weight_decay = float(weight_decay)
        self.grad_scale = 1.0
        self.step_count = 0
        dev = master.device
        self._hp_last = None
        self._hp_dev = torch.zeros(self.n_hp, dtype=torch.float32, device=dev)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.needs_norm = self.clip_norm is not None or self.skip_nonfinite
        self._extended = self.needs_norm or self.ema_decay is not None
        self.ema = self._xhp_dev = self._xhp_last = self._ctl = self._partials = None
        if self._extended:
            self._xhp_dev = torch.zeros(N_XHP, dtype=torch.float32, device=dev)
            self._ctl = torch.zeros(4, dtype=torch.float32, device=dev)
            self._ctl[0] = 1.0  # [coef, skip, norm, skipped steps]
            if self.ema_decay is not None:
                self.ema = master.detach().clone()
            if dev.type == "cuda" and _lib.lib().tony_grad_sumsq_blocks() != SUMSQ_BLOCKS:
                raise _lib.KernelError(f"{_lib.SO_PATH} stores {_lib.lib().tony_grad_sumsq_blocks()} partials per "
                                       f"sum-of-squares launch, the Python side expects {SUMSQ_BLOCKS}: rebuild")

    # -- clipping / skip / EMA ------------------------------------------------------------------------------
    def _ema_decay_now(self) -> float:
        d = self.ema_decay
        if self.ema_warmup:
            t = self.step_count
            d = min(d, (1.0 + t) / (10.0 + t))
        return d

    def _xhp_values(self):
        d = self._ema_decay_now() if self.ema_decay is not None else 0.0
        return [self.clip_norm or 0.0, self.grad_scale, 1.0 if self.skip_nonfinite else 0.0, d, 1.0 - d, 0.0, 0.0,
                0.0]

    def partials(self, n_slots: int = 1) -> torch.Tensor:
        """The ``n_slots`` partial blocks (``SUMSQ_BLOCKS`` floats each, zero until accumulated into) that
        ``finish_norm(n_slots)`` folds; a sharded PS all-reduces them between the two."""
        if not self.needs_norm:
            raise RuntimeError("the gradient norm needs clip_norm or skip_nonfinite")
        if self._partials is None or self._partials.numel() < n_slots * SUMSQ_BLOCKS:
            if self.w.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("partial blocks must exist before a graph capture: call partials(n_slots) first")
            old = self._partials
            self._partials = torch.zeros(n_slots * SUMSQ_BLOCKS, dtype=torch.float32, device=self.w.device)
            if old is not None:
                self._partials[:old.numel()].copy_(old)
        return self._partials[:n_slots * SUMSQ_BLOCKS]

    def share_partials(self, other: "_FlatOptimizer", n_slots: int):
        """Use ``other``'s partial blocks: several optimizers (one per dtype group) then accumulate into their own
        slot of one buffer and each ``finish_norm(n_slots)`` sees the norm over all of them."""
        self._partials = other.partials(n_slots)

    def accumulate_sumsq(self, grad: torch.Tensor, slot: int = 0):
        """Partial block ``slot`` = the sum of squares of ``grad`` (a whole flat gradient, or one bucket's piece
        of it), in a fixed order: the same gradient gives the same bits."""
        if grad.numel() % 4:
            raise ValueError("gradient length must be a multiple of 4")
        blk = self.partials(slot + 1)[slot * SUMSQ_BLOCKS:]
        if self.w.is_cuda:
            rc = _lib.lib().tony_grad_sumsq(grad.data_ptr(), int(grad.dtype == torch.bfloat16), grad.numel(),
                                            blk.data_ptr(), _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_grad_sumsq")
            return
        blk.zero_()
        blk[0] = grad.double().square().sum().float()

    def finish_norm(self, n_slots: int = 1):
        """Fold partial blocks [0, n_slots) into ``[coef, skip, norm, skipped steps]`` for the applies that follow."""
        part = self.partials(n_slots)
        if self.w.is_cuda:
            rc = _lib.lib().tony_clip_ctl(part.data_ptr(), part.numel(), self._xhp_dev.data_ptr(),
                                          self._ctl.data_ptr(), _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_clip_ctl")
            return
        S = part.double().sum().item()
        finite = S == S and S != float("inf")
        clip, gs = _f32(self.clip_norm or 0.0), _f32(self.grad_scale)
        norm = _f32(gs * S ** 0.5) if finite else (float("nan") if S != S else float("inf"))
        skip = self.skip_nonfinite and not finite
        big = clip if not norm > clip else norm  # fmaxf: a nan norm gives clip
        self._ctl[0] = _f32(clip / big) if clip > 0.0 else 1.0
        self._ctl[1] = 1.0 if skip else 0.0
        self._ctl[2] = norm
        if skip:
            self._ctl[3] += 1.0

    def last_norm(self) -> float:
        """The global gradient norm of the last ``finish_norm`` (synchronises: logging and tests only)."""
        return float(self._ctl[2].item()) if self._ctl is not None else float("nan")

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient so far (synchronises: logging and tests only)."""
        return int(self._ctl[3].item()) if self._ctl is not None else 0

    def _apply_x(self, grad: torch.Tensor, lo: int, out_bf16):
        """``apply_range`` with clipping / skip / EMA: tony_optim_apply_x, or the same on CPU tensors."""
        n = grad.numel()
        if self.w.is_cuda:
            code, s0, s1 = self.plane_state()
            rc = _lib.lib().tony_optim_apply_x(
                code, self.w.data_ptr() + 4 * lo, s0.data_ptr() + 4 * lo, 0 if s1 is None else s1.data_ptr() + 4 * lo,
                0 if self.ema is None else self.ema.data_ptr() + 4 * lo, grad.data_ptr(),
                int(grad.dtype == torch.bfloat16), _lib.ptr(out_bf16), n, self._hp_dev.data_ptr(),
                self._xhp_dev.data_ptr(), self._ctl.data_ptr() if self.needs_norm else 0,
                _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_optim_apply_x")
            return
        if self.needs_norm and self._ctl[1].item() != 0.0:
            return  # skipped: nothing changes
        gs = self.grad_scale
        if self.needs_norm:
            self.grad_scale = _f32(_f32(gs) * self._ctl[0].item())
        try:
            self._apply_cpu(grad, lo, out_bf16)
        finally:
            self.grad_scale = gs
        self._ema_cpu(lo, n)

    def _ema_cpu(self, lo, n):
        if self.ema is not None:
            e = self.ema[lo:lo + n]
            e.add_((self.w[lo:lo + n] - e) * (1.0 - self._ema_decay_now()))

    def _extras_state(self, sd: dict) -> dict:
        if self.ema is not None:
            sd["ema"] = self.ema
        if self._extended:
            sd["skipped"] = self.skipped_steps()
        return sd

    def _load_extras(self, sd: dict):
        """After the masters are restored: the EMA and the skipped-step count of a checkpoint.  One written
        without an EMA re-seeds it from the master (with a warning); one with an EMA needs ``ema_decay`` here."""
        if sd.get("ema") is not None and self.ema is None:
            raise ValueError("the checkpoint holds an EMA of the variables, this optimizer keeps none: "
                             "construct it with ema_decay")
        if self.ema is not None:
            if sd.get("ema") is None:
                import warnings

                warnings.warn("optimizer checkpoint without an EMA of the variables: re-seeding it from the master",
                              RuntimeWarning)
                self.ema.copy_(self.w)
            else:
                self.ema.copy_(sd["ema"])
        if self._ctl is not None:
            self._ctl[3] = float(sd.get("skipped", 0))

    def _hp_values(self):
        raise NotImplementedError

    def _push_hp(self):
        if self.w.is_cuda and torch.cuda.is_current_stream_capturing():
            return  # graph capture: the Trainer refreshes hp before every replay
        if self._extended:
            xvals = [float(v) for v in self._xhp_values()]
            if xvals != self._xhp_last:
                self._xhp_dev.copy_(torch.tensor(xvals, dtype=torch.float32), non_blocking=True)
                self._xhp_last = xvals
        vals = [float(v) for v in self._hp_values()]
        if vals == self._hp_last:
            return  # unchanged (constant-lr SGD): no H2D traffic at all
        # pageable source: the copy is staged before copy_ returns, so the host
        # may rewrite its values for the next step without racing the DMA
        self._hp_dev.copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=True)
        self._hp_last = vals

    def begin_step(self):
        """Advance the step counter and push this step's hyper-parameters (before any apply_range)."""
        self.step_count += 1
        if self.w.is_cuda:
            self._push_hp()

    def _check_range(self, grad, lo):
        n = grad.numel()
        if lo < 0 or lo + n > self.w.numel() or lo % 4 or n % 4:
            raise ValueError(f"range [{lo}, {lo + n}) outside the {self.w.numel()}-element shard or not 4-aligned")
        return n

    def _states(self):
        return [getattr(self, attr) for _, attr in self.kind.state]

    def apply_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        """Update master elements [lo, lo + grad.numel()) (one bucket of a sharded PS) with ``grad``;
        hyper-parameters are those pushed by the last ``begin_step``."""
        n = self._check_range(grad, lo)
        if self._extended:
            return self._apply_x(grad, lo, out_bf16)
        if self.w.is_cuda:
            entry = self.kind.entry
            ptrs = [t.data_ptr() + 4 * lo for t in (self.w, *self._states())]
            rc = getattr(_lib.lib(), entry)(*ptrs, grad.data_ptr(), int(grad.dtype == torch.bfloat16),
                                            _lib.ptr(out_bf16), n, self._hp_dev.data_ptr(),
                                            _lib.stream_ptr(self.w.device))
            _lib.check(rc, entry)
            return
        self._apply_cpu(grad, lo, out_bf16)

    def _begin_whole(self, grad: torch.Tensor):
        """What every whole-shard ``step`` starts with: ``begin_step`` and, where it is needed, the norm of ``grad``."""
        if grad.numel() != self.w.numel():
            raise ValueError("grad / shard size mismatch")
        self.begin_step()
        if self.needs_norm:
            self.accumulate_sumsq(grad, 0)
            self.finish_norm(1)

    def step(self, grad: torch.Tensor, out_bf16: torch.Tensor | None = None):
        """One whole-shard update: ``begin_step`` + ``apply_range`` over every element (with ``clip_norm`` or
        ``skip_nonfinite``: the norm of ``grad`` first)."""
        self._begin_whole(grad)
        self.apply_range(grad, 0, out_bf16)

    def state_dict(self):
        sd = {"kind": self.kind.name, "step": self.step_count}
        sd.update((key, getattr(self, attr)) for key, attr in self.kind.state)
        sd["lr"] = self.lr
        return self._extras_state(sd)

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for key, attr in self.kind.state:
            getattr(self, attr).copy_(sd[key])
        self.lr = float(sd.get("lr", self.lr))
        self._load_extras(sd)

    def plane_state(self):
        """``(opt, s0, s1)`` for the PS data plane's apply kernel (csrc/ps_plane.hip ``tony_ps_apply``): its
        optimizer code and the one or two state tensors it updates beside the master (``s1`` may be None)."""
        s = self._states()
        return self.kind.code, s[0], s[1] if len(s) > 1 else None


class FlatSGD(_FlatOptimizer):
    """SGD with (Nesterov) momentum: v = mu*v + g + wd*w ; w -= lr*v (TF MomentumOptimizer semantics)."""

    n_hp = 6
    kind = _Kind("tony_sgd_step", 0, (("momentum_buffer", "v"),), "sgd")

    def __init__(self, master, lr, momentum=0.9, weight_decay=0.0, nesterov=False, resync=False, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        # resync: the bf16 compute copy (``out_bf16``) is the parameters users see and may overwrite
        # (load_state_dict, broadcast_parameters); elements changed there re-seed the fp32 master
        # before the update (csrc/optim_math.h resync4).  Off for the PS, whose masters are the truth.
        self.resync = bool(resync)
        self.v = torch.zeros_like(master)

    def _hp_values(self):
        return [self.lr, self.momentum, self.weight_decay, self.grad_scale, 1.0 if self.nesterov else 0.0,
                1.0 if self.resync else 0.0]

    def _apply_cpu(self, grad, lo, out_bf16):
        n = grad.numel()
        w, v = self.w[lo:lo + n], self.v[lo:lo + n]
        if self.resync and out_bf16 is not None:
            changed = out_bf16 != w.to(out_bf16.dtype)
            w.copy_(torch.where(changed, out_bf16.float(), w))
        g = grad.float() * self.grad_scale + self.weight_decay * w
        v.mul_(self.momentum).add_(g)
        upd = g + self.momentum * v if self.nesterov else v
        w.add_(upd, alpha=-self.lr)
        if out_bf16 is not None:
            out_bf16.copy_(w)


class FlatAdam(_FlatOptimizer):
    """Adam / AdamW (``decoupled=True``) with bias correction."""

    n_hp = 9
    kind = _Kind("tony_adam_step", 1, (("exp_avg", "m"), ("exp_avg_sq", "v")), "adam")

    def __init__(self, master, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        self.eps = float(eps)
        self.decoupled = bool(decoupled)
        self.m = torch.zeros_like(master)
        self.v = torch.zeros_like(master)

    def _hp_values(self):
        t = self.step_count
        return [self.lr, self.b1, self.b2, self.eps, self.weight_decay, self.grad_scale,
                1.0 - self.b1 ** t, 1.0 - self.b2 ** t, 1.0 if self.decoupled else 0.0]

    def _apply_cpu(self, grad, lo, out_bf16):
        n = grad.numel()
        t = self.step_count
        w, m, v = self.w[lo:lo + n], self.m[lo:lo + n], self.v[lo:lo + n]
        g = grad.float() * self.grad_scale
        if self.decoupled:
            w.mul_(1.0 - self.lr * self.weight_decay)
        else:
            g = g + self.weight_decay * w
        m.mul_(self.b1).add_(g, alpha=1 - self.b1)
        v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
        denom = (v.sqrt() / (1 - self.b2 ** t) ** 0.5).add_(self.eps)
        w.addcdiv_(m, denom, value=-self.lr / (1 - self.b1 ** t))
        if out_bf16 is not None:
            out_bf16.copy_(w)


class FlatAdagrad(_FlatOptimizer):
    """Adagrad: g' = g + wd*w ; h += g'^2 ; w -= lr*g' / (sqrt(h) + eps)  (``torch.optim.Adagrad`` with
    ``lr_decay=0``, Keras ``Adagrad``); ``h`` starts at ``initial_accumulator_value``."""

    n_hp = 4
    kind = _Kind("tony_adagrad_step", 2, (("sum", "h"),), "adagrad")

    def __init__(self, master, lr, eps=1e-7, initial_accumulator_value=0.1, weight_decay=0.0, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.eps = float(eps)
        self.h = torch.full_like(master, float(initial_accumulator_value))

    def _hp_values(self):
        return [self.lr, self.eps, self.weight_decay, self.grad_scale]

    def _apply_cpu(self, grad, lo, out_bf16):
        n = grad.numel()
        w, h = self.w[lo:lo + n], self.h[lo:lo + n]
        g = grad.float() * self.grad_scale + self.weight_decay * w
        h.addcmul_(g, g)
        w.addcdiv_(g, h.sqrt().add_(self.eps), value=-self.lr)
        if out_bf16 is not None:
            out_bf16.copy_(w)


class FlatRMSProp(_FlatOptimizer):
    """RMSProp (not centered): g' = g + wd*w ; ms = alpha*ms + (1-alpha)*g'^2, then

    torch style (``tf_style=False``, ``torch.optim.RMSprop``): mom = momentum*mom + g'/(sqrt(ms) + eps) ;
    w -= lr*mom ; ``ms`` starts at 0;
    TF style (``tf_style=True``, ``tf.train.RMSPropOptimizer``, the Inception recipe): mom = momentum*mom +
    lr*g'/sqrt(ms + eps) ; w -= mom ; ``ms`` starts at 1.

    Both states are always kept; ``momentum=0`` falls out of the same formula."""

    n_hp = 7
    kind = _Kind("tony_rmsprop_step", 3, (("square_avg", "ms"), ("momentum_buffer", "mom")), "rmsprop")

    def __init__(self, master, lr, alpha=0.9, momentum=0.0, eps=1e-8, weight_decay=0.0, tf_style=False, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.alpha = float(alpha)
        self.momentum = float(momentum)
        self.eps = float(eps)
        self.tf_style = bool(tf_style)
        self.ms = torch.ones_like(master) if self.tf_style else torch.zeros_like(master)
        self.mom = torch.zeros_like(master)

    def _hp_values(self):
        return [self.lr, self.alpha, self.momentum, self.eps, self.weight_decay, self.grad_scale,
                1.0 if self.tf_style else 0.0]

    def _apply_cpu(self, grad, lo, out_bf16):
        n = grad.numel()
        w, ms, mom = self.w[lo:lo + n], self.ms[lo:lo + n], self.mom[lo:lo + n]
        g = grad.float() * self.grad_scale + self.weight_decay * w
        ms.mul_(self.alpha).addcmul_(g, g, value=1 - self.alpha)
        if self.tf_style:
            mom.mul_(self.momentum).addcdiv_(g, (ms + self.eps).sqrt_(), value=self.lr)
            w.sub_(mom)
        else:
            mom.mul_(self.momentum).addcdiv_(g, ms.sqrt().add_(self.eps))
            w.add_(mom, alpha=-self.lr)
        if out_bf16 is not None:
            out_bf16.copy_(w)

    def state_dict(self):
        return {**super().state_dict(), "tf_style": self.tf_style}

    def load_state_dict(self, sd):
        if bool(sd.get("tf_style", self.tf_style)) != self.tf_style:
            raise ValueError(f"RMSProp checkpoint has tf_style={sd['tf_style']}, this optimizer {self.tf_style}")
        super().load_state_dict(sd)


@dataclass
class Segments:
    """Where the parameter tensors lie in a master shard (built by ``parallel.flat.build_segments``).

    ``starts``  K+1 ascending offsets in master coordinates, multiples of 4, from 0 to the shard's length;
    ``tensor``  the global tensor id in [0, T) of each of the K segments (a tensor cut by a bucket or piece boundary
                gives several segments, possibly on several ranks, with the same id);
    ``adapt``   T booleans: tensor t takes a trust ratio and weight decay (else ratio 1, weight decay 0)."""

    starts: List[int]
    tensor: List[int]
    adapt: List[bool]
    names: Optional[List[str]] = None

    @classmethod
    def whole(cls, n: int) -> "Segments":
        """The shard as one adapted tensor."""
        return cls([0, int(n)], [0], [True])

    def validate(self, n: int):
        s = self.starts
        if len(s) != len(self.tensor) + 1 or len(s) < 2 or s[0] != 0 or s[-1] != n:
            raise ValueError(f"segments must cover [0, {n}) with one tensor id per segment")
        if any(a % 4 for a in s) or any(b <= a for a, b in zip(s, s[1:])):
            raise ValueError("segment offsets must be ascending multiples of 4")
        if not self.adapt or any(not 0 <= t < len(self.adapt) for t in self.tensor):
            raise ValueError(f"segment tensor ids must lie in [0, {len(self.adapt)})")


class _FlatLayerwise(_FlatOptimizer):
    """Common part of ``FlatLARS`` / ``FlatLAMB``: the update of every parameter tensor is scaled by a trust ratio
    taken over that tensor alone (csrc/layerwise.hip).  A step is

        ``norm_range``     once per bucket: a pair (sum w^2, sum x^2) per work item, a fixed order (LAMB's also
                           updates the moments);
        ``fold_norms``     once per step: ``tsum[T][2]``, each tensor's pairs summed in double -- a sharded caller
                           all-reduces ``tsum`` here, so that a tensor cut over two ranks gets its whole norm;
        ``finish_ratios``  once per step: the device table ``(ratio_t, wd_t)``;
        ``apply_range``    once per bucket.

    Ranges handed to ``norm_range`` / ``apply_range`` begin and end on segment boundaries or multiples of
    ``ITEM_FLOATS`` inside a segment.  ``clip_norm`` / ``skip_nonfinite`` (``accumulate_sumsq`` + ``finish_norm``
    come first, as for every kind) and the EMA compose: the clip coefficient multiplies the gradient before the
    ratio is taken, a skipped step writes nothing."""

    layer_kind = 0

    def _init_segments(self, segments: Optional[Segments]):
        n, dev = self.w.numel(), self.w.device
        seg = segments if segments is not None else Segments.whole(n)
        seg.validate(n)
        self.segments = seg
        T = len(seg.adapt)
        if dev.type == "cuda" and _lib.lib().tony_layerwise_item_floats() != ITEM_FLOATS:
            raise _lib.KernelError(f"{_lib.SO_PATH} is built for work items of "
                                   f"{_lib.lib().tony_layerwise_item_floats()} floats, the Python side expects "
                                   f"{ITEM_FLOATS}: rebuild")
        items = []
        for k, t in enumerate(seg.tensor):
            lo, hi = seg.starts[k], seg.starts[k + 1]
            items += [(a // 4, min(a + ITEM_FLOATS, hi) // 4, t, 0) for a in range(lo, hi, ITEM_FLOATS)]
        self._item_lo = [4 * it[0] for it in items]
        order = sorted(range(len(items)), key=lambda j: items[j][2])  # stable: a tensor's items in index order
        tstart = [0] * (T + 1)
        for it in items:
            tstart[it[2] + 1] += 1
        for t in range(T):
            tstart[t + 1] += tstart[t]
        i32 = dict(dtype=torch.int32, device=dev)
        self._items = torch.tensor(items, **i32)
        self._order = torch.tensor(order, **i32)
        self._tstart = torch.tensor(tstart, **i32)
        self._adapt = torch.tensor([int(bool(a)) for a in seg.adapt], **i32)
        self._item_part = torch.zeros(len(items), 2, dtype=torch.float32, device=dev)
        self._seg_part = torch.zeros(len(seg.tensor), 2, dtype=torch.float64)  # the CPU fallback's, per segment
        self.tsum = torch.zeros(T, 2, dtype=torch.float32, device=dev)
        self.table = torch.tensor([[1.0, 0.0]] * T, dtype=torch.float32, device=dev)

    # -- ranges -------------------------------------------------------------------------------------------
    def _item_range(self, lo: int, n: int):
        """Work items [i0, i1) that make up master elements [lo, lo + n)."""
        i0, i1 = bisect.bisect_left(self._item_lo, lo), bisect.bisect_left(self._item_lo, lo + n)
        if n and (i0 >= len(self._item_lo) or self._item_lo[i0] != lo or
                  (i1 < len(self._item_lo) and self._item_lo[i1] != lo + n)):
            raise ValueError(f"range [{lo}, {lo + n}) does not begin and end on work-item boundaries: build the "
                             "segments from the ranges that are applied")
        return i0, i1

    def _segs_in(self, lo: int, n: int):
        """(k, a, b, tensor) of the segments that make up [lo, lo + n), for the CPU fallback."""
        s = self.segments.starts
        k0, k1 = bisect.bisect_left(s, lo), bisect.bisect_left(s, lo + n)
        if n and (s[k0] != lo or s[k1] != lo + n):
            raise ValueError(f"range [{lo}, {lo + n}) does not begin and end on segment boundaries")
        return [(k, s[k], s[k + 1], self.segments.tensor[k]) for k in range(k0, k1)]

    def _skipped_now(self) -> bool:
        return self.needs_norm and self._ctl[1].item() != 0.0

    def _coef_now(self) -> float:
        return self._ctl[0].item() if self.needs_norm else 1.0

    def _ctl_ptr(self) -> int:
        return self._ctl.data_ptr() if self.needs_norm else 0

    # -- the norm stages ----------------------------------------------------------------------------------
    def norm_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        raise NotImplementedError

    def fold_norms(self) -> torch.Tensor:
        """``tsum[T][2]`` from the pairs of every ``norm_range`` of this step; returned for the cross-rank sum."""
        if self.w.is_cuda:
            rc = _lib.lib().tony_layerwise_fold(self._item_part.data_ptr(), self._order.data_ptr(),
                                                self._tstart.data_ptr(), self.tsum.shape[0], self.tsum.data_ptr(),
                                                _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_layerwise_fold")
            return self.tsum
        if self._skipped_now() and self.layer_kind == 1:
            return self.tsum
        acc = torch.zeros(self.tsum.shape, dtype=torch.float64)
        acc.index_add_(0, torch.tensor(self.segments.tensor, dtype=torch.long), self._seg_part)
        self.tsum.copy_(acc)
        return self.tsum

    def _ratio_cpu(self, sw: float, sx: float, coef: float):
        raise NotImplementedError

    def finish_ratios(self):
        """The table ``(ratio_t, wd_t)`` from ``tsum`` (after the cross-rank sum, where there is one)."""
        if self.w.is_cuda:
            rc = _lib.lib().tony_layerwise_ratio(self.layer_kind, self.tsum.data_ptr(), self._adapt.data_ptr(),
                                                 self.tsum.shape[0], self._hp_dev.data_ptr(), self._ctl_ptr(),
                                                 self.table.data_ptr(), _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_layerwise_ratio")
            return
        if self._skipped_now():
            return
        coef, wd = self._coef_now(), _f32(self.weight_decay)
        for t, ad in enumerate(self.segments.adapt):
            if not ad:
                self.table[t, 0], self.table[t, 1] = 1.0, 0.0
                continue
            self.table[t, 0] = self._ratio_cpu(self.tsum[t, 0].item(), self.tsum[t, 1].item(), coef)
            self.table[t, 1] = wd

    def ratios(self) -> torch.Tensor:
        """The trust ratios of the last ``finish_ratios``, one per tensor (a copy)."""
        return self.table[:, 0].clone()

    def step(self, grad: torch.Tensor, out_bf16: torch.Tensor | None = None):
        self._begin_whole(grad)
        self.norm_range(grad, 0, out_bf16)
        self.fold_norms()
        self.finish_ratios()
        self.apply_range(grad, 0, out_bf16)

    def plane_state(self):
        raise NotImplementedError("LARS and LAMB are not available on the xGMI PS data plane")


class FlatLARS(_FlatLayerwise):
    """LARS in the LARC form over SGD with (Nesterov) momentum: per tensor, with wn = ||w|| and gn = ||g|| (the
    averaged, clipped gradient), ratio = trust_coef wn / (gn + wd wn + eps) (1 when either norm is 0), then
    v = mu v + ratio (g + wd w) ; w -= lr v.  Tensors that are not adapted take ratio 1 and no weight decay."""

    n_hp = 8
    kind = _Kind(None, None, (("momentum_buffer", "v"),), "lars")
    layer_kind = 0

    def __init__(self, master, lr, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coef=0.001, eps=0.0,
                 segments: Optional[Segments] = None, resync=False, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.trust_coef = float(trust_coef)
        self.eps = float(eps)
        self.resync = bool(resync)
        self.v = torch.zeros_like(master)
        self._init_segments(segments)

    def _hp_values(self):
        return [self.lr, self.momentum, self.weight_decay, self.grad_scale, 1.0 if self.nesterov else 0.0,
                1.0 if self.resync else 0.0, self.trust_coef, self.eps]

    def _resynced(self, w, out_bf16):
        if self.resync and out_bf16 is not None and out_bf16.dtype == torch.bfloat16:
            return torch.where(out_bf16 != w.to(out_bf16.dtype), out_bf16.float(), w)
        return w

    def norm_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        """The pairs (sum w^2, sum g^2) of master elements [lo, lo + grad.numel()); reads only."""
        n = self._check_range(grad, lo)
        if self.w.is_cuda:
            i0, i1 = self._item_range(lo, n)
            rc = _lib.lib().tony_lars_norm(self.w.data_ptr(), grad.data_ptr(), int(grad.dtype == torch.bfloat16),
                                           _lib.ptr(out_bf16), lo, self._items.data_ptr() + 16 * i0, i1 - i0,
                                           self._item_part.data_ptr() + 8 * i0, self._hp_dev.data_ptr(),
                                           _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_lars_norm")
            return
        for k, a, b, _ in self._segs_in(lo, n):
            w = self._resynced(self.w[a:b], None if out_bf16 is None else out_bf16[a - lo:b - lo])
            self._seg_part[k, 0] = w.double().square().sum()
            self._seg_part[k, 1] = grad[a - lo:b - lo].double().square().sum()

    def _ratio_cpu(self, sw, sg, coef):
        wn, gn = sw ** 0.5, _f32(self.grad_scale) * coef * sg ** 0.5
        if not (wn > 0.0 and gn > 0.0):
            return 1.0
        return _f32(_f32(self.trust_coef) * wn / (gn + _f32(self.weight_decay) * wn + _f32(self.eps)))

    def apply_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        n = self._check_range(grad, lo)
        if self.w.is_cuda:
            i0, i1 = self._item_range(lo, n)
            rc = _lib.lib().tony_lars_apply(
                self.w.data_ptr(), self.v.data_ptr(), 0 if self.ema is None else self.ema.data_ptr(),
                grad.data_ptr(), int(grad.dtype == torch.bfloat16), _lib.ptr(out_bf16), lo,
                self._items.data_ptr() + 16 * i0, i1 - i0, self.table.data_ptr(), self._hp_dev.data_ptr(),
                0 if self._xhp_dev is None else self._xhp_dev.data_ptr(), self._ctl_ptr(),
                _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_lars_apply")
            return
        if self._skipped_now():
            return
        gsc = _f32(_f32(self.grad_scale) * self._coef_now())
        for _, a, b, t in self._segs_in(lo, n):
            ratio, wd = self.table[t, 0].item(), self.table[t, 1].item()
            w, v = self.w[a:b], self.v[a:b]
            out = None if out_bf16 is None else out_bf16[a - lo:b - lo]
            w.copy_(self._resynced(w, out))
            g = grad[a - lo:b - lo].float() * _f32(gsc * ratio) + _f32(wd * ratio) * w
            v.mul_(self.momentum).add_(g)
            w.add_(g + self.momentum * v if self.nesterov else v, alpha=-self.lr)
            if out is not None:
                out.copy_(w)
        self._ema_cpu(lo, n)


class FlatLAMB(_FlatLayerwise):
    """LAMB: Adam's moments with bias correction, u = (m/bc1) / (sqrt(v/bc2) + eps) + wd w, and per tensor
    ratio = ||w|| / ||u|| (1 when either norm is 0), w -= lr ratio u.  Tensors that are not adapted take ratio 1
    and no weight decay (plain Adam)."""

    n_hp = 8
    kind = _Kind(None, None, (("exp_avg", "m"), ("exp_avg_sq", "v")), "lamb")
    layer_kind = 1

    def __init__(self, master, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
                 segments: Optional[Segments] = None, **extra):
        super().__init__(master, lr, weight_decay, **extra)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        self.eps = float(eps)
        self.m = torch.zeros_like(master)
        self.v = torch.zeros_like(master)
        self._init_segments(segments)

    def _hp_values(self):
        t = self.step_count
        return [self.lr, self.b1, self.b2, self.eps, self.weight_decay, self.grad_scale, 1.0 - self.b1 ** t,
                1.0 - self.b2 ** t]

    def _u_cpu(self, a, b, wd):
        t = self.step_count
        bc1, bc2 = 1.0 - self.b1 ** t, 1.0 - self.b2 ** t
        return (self.m[a:b] / bc1) / ((self.v[a:b] / bc2).sqrt() + self.eps) + wd * self.w[a:b]

    def norm_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        """The moment update of master elements [lo, lo + grad.numel()) and their pairs (sum w^2, sum u^2); with
        ``clip_norm`` / ``skip_nonfinite`` it needs ``finish_norm`` first (it reads the coefficient and the skip)."""
        n = self._check_range(grad, lo)
        if self.w.is_cuda:
            i0, i1 = self._item_range(lo, n)
            rc = _lib.lib().tony_lamb_norm(self.w.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), grad.data_ptr(),
                                           int(grad.dtype == torch.bfloat16), lo, self._items.data_ptr() + 16 * i0,
                                           i1 - i0, self._adapt.data_ptr(), self._item_part.data_ptr() + 8 * i0,
                                           self._hp_dev.data_ptr(), self._ctl_ptr(), _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_lamb_norm")
            return
        if self._skipped_now():
            return
        gsc = _f32(_f32(self.grad_scale) * self._coef_now())
        for k, a, b, t in self._segs_in(lo, n):
            g = grad[a - lo:b - lo].float() * gsc
            self.m[a:b].mul_(self.b1).add_(g, alpha=1 - self.b1)
            self.v[a:b].mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            u = self._u_cpu(a, b, _f32(self.weight_decay) if self.segments.adapt[t] else 0.0)
            self._seg_part[k, 0] = self.w[a:b].double().square().sum()
            self._seg_part[k, 1] = u.double().square().sum()

    def _ratio_cpu(self, sw, su, coef):
        wn, un = sw ** 0.5, su ** 0.5
        return _f32(wn / un) if wn > 0.0 and un > 0.0 else 1.0

    def apply_range(self, grad: torch.Tensor, lo: int = 0, out_bf16: torch.Tensor | None = None):
        """``w -= lr ratio_t u`` over master elements [lo, lo + grad.numel()): the gradient itself was consumed by
        ``norm_range`` and is not read again."""
        n = self._check_range(grad, lo)
        if self.w.is_cuda:
            i0, i1 = self._item_range(lo, n)
            rc = _lib.lib().tony_lamb_apply(
                self.w.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                0 if self.ema is None else self.ema.data_ptr(), _lib.ptr(out_bf16), lo,
                self._items.data_ptr() + 16 * i0, i1 - i0, self.table.data_ptr(), self._hp_dev.data_ptr(),
                0 if self._xhp_dev is None else self._xhp_dev.data_ptr(), self._ctl_ptr(),
                _lib.stream_ptr(self.w.device))
            _lib.check(rc, "tony_lamb_apply")
            return
        if self._skipped_now():
            return
        for _, a, b, t in self._segs_in(lo, n):
            ratio, wd = self.table[t, 0].item(), self.table[t, 1].item()
            self.w[a:b].add_(self._u_cpu(a, b, wd), alpha=-_f32(_f32(self.lr) * ratio))
            if out_bf16 is not None:
                out_bf16[a - lo:b - lo].copy_(self.w[a:b])
        self._ema_cpu(lo, n)


def grad_stats(grad: torch.Tensor):
    """Return a device tensor [sum(g^2), any_nonfinite] for a flat gradient (H12)."""
    if grad.is_cuda:
        out = torch.empty(2, dtype=torch.float32, device=grad.device)
        rc = _lib.lib().tony_grad_stats(grad.data_ptr(), int(grad.dtype == torch.bfloat16), grad.numel(),
                                        out.data_ptr(), _lib.stream_ptr(grad.device))
        _lib.check(rc, "tony_grad_stats")
        return out
    g = grad.float()
    return torch.stack([(g * g).sum(), (~torch.isfinite(g)).any().float()])
