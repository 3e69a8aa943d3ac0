"""MXNet-style key-value store (``mx.kv``) for jobs launched by TonY's mxnet runtime.

TonY's mxnet runtime (T/runtime/MXNetRuntime.java:44-66) starts ``scheduler``,
``server`` and ``worker`` tasks with ``DMLC_ROLE / DMLC_PS_ROOT_URI /
DMLC_PS_ROOT_PORT / DMLC_NUM_SERVER / DMLC_NUM_WORKER``; the reference job
(EX/linearregression-mxnet/src/mxnet_dist_ex.py:35,61-68) trains through
``mx.kv.create('dist_async')``.  MXNet/ps-lite are not part of this stack, so
this module implements the kvstore semantics itself:

``local`` / ``device``
    one process; ``push`` sums the pushed list, the updater (if set) runs on
    the stored value, ``pull`` copies it out.
``dist_sync``
    servers own the keys (key id mod #servers).  A push round completes when
    every worker has pushed a key; the server then applies the optimizer to
    the *sum* (or stores the sum), and a worker's pull issued after its own
    push waits for that round -- the BSP semantics of ps-lite's sync mode.
``dist_async``
    every push is applied on arrival; pulls return the current value.
``dist_device_sync``
    no servers in the data path: the workers all-reduce the pushed gradients
    with RCCL (the xGMI path for GPU tensors) and run the same updater on
    every worker (replicated, deterministic).

Transport for the server modes: one torch.distributed (gloo) group over
servers + workers; the scheduler task hosts its TCPStore on
``DMLC_PS_ROOT_PORT`` and exits when every member has finished.  Requests are
an int64 header ``[op, key, numel, dtype]`` followed by the payload.

GPU payload plane (``TONY_KV_PLANE=xgmi``, the default when every member sees a GPU): every member
allocates an IPC-mapped window on its GPU (csrc/ps_plane.hip) and maps its peers' -- a worker the
servers', a server the workers'.  A pushed GPU tensor is stored by a copy kernel straight into its
row of the owning server's window and only the header goes over gloo; the server replies to a pull
by storing the value into the worker's landing area.  Neither side waits on the host: every copy
kernel's workgroups add to a u32 counter in the consumer's window header after their bytes
(``tony_kv_copy_flag``), and the consumer's stream waits on the device for the counter to reach the
copy's cumulative total (``tony_kv_wait``, bounded by ``TONY_KV_WAIT_S``; a timeout sets the window's
error word, which ``barrier`` / ``close`` raise) before the kernel that reads the bytes.  The payload
bytes never leave the GPUs (xGMI between devices; the server may share a worker's GPU, like TonY's
0-GPU ps).  Keys that do not fit the windows (``TONY_KV_WINDOW_MB``) or the flag tables, and CPU
tensors, keep the gloo payload.  A worker re-pushing a key before pulling it (its last row may not have
been read yet) sends that push over gloo: the pull's reply is what orders the server's read of the row
before the worker's next store into it (the server reads the row on its stream before it stores the
reply; the worker's next push is issued behind its wait for that reply).

Gradient compression (``set_gradient_compression({'type': '2bit', 'threshold': thr})``, the dist modes): every
worker keeps an fp32 residual ``r`` per fp32 key on the gradient's device, zero before the first compressed push.
A push of ``g`` (a list summed first) forms ``t = r + g`` and sends one of three codes per element: 1 when
``t >= thr`` (``r = t - thr``), 2 when ``t <= -thr`` (``r = t + thr``), else 0 (``r = t``; a NaN ``t`` compares
false twice) -- each line one fp32 operation.  Element ``i`` is bits ``2 * (i & 15)`` and the next of
little-endian u32 word ``i >> 4``; a push carries ``ceil(n / 16)`` words, the unused pairs of the last one 0.
The receiver decodes 0 / 1 / 2 to ``0.0`` / ``+thr`` / ``-thr`` (code 3, never produced, to ``0.0``) and merges
the fp32 values as it merges plain pushes, so the optimizer sees the sum of the decoded pushes; pulls are never
compressed and keys of another dtype are pushed as without it.  On the plane one kernel quantises, updates the
residual and stores the words straight into the worker's row of the server's window (``tony_kv_quant2``, counted
on the key's push flag by ``tony_kv_quant_blocks(n)`` workgroups: 0.25 B per element cross the link in place of
4), and the server's read of the row decodes it (``tony_kv_dequant2``); a push that keeps the gloo payload sends
the words.  ``dist_device_sync`` all-gathers the words and every worker sums the decoded pushes in rank order.
The call is collective over the workers like ``set_optimizer`` (rank 0 ships the setting to the servers) and is
allowed until the first push; a store that never gets it takes none of this code.

Row-sparse keys (``RowSparse``, ``row_sparse_pull``): a key whose ``init`` value is a ``RowSparse`` is a sparse key;
its stored value is the dense ``[R, ...]`` tensor.  ``RowSparse(indices, data, shape)`` names ``nnz`` rows by int64
``indices``, strictly increasing and in ``[0, R)`` (checked at construction: one host synchronisation for GPU
tensors, before any kernel); ``RowSparse.from_rows`` builds one from unsorted ids with duplicates (stable sort, the
duplicates of a row summed in order of occurrence, one fp32 add each).  A sparse key is pushed ``RowSparse`` values
only, a dense key tensors only (``TypeError`` otherwise); ``pull(ignore_sparse=True)`` skips sparse keys,
``ignore_sparse=False`` pulls them dense; ``row_sparse_pull(key, out, row_ids)`` leaves the sorted unique
``row_ids`` in ``out.indices`` and those rows of the stored value in ``out.data`` (out-of-range ids: ``ValueError``
on the caller, nothing sent), and in ``dist_sync`` waits for the worker's own pushed round as ``pull`` does.
Merging is fully ordered: a pushed list in list order, a ``dist_sync`` round in worker order, ``dist_device_sync``
in rank order; the merged index set is the sorted union and a merged row is ``acc = first source having it; acc =
acc + next source having it; ...``, one fp32 add each.  With no optimizer the store takes the merged push as its
value (rows not pushed become zero); with one, only the merged rows of the weight and of the optimizer's state
(dense ``[R, ...]``, zero at first use) change -- every other row keeps its bits.  Lazy SGD, per element of a
touched row, every line one separately rounded fp32 operation (no contraction)::

    g1 = g * rescale_grad
    g2 = clip_gradient is None ? g1 : (g1 > c ? c : (g1 < -c ? -c : g1))   # a NaN stays NaN
    p  = wd * w ;  g3 = g2 + p
    momentum == 0:  s = lr * g3 ; w = w - s
    momentum != 0:  m = momentum * m ; s = lr * g3 ; m = m - s ; w = w + m

fp32 GPU keys whose rows are a multiple of 16 B run this in one kernel (``tony_kv_rsp_sgd``), their merges in
``tony_kv_rsp_merge`` and their row reads in ``tony_kv_rsp_gather``; lazy Adam, CPU keys and other dtypes or row
lengths gather the touched rows of weight and state, run ``Optimizer.update`` on them and scatter them back (Adam's
``t`` counts updates of the key).  On the wire a sparse push is the header (``numel`` = ``nnz``), the ids, the rows;
on the plane the worker stores rows, then ids, into its row of the server's window (two flagged copies) when
``nnz * row_bytes + pad16(8 * nnz) <= pad16(key bytes)`` and the key's row is known to be read, else over gloo;
``nnz == 0`` sends the header only.  A ``row_sparse_pull`` sends its unique ids over gloo (8 B per row against
``row_bytes``; the host needs ``nnz`` anyway: one synchronisation per call) and the server gathers the rows straight
into the worker's landing area, counted on the worker's reply flag; the ordering rules of the dense pull apply
unchanged.  ``dist_device_sync`` all-gathers ``nnz``, then ids and rows padded to the largest.  A ``RowSparse`` push
ignores the gradient-compression setting, as MXNet's does.  A store that never sees a ``RowSparse`` runs none of this.

Fused optimizer kinds (``nag``, ``adagrad``, ``rmsprop`` plain and ``centered=True``, ``ftrl``), dense and lazy.  Their
contract is fixed to the bit as lazy SGD's is: per element, every line below is one separately rounded fp32 operation
(no contraction); ``sqrt`` and ``/`` are the correctly rounded ones; a constant such as ``1 - gamma1`` is formed in
double on the host and rounded once to fp32; a NaN stays a NaN (its sign and payload are no part of the contract).
``g1``, ``g2`` are lazy SGD's (the rescale, then the clip in its comparison form).

``nag`` (state ``mom`` when momentum != 0; at momentum 0 the lines of lazy SGD at momentum 0)::

    p  = wd * w ;  g3 = g2 + p
    m  = momentum * m ;  m = m + g3
    q  = momentum * m ;  g4 = g3 + q
    s  = lr * g4 ;  w = w - s

``adagrad`` (state ``history``; ``epsilon`` 1e-7 by default)::

    q = g2 * g2 ;  h = h + q
    e = h + eps ;  r = sqrt(e) ;  d = g2 / r
    p = wd * w ;  u = d + p
    s = lr * u ;  w = w - s

``rmsprop`` (state ``n``; ``gamma1`` 0.9, ``epsilon`` 1e-8)::

    p = wd * w ;  g3 = g2 + p
    q = g3 * g3 ;  a = (1-gamma1) * q ;  b = gamma1 * n ;  n = a + b
    e = n + eps ;  r = sqrt(e) ;  d = g3 / r
    s = lr * d ;  w = w - s

``rmsprop`` with ``centered=True`` (states ``n``, ``g``, ``delta``; ``gamma2`` 0.9): ``n`` as above, then::

    c  = (1-gamma1) * g3 ;  b2 = gamma1 * gb ;  gb = c + b2
    gg = gb * gb ;  e1 = n - gg ;  e = e1 + eps
    r  = sqrt(e) ;  d = g3 / r ;  s = lr * d
    dl = gamma2 * delta ;  delta = dl - s ;  w = w + delta

``ftrl`` (states ``z``, ``n``; ``lamda1`` 0.01, ``beta`` 1.0; ``wd`` enters only the denominator)::

    q  = g2 * g2 ;  n1 = n + q
    r1 = sqrt(n1) ;  r0 = sqrt(n) ;  dr = r1 - r0
    sg = dr / lr ;  t = sg * w
    z1 = z + g2 ;  z = z1 - t ;  n = n1
    |z| <= lamda1 :  w = +0.0
    else:            num = copysign(lamda1, z) - z
                     b1 = beta + r1 ;  d0 = b1 / lr ;  den = d0 + wd
                     w = num / den                  # a NaN z fails the comparison: the division carries it on

A contiguous, 16-byte aligned fp32 GPU key with an fp32 gradient runs its update in one launch (``tony_kv_opt_dense``,
csrc/kv_optim.hip), and the merged push of a row-sparse fp32 GPU key whose rows are a multiple of 16 B in one launch
on its touched rows (``tony_kv_opt_rows``); CPU tensors, other dtypes (computed in fp32, rounded once on the store)
and other row lengths run the same lines as separate torch operations, a row-sparse key through the gather / update /
scatter of lazy Adam.  Lazy updates are lazy SGD's: only the merged rows of the weight and of every state tensor
(dense ``[R, ...]`` fp32, zero at first use) change.  ``sgd`` and ``adam`` run none of this, and a store that is never
given one of these kinds runs none of it either.
"""
from __future__ import annotations

import datetime
import json
import os
import time
from typing import Dict, List, Optional, Union

import torch
import torch.distributed as dist

OP_INIT, OP_PUSH, OP_PULL, OP_OPT, OP_STOP, OP_PUSH_X, OP_PULL_X = range(7)  # _X: payload on the GPU plane
# gradient compression: the setting (JSON, like OP_OPT), a 2-bit push with its words over gloo (the header keeps
# the gradient's numel; the payload is ceil(numel / 16) int32 words) and one with its words on the GPU plane
OP_GC, OP_PUSH_C, OP_PUSH_CX = 7, 8, 9
# row-sparse keys (numel carries nnz): init of a sparse key (the dense payload, then int64 [R]); a push over gloo
# (int64 [ids..., row elements], then the rows) and on the GPU plane; a row_sparse_pull answered over gloo and on
# the plane (both: the ids follow the header over gloo)
OP_INIT_RSP, OP_PUSH_RSP, OP_PUSH_RSPX, OP_PULL_RSP, OP_PULL_RSPX = 10, 11, 12, 13, 14
TAG_HDR, TAG_DATA, TAG_REPLY = 1, 2, 3
_DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.uint8]
_EXIT_KEY = "tony/kv/exited"


def _dcode(dt: torch.dtype) -> int:
    return _DTYPES.index(dt)


# -- optimizers (server- or worker-side updater) -----------------------------------------------
def _f32(x: float) -> torch.Tensor:
    """A hyperparameter as the kernels see it: formed in double, rounded once to fp32."""
    return torch.tensor(float(x), dtype=torch.float32)


def _sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root.  On a GPU that is ``torch.sqrt`` (held to the contract bit for bit by
    tests/test_kv_optim_gpu.py).  ``torch.sqrt`` of a contiguous CPU tensor goes through a vector math
    library that is off by an ulp now and then; there the root is taken in double and rounded to fp32, which is the
    correctly rounded one for any faithful double root (scaled to [1, 2), the exact root of an fp32 number is never
    within 2^-50 of the midpoint of two fp32 numbers -- the square of a midpoint k 2^-24 differs from the number by a
    multiple of 2^-48 -- and a faithful double root is within 2^-52 of the exact one)."""
    return torch.sqrt(x) if x.is_cuda else x.double().sqrt().float()


class Optimizer:
    """``mx.optimizer`` subset: sgd (momentum, wd, rescale_grad, clip_gradient) and adam, and the kinds whose
    contract is fixed to the bit (module docstring): nag, adagrad, rmsprop (plain and ``centered``) and ftrl."""

    _FUSED = {"nag": 0, "adagrad": 1, "rmsprop": 2, "ftrl": 4}  # the kinds of csrc/kv_optim.hip (3: centered rmsprop)
    _EPSILON = {"adagrad": 1e-7}  # the default of a kind when ``epsilon`` is not given (every other kind: 1e-8)

    def __init__(self, name: str = "sgd", learning_rate: float = 0.01, momentum: float = 0.0, wd: float = 0.0,
                 rescale_grad: float = 1.0, clip_gradient: Optional[float] = None, beta1: float = 0.9,
                 beta2: float = 0.999, epsilon: Optional[float] = None, gamma1: float = 0.9, gamma2: float = 0.9,
                 centered: bool = False, lamda1: float = 0.01, beta: float = 1.0):
        self.name = name.lower()
        if self.name not in ("sgd", "adam") and self.name not in self._FUSED:
            raise ValueError(f"unsupported optimizer {name!r}")
        if centered and self.name != "rmsprop":
            raise ValueError(f"centered=True is an option of rmsprop, not of {self.name!r}")
        if epsilon is None:
            epsilon = self._EPSILON.get(self.name, 1e-8)
        self.cfg = dict(name=self.name, learning_rate=learning_rate, momentum=momentum, wd=wd,
                        rescale_grad=rescale_grad, clip_gradient=clip_gradient, beta1=beta1, beta2=beta2,
                        epsilon=epsilon)
        if self.name in self._FUSED:  # (sgd and adam keep exactly the keys they had)
            for k, v in (("lamda1", lamda1), ("epsilon", epsilon), ("gamma1", gamma1), ("gamma2", gamma2)):
                if not float(v) >= 0.0:
                    raise ValueError(f"{self.name}: {k} must not be negative, not {v!r}")
            self.cfg.update(gamma1=gamma1, gamma2=gamma2, centered=bool(centered), lamda1=lamda1, beta=beta)
        else:  # sgd and adam have none of these: a value given to them would be dropped without a word
            for k, v, default in (("gamma1", gamma1, 0.9), ("gamma2", gamma2, 0.9), ("lamda1", lamda1, 0.01),
                                  ("beta", beta, 1.0)):
                if v != default:
                    raise ValueError(f"{k} is not a hyperparameter of {self.name!r}")
        self.state: Dict[int, dict] = {}
        self.kernel_ops = [0, 0]  # tony_kv_opt_dense / tony_kv_opt_rows launches (tests)
        self._scalars: Dict[torch.device, tuple] = {}  # _fused_math's fp32 scalars per device (and the cfg they hold)

    def to_json(self) -> str:
        return json.dumps(self.cfg)

    @classmethod
    def from_json(cls, s: str) -> "Optimizer":
        return cls(**json.loads(s))

    def _state_names(self) -> tuple:
        """The names of the state tensors a fused kind's setting keeps per key (``_ROW_STATE``: every one a kind may
        keep)."""
        names = self._ROW_STATE[self.name]
        if self.name == "nag":
            return names if self.cfg["momentum"] else ()
        if self.name == "rmsprop" and not self.cfg["centered"]:
            return names[:1]
        return names

    def _fused_args(self) -> tuple:
        """The kind and the hyperparameters of ``tony_kv_opt_dense`` / ``tony_kv_opt_rows`` (csrc/kv_optim.hip)."""
        c = self.cfg
        clip = c["clip_gradient"]
        kind = 3 if c.get("centered") else self._FUSED[self.name]
        return kind, (c["learning_rate"], c["wd"], c["rescale_grad"], int(clip is not None),
                      0.0 if clip is None else clip, c["momentum"], c["epsilon"], c["gamma1"], 1 - c["gamma1"],
                      c["gamma2"], c["lamda1"], c["beta"])

    def _fused_math(self, w: torch.Tensor, st: Dict[str, torch.Tensor], g: torch.Tensor) -> torch.Tensor:
        """The contract of the module docstring as a torch composition on fp32 tensors of one shape: every op one
        rounding, every hyperparameter an fp32 scalar.  Returns the new weight; the new states replace ``st``'s."""
        c = self.cfg
        # the scalars live on the tensors' device (torch divides by a CPU scalar as a product with its reciprocal) and
        # are made once per device and setting, not copied there on every update
        sig, k = self._scalars.get(w.device, (None, None))
        if sig != tuple(c.values()):
            k = {n: _f32(v).to(w.device) for n, v in c.items()
                 if isinstance(v, (int, float)) and not isinstance(v, bool)}
            k["omg1"] = _f32(1 - c["gamma1"]).to(w.device)
            self._scalars[w.device] = (tuple(c.values()), k)
        lr, wd = k["learning_rate"], k["wd"]
        g2 = g * k["rescale_grad"]
        if c["clip_gradient"] is not None:
            cl = k["clip_gradient"]
            g2 = torch.where(g2 > cl, cl, torch.where(g2 < -cl, -cl, g2))  # a NaN stays NaN
        if self.name == "nag":
            g3 = g2 + wd * w
            if not c["momentum"]:
                return w - lr * g3
            mom = k["momentum"]
            m = mom * st["mom"]
            m = m + g3
            st["mom"] = m
            g4 = g3 + mom * m
            return w - lr * g4
        if self.name == "adagrad":
            h = st["history"] + g2 * g2
            st["history"] = h
            r = _sqrt_rn(h + k["epsilon"])
            u = g2 / r + wd * w
            return w - lr * u
        if self.name == "rmsprop":
            g1, omg, eps = k["gamma1"], k["omg1"], k["epsilon"]
            g3 = g2 + wd * w
            a = omg * (g3 * g3)
            n = a + g1 * st["n"]
            st["n"] = n
            if not c["centered"]:
                return w - lr * (g3 / _sqrt_rn(n + eps))
            cc = omg * g3
            gb = cc + g1 * st["g"]
            st["g"] = gb
            e = (n - gb * gb) + eps
            s = lr * (g3 / _sqrt_rn(e))
            delta = k["gamma2"] * st["delta"] - s
            st["delta"] = delta
            return w + delta
        l1, beta = k["lamda1"], k["beta"]  # ftrl
        n1 = st["n"] + g2 * g2
        r1 = _sqrt_rn(n1)
        sg = (r1 - _sqrt_rn(st["n"])) / lr
        z = (st["z"] + g2) - sg * w
        st["z"], st["n"] = z, n1
        den = (beta + r1) / lr + wd
        return torch.where(z.abs() <= l1, torch.zeros_like(z), (torch.copysign(l1, z) - z) / den)

    def _update_fused(self, key: int, weight: torch.Tensor, grad: torch.Tensor) -> None:
        """``update`` of nag / adagrad / rmsprop / ftrl: one ``tony_kv_opt_dense`` launch on a contiguous, 16-byte
        aligned fp32 GPU key with an fp32 gradient, else the torch composition (other dtypes compute in fp32 and
        round once on the store)."""
        if grad.numel() != weight.numel():  # (the kernel would read the gradient's allocation to the key's length)
            raise ValueError(f"key {key}: a gradient of {grad.numel()} elements for a value of {weight.numel()}")
        st = self.state.setdefault(key, {"t": 0})
        names = self._state_names()
        for n in names:
            if n not in st:
                st[n] = torch.zeros(weight.shape, dtype=torch.float32, device=weight.device)
        if (weight.is_cuda and weight.dtype == torch.float32 and grad.dtype == torch.float32
                and weight.is_contiguous() and weight.data_ptr() % 16 == 0 and grad.device == weight.device
                and self._kernel_states(st, names, weight)):
            from ..ops import _lib

            if not weight.numel():
                return
            g = _aligned16(grad)
            kind, hp = self._fused_args()
            ptrs = [st[n].data_ptr() for n in names] + [None] * (3 - len(names))
            with torch.cuda.device(weight.device):
                _lib.check(_lib.lib().tony_kv_opt_dense(kind, weight.data_ptr(), *ptrs, g.data_ptr(), weight.numel(),
                                                        *hp, _lib.stream_ptr(weight.device)), "tony_kv_opt_dense")
            self.kernel_ops[0] += 1
            return
        self._update_torch(st, names, weight, grad)

    @staticmethod
    def _kernel_states(st: dict, names, weight: torch.Tensor) -> bool:
        """Whether the kernels take the state tensors ``names``: fp32 of the weight's shape on its device, contiguous
        and 16-byte aligned (a state restored from a file may be anything)."""
        return all(st[n].device == weight.device and st[n].dtype == torch.float32 and st[n].shape == weight.shape
                   and st[n].is_contiguous() and st[n].data_ptr() % 16 == 0 for n in names)

    def _update_torch(self, st: dict, names, weight: torch.Tensor, grad: torch.Tensor) -> None:
        """The fused kinds' update of ``weight`` and the states ``names`` of ``st`` as the torch composition."""
        new = {n: st[n] for n in names}
        w = self._fused_math(weight.float(), new, grad.float().reshape(weight.shape))
        weight.copy_(w)
        for n in names:
            st[n].copy_(new[n])

    def update(self, key: int, weight: torch.Tensor, grad: torch.Tensor) -> None:
        if self.name in self._FUSED:
            self._update_fused(key, weight, grad)
            return
        c = self.cfg
        g = grad.float() * c["rescale_grad"]
        if c["clip_gradient"] is not None:
            g.clamp_(-c["clip_gradient"], c["clip_gradient"])
        w = weight if weight.dtype == torch.float32 else weight.float()
        g.add_(w, alpha=c["wd"])
        st = self.state.setdefault(key, {"t": 0})
        lr = c["learning_rate"]
        if self.name == "sgd":
            if c["momentum"]:
                m = st.setdefault("mom", torch.zeros_like(w))
                m.mul_(c["momentum"]).add_(g, alpha=-lr)
                w.add_(m)
            else:
                w.add_(g, alpha=-lr)
        else:
            st["t"] += 1
            m = st.setdefault("m", torch.zeros_like(w))
            v = st.setdefault("v", torch.zeros_like(w))
            m.mul_(c["beta1"]).add_(g, alpha=1 - c["beta1"])
            v.mul_(c["beta2"]).addcmul_(g, g, value=1 - c["beta2"])
            t = st["t"]
            lr_t = lr * (1 - c["beta2"] ** t) ** 0.5 / (1 - c["beta1"] ** t)
            w.addcdiv_(m, v.sqrt().add_(c["epsilon"]), value=-lr_t)
        if w is not weight:
            weight.copy_(w)

    _ROW_STATE = {"sgd": ("mom",), "adam": ("m", "v"), "nag": ("mom",), "adagrad": ("history",),
                  "rmsprop": ("n", "g", "delta"), "ftrl": ("z", "n")}

    def _row_state(self, key: int, weight: torch.Tensor):
        """A sparse key's state and the names of its tensors: dense fp32 ``[R, ...]``, zero at first use."""
        st = self.state.setdefault(key, {"t": 0})
        if self.name in self._FUSED:
            names = list(self._state_names())
        else:
            names = [n for n in self._ROW_STATE[self.name] if self.name == "adam" or self.cfg["momentum"]]
        for n in names:
            if n not in st:
                st[n] = torch.zeros(weight.shape, dtype=torch.float32, device=weight.device)
        return st, names

    def update_rows(self, key: int, weight: torch.Tensor, ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        """The lazy update of a row-sparse key (module docstring): rows ``ids`` (sorted, unique, in range) of the
        dense ``weight`` [R, ...] and of its state from the compact ``grad_rows``; every other row keeps its bits."""
        c = self.cfg
        re = _row_elems(weight.shape)
        if self.name in self._FUSED and (ids.dim() != 1 or grad_rows.numel() != ids.numel() * re):
            raise ValueError(f"key {key}: {grad_rows.numel()} gradient elements for {ids.numel()} rows of {re}")
        st, names = self._row_state(key, weight)
        if (self.name == "sgd" and _rsp_kernel_rows(weight, re) and weight.is_contiguous()
                and weight.data_ptr() % 16 == 0 and grad_rows.dtype == torch.float32):
            from ..ops import _lib

            if not ids.numel():  # no row to touch (and no address of an empty tensor to hand to a launcher)
                return
            ids, g = _aligned16(ids), _aligned16(grad_rows)
            mom = st["mom"].data_ptr() if names else None
            clip = c["clip_gradient"]
            with torch.cuda.device(weight.device):
                _lib.check(_lib.lib().tony_kv_rsp_sgd(
                    weight.data_ptr(), mom, ids.data_ptr(), g.data_ptr(), ids.numel(), re, weight.shape[0],
                    c["learning_rate"], c["momentum"], c["wd"], c["rescale_grad"], int(clip is not None),
                    0.0 if clip is None else clip, _lib.stream_ptr(weight.device)), "tony_kv_rsp_sgd")
            return
        if (self.name in self._FUSED and _rsp_kernel_rows(weight, re) and weight.is_contiguous()
                and weight.data_ptr() % 16 == 0 and grad_rows.dtype == torch.float32 and ids.dtype == torch.int64
                and ids.device == weight.device and grad_rows.device == weight.device
                and self._kernel_states(st, names, weight)):
            from ..ops import _lib

            if not ids.numel():
                return
            ids, g = _aligned16(ids), _aligned16(grad_rows)
            kind, hp = self._fused_args()
            ptrs = [st[n].data_ptr() for n in names] + [None] * (3 - len(names))
            with torch.cuda.device(weight.device):
                _lib.check(_lib.lib().tony_kv_opt_rows(
                    kind, weight.data_ptr(), *ptrs, ids.data_ptr(), g.data_ptr(), ids.numel(), re, weight.shape[0],
                    *hp, _lib.stream_ptr(weight.device)), "tony_kv_opt_rows")
            self.kernel_ops[1] += 1
            return
        self.update_rows_generic(key, weight, ids, grad_rows)

    def update_rows_generic(self, key: int, weight: torch.Tensor, ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        """``update_rows`` for any optimizer, device and dtype: the touched rows of weight and state gathered,
        the dense update's math on them, scattered back."""
        st, names = self._row_state(key, weight)
        rows = Optimizer(**self.cfg)
        rows.state[key] = {"t": st["t"], **{n: st[n].index_select(0, ids) for n in names}}
        w = weight.index_select(0, ids)
        rows.update(key, w, grad_rows)
        weight.index_copy_(0, ids, w)
        for n in names:
            st[n].index_copy_(0, ids, rows.state[key][n])
        st["t"] = rows.state[key]["t"]

    def state_dict(self):
        return {"cfg": self.cfg, "state": self.state}


def create_optimizer(name: str = "sgd", **kw) -> Optimizer:
    return Optimizer(name, **kw)


def _as_list(v) -> List[torch.Tensor]:
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _merge(vals: List[torch.Tensor]) -> torch.Tensor:
    out = vals[0].detach().clone()
    for v in vals[1:]:
        out.add_(v.to(out.device))
    return out


# -- 2-bit gradient compression (module docstring) ----------------------------------------------
def _gc_threshold(params) -> Optional[float]:
    """The threshold a ``set_gradient_compression`` request asks 2-bit compression for; None for no compression."""
    if not isinstance(params, dict):
        raise ValueError("gradient compression parameters must be a dict")
    unknown = sorted(set(params) - {"type", "threshold"})
    if unknown:
        raise ValueError(f"unknown gradient compression parameters {unknown}")
    kind = params.get("type")
    if kind is not None and not isinstance(kind, str):
        raise ValueError(f"gradient compression type must be '2bit', 'none' or None, not {kind!r}")
    try:
        thr = float(torch.tensor(float(params.get("threshold", 0.5)), dtype=torch.float32))  # as the kernels see it
    except (TypeError, ValueError):
        raise ValueError(f"gradient compression threshold {params.get('threshold')!r} is not a number") from None
    if not 0.0 < thr < float("inf"):
        raise ValueError(f"gradient compression threshold must be a positive fp32 number, not {params['threshold']!r}")
    if kind in (None, "none"):
        return None
    if kind != "2bit":
        raise NotImplementedError(f"gradient compression type {kind!r} is not supported by this kvstore")
    return thr


def _gc_words(n: int) -> int:
    return (n + 15) // 16


def _quant2_torch(g: torch.Tensor, r: torch.Tensor, thr: float) -> torch.Tensor:
    """The 2-bit push of flat fp32 ``g`` on the CPU: ``r`` updated in place, the packed int32 words returned."""
    th = torch.tensor(thr, dtype=torch.float32)
    t = r + g
    pos, neg = t >= th, t <= -th
    r.copy_(torch.where(pos, t - th, torch.where(neg, t + th, t)))
    code = pos.to(torch.int64) + 2 * neg.to(torch.int64)
    code = torch.nn.functional.pad(code, (0, -code.numel() % 16)).view(-1, 16)
    w = (code << (2 * torch.arange(16))).sum(1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def _dequant2_torch(words: torch.Tensor, n: int, thr: float) -> torch.Tensor:
    """The fp32 values of ``n`` elements packed in int32 ``words`` (CPU)."""
    lut = torch.tensor([0.0, thr, -thr, 0.0], dtype=torch.float32)
    codes = (words.to(torch.int64).view(-1, 1) >> (2 * torch.arange(16))) & 3
    return lut[codes.reshape(-1)[:n]]


def _quant2_gpu(g: torch.Tensor, r: torch.Tensor, thr: float, dst: Optional[int] = None,
                flag: Optional[int] = None) -> Optional[torch.Tensor]:
    """``tony_kv_quant2`` of flat fp32 ``g`` (16-B aligned) on its device's stream: the words to the device
    address ``dst`` (counted on ``flag``), or into a new int32 tensor, which is returned."""
    from ..ops import _lib

    words = None
    if dst is None:
        words = torch.empty(_gc_words(g.numel()), dtype=torch.int32, device=g.device)
        dst = words.data_ptr()
    with torch.cuda.device(g.device):
        _lib.check(_lib.lib().tony_kv_quant2(dst, g.data_ptr(), r.data_ptr(), g.numel(), thr, flag,
                                             _lib.stream_ptr(g.device)), "tony_kv_quant2")
    return words


def _dequant2_gpu(words: torch.Tensor, n: int, thr: float, nsrc: int = 1) -> torch.Tensor:
    """``tony_kv_dequant2``: the ordered fp32 sum of ``nsrc`` packed pushes, back to back in int32 ``words``."""
    from ..ops import _lib

    out = torch.empty(n, dtype=torch.float32, device=words.device)
    with torch.cuda.device(words.device):
        _lib.check(_lib.lib().tony_kv_dequant2(out.data_ptr(), words.data_ptr(), n, thr, nsrc, _gc_words(n), None,
                                               _lib.stream_ptr(words.device)), "tony_kv_dequant2")
    return out


def _aligned16(g: torch.Tensor) -> torch.Tensor:
    g = g.contiguous()
    return g.clone() if g.data_ptr() % 16 else g  # the kernels move 16-B aligned addresses: a view at an odd offset


class _Residuals:
    """A worker's quantisation residual per key: fp32, on the gradient's device, zero before the first push."""

    def __init__(self):
        self.r: Dict[int, torch.Tensor] = {}

    def of(self, kid: int, g: torch.Tensor) -> torch.Tensor:
        r = self.r.get(kid)
        if r is None:
            r = self.r[kid] = torch.zeros_like(g)
        elif r.device != g.device:  # (the kernel must never see a residual of another device)
            r = self.r[kid] = r.to(g.device)
        return r

    def quantise(self, kid: int, g: torch.Tensor, thr: float) -> torch.Tensor:
        """The int32 words of pushing flat fp32 ``g`` (on its device), by the kernel on a GPU."""
        if g.is_cuda:
            g = _aligned16(g)
            return _quant2_gpu(g, self.of(kid, g), thr)
        return _quant2_torch(g, self.of(kid, g), thr)


# -- row-sparse values (module docstring) -------------------------------------------------------
class RowSparse:
    """``nnz`` rows of a dense ``shape`` tensor: int64 ``indices`` [nnz], strictly increasing and in
    ``[0, shape[0])``, and ``data`` [nnz, *shape[1:]] on the same device."""

    def __init__(self, indices: torch.Tensor, data: torch.Tensor, shape, _checked: bool = False):
        self.shape = tuple(int(d) for d in shape)
        if not self.shape or self.shape[0] < 0:
            raise ValueError(f"a RowSparse needs a shape of at least one dimension, not {shape!r}")
        if indices.dtype != torch.int64 or indices.dim() != 1:
            raise ValueError("RowSparse indices must be an int64 vector")
        if tuple(data.shape) != (indices.numel(),) + self.shape[1:]:
            raise ValueError(f"RowSparse data of shape {tuple(data.shape)} does not hold {indices.numel()} rows of "
                             f"shape {self.shape[1:]}")
        if indices.device != data.device:
            raise ValueError("RowSparse indices and data must be on the same device")
        if not _checked and indices.numel():
            bad = (indices[0] < 0) | (indices[-1] >= self.shape[0]) | (indices[1:] <= indices[:-1]).any()
            if bool(bad):  # (the one host synchronisation of a GPU value)
                raise ValueError(f"RowSparse indices must be strictly increasing and in [0, {self.shape[0]})")
        self.indices, self.data = indices, data

    @property
    def nnz(self) -> int:
        return self.indices.numel()

    def to_dense(self) -> torch.Tensor:
        out = torch.zeros(self.shape, dtype=self.data.dtype, device=self.data.device)
        if self.nnz:
            out.index_copy_(0, self.indices, self.data)
        return out

    @classmethod
    def from_rows(cls, ids: torch.Tensor, rows: torch.Tensor, shape) -> "RowSparse":
        """From unsorted ``ids`` with duplicates (an embedding's backward): stable sort, the rows of one id summed
        in order of occurrence as fp32 adds, left to right."""
        ids = ids.reshape(-1).to(torch.int64)
        shape = tuple(int(d) for d in shape)
        rows = rows.reshape((ids.numel(),) + shape[1:])
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= shape[0]):
            raise ValueError(f"row ids must be in [0, {shape[0]})")
        sid, order = torch.sort(ids, stable=True)
        uniq, counts = torch.unique_consecutive(sid, return_counts=True)
        starts = torch.cumsum(counts, 0) - counts
        acc = rows.index_select(0, order.index_select(0, starts)).float()
        for k in range(1, int(counts.max()) if ids.numel() else 0):
            sel = (counts > k).nonzero().reshape(-1)
            nxt = rows.index_select(0, order.index_select(0, starts.index_select(0, sel) + k)).float()
            acc.index_copy_(0, sel, acc.index_select(0, sel) + nxt)
        return cls(uniq, acc.to(rows.dtype), shape, _checked=True)


def _rsp_kernel_rows(t: torch.Tensor, row_elems: int) -> bool:
    """Whether the row-sparse kernels take rows of ``t``: fp32 on a GPU, the row a multiple of 16 B."""
    return t.is_cuda and t.dtype == torch.float32 and row_elems > 0 and row_elems % 4 == 0


def _row_elems(shape) -> int:
    n = 1
    for d in shape[1:]:
        n *= int(d)
    return n


def _unique_row_ids(row_ids: torch.Tensor, rows: int) -> torch.Tensor:
    """The sorted unique ids of a ``row_sparse_pull``; ``ValueError`` for one outside ``[0, rows)`` (one host
    synchronisation for a GPU tensor: the host needs their count anyway)."""
    ids = torch.unique(row_ids.reshape(-1).to(torch.int64))
    if ids.numel() and (int(ids[0]) < 0 or int(ids[-1]) >= rows):
        raise ValueError(f"row_sparse_pull: row ids must be in [0, {rows})")
    return ids


def _rsp_gather(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """Rows ``ids`` (sorted, in range, on the table's device) of the dense ``[R, ...]`` ``table``."""
    re = _row_elems(table.shape)
    if not (ids.numel() and _rsp_kernel_rows(table, re) and table.is_contiguous() and table.data_ptr() % 16 == 0):
        return table.index_select(0, ids)
    from ..ops import _lib

    ids = ids.contiguous()
    out = torch.empty((ids.numel(),) + tuple(table.shape[1:]), dtype=table.dtype, device=table.device)
    with torch.cuda.device(table.device):
        _lib.check(_lib.lib().tony_kv_rsp_gather(out.data_ptr(), table.data_ptr(), ids.data_ptr(), ids.numel(), 4 * re,
                                                 table.shape[0], None, None, _lib.stream_ptr(table.device)),
                   "tony_kv_rsp_gather")
    return out


def _rsp_merge(vals: List[RowSparse], device=None, dtype=None) -> RowSparse:
    """The ordered merge of row-sparse values (module docstring) on ``device`` (the first value's by default)."""
    first = vals[0]
    device = first.data.device if device is None else torch.device(device)
    dtype = first.data.dtype if dtype is None else dtype
    vals = [v if (v.data.device == device and v.data.dtype == dtype) else
            RowSparse(v.indices.to(device), v.data.to(device, dtype), v.shape, _checked=True) for v in vals]
    for v in vals[1:]:
        if v.shape != first.shape:
            raise ValueError(f"row-sparse values of shapes {first.shape} and {v.shape} cannot be merged")
    if len(vals) == 1:
        return vals[0]
    union = torch.unique(torch.cat([v.indices for v in vals]))
    re, nu = _row_elems(first.shape), union.numel()
    if nu and _rsp_kernel_rows(vals[0].data, re) and len(vals) <= _MAX_KV_WORKERS:
        import ctypes

        from ..ops import _lib

        srcs = [(_aligned16(v.indices), _aligned16(v.data)) for v in vals]
        out = torch.empty((nu,) + first.shape[1:], dtype=torch.float32, device=device)
        arr = ctypes.c_int64 * len(vals)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().tony_kv_rsp_merge(
                out.data_ptr(), union.data_ptr(), nu, arr(*[i.data_ptr() if i.numel() else 0 for i, _ in srcs]),
                arr(*[d.data_ptr() if d.numel() else 0 for _, d in srcs]), arr(*[i.numel() for i, _ in srcs]),
                len(vals), re, _lib.stream_ptr(device)), "tony_kv_rsp_merge")
        return RowSparse(union, out, first.shape, _checked=True)
    acc = torch.zeros((nu,) + first.shape[1:], dtype=torch.float32, device=device)
    have = torch.zeros(nu, dtype=torch.bool, device=device)
    for v in vals:
        if not v.nnz:
            continue
        pos = torch.searchsorted(union, v.indices)
        d = v.data.float()
        seen = have.index_select(0, pos).view((-1,) + (1,) * (d.dim() - 1))
        acc.index_copy_(0, pos, torch.where(seen, acc.index_select(0, pos) + d, d))
        have.index_fill_(0, pos, True)
    return RowSparse(union, acc.to(dtype), first.shape, _checked=True)


def _rsp_apply(opt: Optional["Optimizer"], kid: int, weight: torch.Tensor, merged: RowSparse) -> None:
    """A merged row-sparse push into the dense ``weight`` [R, ...] (module docstring)."""
    merged = _rsp_merge([merged], weight.device)
    if opt is None:
        weight.zero_()
        if merged.nnz:
            weight.index_copy_(0, merged.indices, merged.data.to(weight.dtype))
        return
    opt.update_rows(kid, weight, merged.indices, merged.data)


class _KeyIds:
    def __init__(self):
        self.ids: Dict[object, int] = {}

    def __call__(self, key) -> int:
        if isinstance(key, int):
            return key
        if key not in self.ids:
            self.ids[key] = len(self.ids) + (1 << 40)  # string keys live above int keys
        return self.ids[key]


# -- local ----------------------------------------------------------------------------------------
class KVStore:
    def __init__(self, kind: str = "local"):
        self.type = kind
        self._store: Dict[int, torch.Tensor] = {}
        self._opt: Optional[Optimizer] = None
        self._key = _KeyIds()
        self._sparse: Dict[int, tuple] = {}  # sparse keys (init with a RowSparse) -> their dense shape

    @property
    def rank(self) -> int:
        return 0

    @property
    def num_workers(self) -> int:
        return 1

    def _keys_vals(self, key, value):
        if isinstance(key, (list, tuple)):
            return list(key), list(value)
        return [key], [value]

    def init(self, key, value) -> None:
        for k, v in zip(*self._keys_vals(key, value)):
            self._store[self._key(k)] = self._init_value(self._key(k), v)

    def _init_value(self, kid: int, v) -> torch.Tensor:
        """The dense tensor a key starts from; a ``RowSparse`` value makes the key a sparse key."""
        v = _as_list(v)[0]
        if isinstance(v, RowSparse):
            self._sparse[kid] = v.shape
            return v.to_dense()
        return v.detach().clone()

    def _sparse_push(self, kid: int, vals: list) -> bool:
        """Whether ``vals`` is a row-sparse push of a sparse key; ``TypeError`` when value and key kinds differ."""
        rsp = [isinstance(v, RowSparse) for v in vals]
        if kid in self._sparse:
            if not all(rsp):
                raise TypeError(f"key {kid} is a row-sparse key: push RowSparse values to it")
            for v in vals:
                if v.shape != self._sparse[kid]:
                    raise ValueError(f"key {kid} has shape {self._sparse[kid]}, the pushed RowSparse {v.shape}")
            return True
        if any(rsp):
            raise TypeError(f"key {kid} is a dense key: a RowSparse cannot be pushed to it")
        return False

    def push(self, key, value, priority: int = 0) -> None:  # noqa: ARG002
        for k, v in zip(*self._keys_vals(key, value)):
            kid = self._key(k)
            if self._sparse_push(kid, _as_list(v)):
                self._apply_rsp(kid, _rsp_merge(_as_list(v)))
                continue
            g = _merge(_as_list(v))
            self._apply(kid, g)

    def _apply_rsp(self, kid: int, merged: "RowSparse") -> None:
        if kid not in self._store:
            raise KeyError(f"key {kid} was not initialised")
        _rsp_apply(self._opt, kid, self._store[kid], merged)

    def row_sparse_pull(self, key, out=None, row_ids=None, priority: int = 0) -> None:  # noqa: ARG002
        """``out.indices`` <- the sorted unique ``row_ids``, ``out.data`` <- those rows of the stored value (module
        docstring); ``out`` a ``RowSparse`` or a list of them per key, ``row_ids`` one tensor per ``out``."""
        keys, outs = self._keys_vals(key, out)
        rids = list(row_ids) if isinstance(key, (list, tuple)) else [row_ids]
        for k, o, r in zip(keys, outs, rids):
            kid = self._key(k)
            os_ = _as_list(o)
            rs = list(r) if isinstance(r, (list, tuple)) else [r] * len(os_)
            for dst, ids in zip(os_, rs):
                if not isinstance(dst, RowSparse):
                    raise TypeError("row_sparse_pull fills RowSparse values")
                shape = self._rsp_shape(kid, dst)
                ids = _unique_row_ids(ids, shape[0])
                dev = dst.data.device
                rows = self._pull_rows(kid, ids, shape, dst.data.dtype, dev)
                dst.indices, dst.data, dst.shape = ids.to(dev), rows.to(dev).view((ids.numel(),) + shape[1:]), shape

    def _rsp_shape(self, kid: int, dst: "RowSparse") -> tuple:  # noqa: ARG002
        if kid not in self._store:
            raise KeyError(f"key {kid} was not initialised")
        return tuple(self._store[kid].shape)

    def _pull_rows(self, kid: int, ids: torch.Tensor, shape: tuple, dtype, device) -> torch.Tensor:  # noqa: ARG002
        src = self._store[kid]
        return _rsp_gather(src, ids.to(src.device))

    def _apply(self, kid: int, merged: torch.Tensor) -> None:
        if kid not in self._store:
            raise KeyError(f"key {kid} was not initialised")
        if self._opt is not None:
            self._opt.update(kid, self._store[kid], merged.to(self._store[kid].device))
        else:
            self._store[kid].copy_(merged)

    def pull(self, key, out=None, priority: int = 0, ignore_sparse: bool = True):  # noqa: ARG002
        keys, outs = self._keys_vals(key, out)
        for k, o in zip(keys, outs):
            if ignore_sparse and self._key(k) in self._sparse:
                continue
            src = self._store[self._key(k)]
            for t in _as_list(o):
                t.copy_(src.to(t.device))

    def pushpull(self, key, value, out=None, priority: int = 0) -> None:
        self.push(key, value, priority)
        self.pull(key, out if out is not None else value, priority)

    def set_optimizer(self, optimizer: Optimizer) -> None:
        self._opt = optimizer

    def set_gradient_compression(self, params: dict) -> None:
        if _gc_threshold(params) is not None:  # a one-process store has no wire to compress
            raise NotImplementedError(f"gradient compression is not supported by a {self.type!r} kvstore")

    def barrier(self) -> None:
        pass

    def save_optimizer_states(self, fname: str, dump_optimizer: bool = False) -> None:  # noqa: ARG002
        if self._opt is None:
            raise RuntimeError("no optimizer set")
        torch.save({"cfg": json.dumps(self._opt.cfg), "state": self._opt.state}, fname)

    def load_optimizer_states(self, fname: str) -> None:
        sd = torch.load(fname, weights_only=True)
        self._opt = Optimizer.from_json(sd["cfg"])
        self._opt.state = sd["state"]

    def close(self) -> None:
        pass


# -- dist (servers) -------------------------------------------------------------------------------
def _env_int(name: str, default: int) -> int:
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default


class _Topology:
    def __init__(self):
        e = os.environ
        self.role = e.get("DMLC_ROLE", "worker")
        self.num_servers = _env_int("DMLC_NUM_SERVER", 0)
        self.num_workers = _env_int("DMLC_NUM_WORKER", 1)
        self.root_uri = e.get("DMLC_PS_ROOT_URI", "127.0.0.1")
        self.root_port = _env_int("DMLC_PS_ROOT_PORT", 0)
        self.index = _env_int("TASK_INDEX", 0)

    @property
    def world(self) -> int:
        return self.num_servers + self.num_workers

    @property
    def rank(self) -> int:
        return self.index if self.role == "server" else self.num_servers + self.index

    def server_of(self, kid: int) -> int:
        return kid % self.num_servers


def _connect(topo: _Topology, timeout_s: float = 1800.0) -> dist.TCPStore:
    return dist.TCPStore(topo.root_uri, topo.root_port, topo.world + 1, False,
                         timeout=datetime.timedelta(seconds=timeout_s))


def _init_group(topo: _Topology):
    store = _connect(topo)
    if not dist.is_initialized():
        dist.init_process_group("gloo", store=dist.PrefixStore("tony-kv", store), rank=topo.rank,
                                world_size=topo.world)
    workers = dist.new_group(list(range(topo.num_servers, topo.world)))
    return store, workers


def _pad16(n: int) -> int:
    return (n + 15) // 16 * 16


# device flag tables in a plane window's header (csrc/ps_plane.hip: the first 1 MiB is the PS plane's
# arrival table, unused by a kvstore process): a server's push counters [key slot][worker], a worker's
# reply counters [server][key slot]
_MAX_SLOTS, _MAX_KV_WORKERS = 4096, 64
_REPLY_FLAGS = 4 * _MAX_SLOTS * _MAX_KV_WORKERS


def _push_flag(slot: int, worker: int) -> int:
    return 4 * (slot * _MAX_KV_WORKERS + worker)


def _reply_flag(topo: "_Topology", server: int, slot: int) -> int:
    return _REPLY_FLAGS + 4 * (server * (_MAX_SLOTS // max(1, topo.num_servers)) + slot)


def _wait_budget_s() -> float:
    return float(os.environ.get("TONY_KV_WAIT_S", "300"))


def _plane_wanted() -> bool:
    mode = os.environ.get("TONY_KV_PLANE", "auto").lower()
    if mode in ("gloo", "0", "off"):
        return False
    if mode == "xgmi" and not torch.cuda.is_available():
        raise RuntimeError("TONY_KV_PLANE=xgmi but this task sees no GPU")
    return torch.cuda.is_available()


class _KvLayout:
    """Where each key's bytes live in the plane windows, computed identically by a server and every worker
    from the keys in init order (a server sees only its own keys, which is all its part depends on):
    server s's window holds, per key it owns, one receive row per worker; a worker's window is split in one
    landing region per server, each holding that server's keys back to back."""

    def __init__(self, topo: "_Topology", window_bytes: int):
        self.topo, self.bytes = topo, window_bytes
        self.region = window_bytes // max(1, topo.num_servers) // 16 * 16  # a worker's landing region per server
        self.row_used = [0] * topo.num_servers
        self.land_used = [0] * topo.num_servers
        self.slots = [0] * topo.num_servers
        self.keys: Dict[int, tuple] = {}  # kid -> (server, nbytes, row_off, land_off, flag slot)

    def add_key(self, kid: int, nbytes: int) -> bool:
        s = self.topo.server_of(kid)
        rows = self.topo.num_workers * _pad16(nbytes)
        if (self.row_used[s] + rows > self.bytes or self.land_used[s] + _pad16(nbytes) > self.region
                or self.slots[s] >= _MAX_SLOTS // max(1, self.topo.num_servers)
                or self.topo.num_workers > _MAX_KV_WORKERS):
            return False  # stays on the gloo payload path (decided identically on every member)
        self.keys[kid] = (s, nbytes, self.row_used[s], s * self.region + self.land_used[s], self.slots[s])
        self.row_used[s] += rows
        self.land_used[s] += _pad16(nbytes)
        self.slots[s] += 1
        return True


class _KvPlane:
    """The GPU payload windows of one server / worker (module docstring), laid out by _KvLayout."""

    def __init__(self, topo: "_Topology", device: torch.device):
        import ctypes

        from ..ops import _lib

        self.topo, self.device, self.L = topo, device, _lib.lib()
        self.bytes = int(os.environ.get("TONY_KV_WINDOW_MB", "64")) << 20
        hsize = self.L.tony_xgmi_handle_bytes()
        win, handle = ctypes.c_void_p(), (ctypes.c_uint8 * hsize)()
        with torch.cuda.device(device):
            rc = self.L.tony_ps_window_alloc(self.bytes, ctypes.byref(win), handle)
        self.window = win.value if rc == 0 else None
        self._opened: List[int] = []
        hdr = self.L.tony_ps_header_bytes()
        allh: List[Optional[bytes]] = [None] * topo.world
        dist.all_gather_object(allh, bytes(handle) if rc == 0 else b"")  # every member joins, even on failure
        _lib.check(rc, "tony_ps_window_alloc")
        if not all(allh):
            raise RuntimeError("a peer could not allocate its window")
        self.base = self.window + hdr
        self.peer: Dict[int, int] = {}
        self.peer_win: Dict[int, int] = {}  # window bases (flag tables) of the peers
        peers = range(topo.num_servers, topo.world) if topo.role == "server" else range(topo.num_servers)
        for r in peers:
            p = ctypes.c_void_p()
            buf = (ctypes.c_uint8 * hsize).from_buffer_copy(allh[r])
            with torch.cuda.device(device):
                _lib.check(self.L.tony_xgmi_open(buf, ctypes.byref(p)), f"tony_xgmi_open(rank {r})")
            self.peer[r] = p.value + hdr
            self.peer_win[r] = p.value
            self._opened.append(p.value)
        self.layout = _KvLayout(topo, self.bytes)
        self.keys = self.layout.keys
        self._side: Dict[int, "torch.cuda.Stream"] = {}  # server: per pushing worker, waits + row reads
        self._arrived: Dict[tuple, int] = {}  # server: (kid, worker) -> flag counts expected so far
        # the window's error word, copied to pinned host memory behind every POLL_EVERY-th copy: a timed-out
        # device wait surfaces within a few calls on both sides without a device synchronisation
        self._err_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._polls = 0

    POLL_EVERY = 8

    def poll(self) -> None:
        """Raise if an earlier asynchronous read of the error word saw a timed-out wait; queue a new read."""
        from ..ops import _lib

        if int(self._err_host[0]):
            self.check()
        _lib.check(self.L.tony_ps_error_async(self.window, self._err_host.data_ptr(), _lib.stream_ptr(self.device)),
                   "tony_ps_error_async")

    def add_key(self, kid: int, nbytes: int) -> bool:
        return self.layout.add_key(kid, nbytes)

    def copy(self, dst: int, src: int, nbytes: int) -> None:
        """Stream-ordered local copy out of this rank's window behind a wait: skipped on the device when a
        wait of this window timed out (no stale or partial payload is merged or pulled), and the error is
        raised by the next check."""
        from ..ops import _lib

        with torch.cuda.device(self.device):
            _lib.check(self.L.tony_kv_copy(dst, src, nbytes, self.window, _lib.stream_ptr(self.device)),
                       "tony_kv_copy")
            self._polls += 1
            if self._polls % self.POLL_EVERY == 0:  # a cheap asynchronous read of the error word
                self.poll()

    def send(self, dst: int, src: int, nbytes: int, flag: int) -> int:
        """Copy into a peer's window and count it on the peer's flag at window offset ``flag`` (no host
        wait); returns the count the copy adds (the consumer's target grows by it)."""
        from ..ops import _lib

        with torch.cuda.device(self.device):
            _lib.check(self.L.tony_kv_copy_flag(dst, src, nbytes, flag, _lib.stream_ptr(self.device)),
                       "tony_kv_copy_flag")
        return self.L.tony_kv_copy_blocks(nbytes)

    def take(self, kid: int, w: int, numel: int, dtype: torch.dtype, thr: Optional[float] = None):
        """Server: worker w's pushed row of kid as a new tensor, and the event after its read.  The row has
        landed once the worker's copy counted all its workgroups on the key's push flag (``thr``: a 2-bit
        push -- the row holds ceil(numel / 16) words, counted by the workgroups of the worker's quantise
        kernel, and the read decodes them).  The wait and
        the read run on the worker's own stream: the bytes may depend on a reply this server has yet to
        store (the worker pushes behind its wait for its last pull), so nothing else may queue behind
        the wait.  The worker rewrites the row only behind its wait for a later reply, which the server
        stores after merging this round -- no host wait on either side."""
        _, nbytes, row_off, _, slot = self.keys[kid]
        side = self._side.get(w)
        if side is None:
            side = self._side[w] = torch.cuda.Stream(self.device)
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(side):
            buf = torch.empty(numel, dtype=dtype, device=self.device)
            blocks = self.L.tony_kv_copy_blocks(nbytes) if thr is None else self.L.tony_kv_quant_blocks(numel)
            n = self._arrived[(kid, w)] = self._arrived.get((kid, w), 0) + blocks
            self.wait(_push_flag(slot, w), n)
            if thr is None:
                self.copy(buf.data_ptr(), self.base + row_off + w * _pad16(nbytes), nbytes)
            else:
                self.decode(buf.data_ptr(), self.base + row_off + w * _pad16(nbytes), numel, thr)
            ev = torch.cuda.Event()
            ev.record(side)
        buf.record_stream(main)
        return buf, ev

    def take_rsp(self, kid: int, w: int, nnz: int, dtype: torch.dtype, row_elems: int):
        """Server: worker w's row-sparse push of kid -- ``nnz`` rows, then their int64 ids, in the worker's row of
        the window (two flagged copies on the key's push flag) -- as new tensors, and the event after their read;
        waited for and read on the worker's side stream like ``take``."""
        _, nbytes, row_off, _, slot = self.keys[kid]
        side = self._side.get(w)
        if side is None:
            side = self._side[w] = torch.cuda.Stream(self.device)
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(side):
            rows = torch.empty(nnz * row_elems, dtype=dtype, device=self.device)
            ids = torch.empty(nnz, dtype=torch.int64, device=self.device)
            rb = rows.numel() * rows.element_size()
            blocks = self.L.tony_kv_copy_blocks(rb) + self.L.tony_kv_copy_blocks(8 * nnz)
            n = self._arrived[(kid, w)] = self._arrived.get((kid, w), 0) + blocks
            self.wait(_push_flag(slot, w), n)
            src = self.base + row_off + w * _pad16(nbytes)
            self.copy(rows.data_ptr(), src, rb)
            self.copy(ids.data_ptr(), src + rb, 8 * nnz)
            ev = torch.cuda.Event()
            ev.record(side)
        rows.record_stream(main)
        ids.record_stream(main)
        return ids, rows, ev

    def decode(self, dst: int, src: int, numel: int, thr: float) -> None:
        """``copy`` for a row of 2-bit words: ``numel`` fp32 values decoded out of this rank's window, skipped on
        the device like the copy when a wait of this window timed out."""
        from ..ops import _lib

        with torch.cuda.device(self.device):
            _lib.check(self.L.tony_kv_dequant2(dst, src, numel, thr, 1, _gc_words(numel), self.window,
                                               _lib.stream_ptr(self.device)), "tony_kv_dequant2")
            self._polls += 1
            if self._polls % self.POLL_EVERY == 0:
                self.poll()

    def wait(self, flag_off: int, target: int) -> None:
        """Hold this rank's stream until the counter at ``flag_off`` of its window reaches ``target``."""
        from ..ops import _lib

        with torch.cuda.device(self.device):
            _lib.check(self.L.tony_kv_wait(self.window + flag_off, target & 0xFFFFFFFF, self.window,
                                           _wait_budget_s(), _lib.stream_ptr(self.device)), "tony_kv_wait")

    def check(self) -> None:
        """Raise if one of this rank's device waits timed out (synchronises the device)."""
        import ctypes

        from ..ops import _lib

        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            err = ctypes.c_int(0)
            _lib.check(self.L.tony_ps_error(self.window, ctypes.byref(err)), "tony_ps_error")
        if err.value:
            raise RuntimeError(f"kvstore plane: a device wait timed out after {_wait_budget_s()} s "
                               "(TONY_KV_WAIT_S): a peer never delivered its payload")

    def close(self) -> None:
        """Unmap the peers and free the window; raises afterwards if a device wait of this rank timed out
        (the copies behind it were skipped, so the run's payloads are not trustworthy)."""
        err = None
        if getattr(self, "window", None) is not None:
            torch.cuda.synchronize(self.device)  # no copy into or out of a window is left in flight
            try:
                self.check()
            except RuntimeError as e:
                err = e
        for p in self._opened:
            self.L.tony_xgmi_close(p)
        self._opened = []
        if getattr(self, "window", None) is not None:
            self.L.tony_xgmi_free(self.window)
            self.window = None
        if err is not None:
            raise err


def _make_plane(topo: "_Topology", device: Optional[torch.device]) -> Optional[_KvPlane]:
    """Collective over servers + workers: the plane when every member wants it (else None everywhere)."""
    want = device is not None and _plane_wanted()
    allw: List[Optional[bool]] = [None] * topo.world
    dist.all_gather_object(allw, want)
    if not all(allw):
        return None
    plane, err = None, ""
    try:
        plane = _KvPlane(topo, device)
    except Exception as e:  # noqa: BLE001 - e.g. a peer GPU this task cannot see: agree on gloo everywhere
        err = f"{type(e).__name__}: {e}"
    errs: List[Optional[str]] = [None] * topo.world
    dist.all_gather_object(errs, err)
    if any(errs):
        if plane is not None:
            plane.close()
        import sys

        print(f"[tony kvstore] GPU payload plane unavailable, payloads over gloo: "
              f"{'; '.join(f'rank {r}: {e}' for r, e in enumerate(errs) if e)}", file=sys.stderr, flush=True)
        return None
    return plane


def run_scheduler(poll_s: float = 0.05) -> int:
    """The scheduler role: host the rendezvous store until every server and worker exited."""
    topo = _Topology()
    store = dist.TCPStore("0.0.0.0", topo.root_port, topo.world + 1, True,
                          timeout=datetime.timedelta(seconds=1800), wait_for_workers=False)
    while store.add(_EXIT_KEY, 0) < topo.world:
        time.sleep(poll_s)
    return 0


class _Server:
    def __init__(self, topo: _Topology, sync: bool, plane: Optional[_KvPlane] = None):
        self.topo = topo
        self.sync = sync
        self.plane = plane
        self.values: Dict[int, torch.Tensor] = {}
        self.pushed: Dict[int, set] = {}
        self.deferred: Dict[int, List[int]] = {}
        self.opt: Optional[Optimizer] = None
        self.early: Dict[int, list] = {}
        self.gc: Optional[float] = None  # 2-bit gradient compression threshold (OP_GC)
        self.early_gc: list = []  # compressed pushes that arrived before the setting
        self.sends = []
        self.applied = 0
        self.round: Dict[int, list] = {}  # kid -> [(worker, arrival, payload, event)] of the open round
        self.rsp: Dict[int, tuple] = {}  # sparse keys -> (rows R, elements of a row)

    def _reply_rows(self, kid: int, worker: int, via_plane: bool, ids: torch.Tensor) -> None:
        """The answer to a row_sparse_pull: rows ``ids`` of the value, gathered straight into the worker's landing
        area and counted on its reply flag, or over gloo."""
        rows, re = self.rsp[kid]
        table = self.values[kid].view(rows, re)
        if via_plane:
            from ..ops import _lib

            srv, _, _, land_off, slot = self.plane.keys[kid]
            ids = ids.to(self.plane.device)
            with torch.cuda.device(self.plane.device):
                _lib.check(self.plane.L.tony_kv_rsp_gather(
                    self.plane.peer[worker] + land_off, table.data_ptr(), ids.data_ptr(), ids.numel(),
                    re * table.element_size(), rows, self.plane.peer_win[worker] + _reply_flag(self.topo, srv, slot),
                    None, _lib.stream_ptr(self.plane.device)), "tony_kv_rsp_gather")
            return
        self.sends.append(dist.isend(table.index_select(0, ids.to(table.device)).cpu().contiguous(), worker,
                                     tag=TAG_REPLY))

    def _reply(self, kid: int, worker: int, via_plane: bool = False, ids: Optional[torch.Tensor] = None) -> None:
        if ids is not None:
            self._reply_rows(kid, worker, via_plane, ids)
            return
        if via_plane:  # the value into the worker's landing area, counted on the worker's reply flag
            srv, nbytes, _, land_off, slot = self.plane.keys[kid]
            v = self.values[kid].contiguous()
            self.plane.send(self.plane.peer[worker] + land_off, v.data_ptr(), nbytes,
                            self.plane.peer_win[worker] + _reply_flag(self.topo, srv, slot))
            return
        self.sends.append(dist.isend(self.values[kid].contiguous().cpu(), worker, tag=TAG_REPLY))

    def _merge_round(self, kid: int) -> torch.Tensor:
        """The open round's pushes of kid summed in worker order (deterministic), on this stream after
        every plane push's row read (device events: the host never waits for a payload)."""
        v = self.values[kid]
        merged = None
        if kid in self.rsp:  # row-sparse pushes: the ordered merge of the module docstring
            vals = []
            for _, _, b, ev in sorted(self.round.pop(kid), key=lambda e: (e[0], e[1])):
                if ev is not None:
                    torch.cuda.current_stream(v.device).wait_event(ev)
                vals.append(b)
            return _rsp_merge(vals, v.device)
        for _, _, b, ev in sorted(self.round.pop(kid), key=lambda e: (e[0], e[1])):
            if ev is not None:
                torch.cuda.current_stream(v.device).wait_event(ev)
            b = b.to(v.device, v.dtype)  # every payload buffer is this server's own: summed in place
            merged = b if merged is None else merged.add_(b)
        return merged

    def _finish_round(self, kid: int) -> None:
        merged = self._merge_round(kid)
        if kid in self.rsp:
            _rsp_apply(self.opt, kid, self.values[kid].view(self.rsp[kid][0], -1), merged)
        elif self.opt is not None:
            self.opt.update(kid, self.values[kid], merged)
        else:
            self.values[kid].copy_(merged)
        self.applied += 1
        self.pushed[kid] = set()
        for w, via, ids in self.deferred.pop(kid, []):
            self._reply(kid, w, via, ids)

    def _rsp_request(self, worker: int, hdr: List[int], buf):
        """A row-sparse request: its payload received, a pull answered (or deferred).  Returns None when it is
        dealt with or parked, else ``(op, payload, event)`` for ``handle`` to carry on with: an ``OP_INIT`` with the
        dense value or an ``OP_PUSH`` with the pushed ``RowSparse``."""
        op, kid, numel, dcode = hdr
        dt = _DTYPES[dcode]
        if buf is None:
            if op == OP_INIT_RSP:
                dense, rows = torch.empty(numel, dtype=dt), torch.empty(1, dtype=torch.int64)
                dist.recv(dense, worker, tag=TAG_DATA)
                dist.recv(rows, worker, tag=TAG_DATA)
                buf = (dense, int(rows[0]))
            elif op == OP_PUSH_RSP and numel:
                meta = torch.empty(numel + 1, dtype=torch.int64)  # the ids, then the elements of a row
                dist.recv(meta, worker, tag=TAG_DATA)
                data = torch.empty(numel * int(meta[-1]), dtype=dt)
                dist.recv(data, worker, tag=TAG_DATA)
                buf = (meta[:-1].clone(), data)
            elif op in (OP_PULL_RSP, OP_PULL_RSPX):
                buf = torch.empty(numel, dtype=torch.int64)
                dist.recv(buf, worker, tag=TAG_DATA)
        if op == OP_INIT_RSP:
            dense, rows = buf
            self.rsp[kid] = (rows, dense.numel() // max(1, rows))
            return OP_INIT, dense, None
        if kid not in self.values:  # raced ahead of worker 0's INIT: replayed once the key exists (see handle)
            self.early.setdefault(kid, []).append((worker, hdr, buf))
            return None
        rows, re = self.rsp[kid]
        if op in (OP_PULL_RSP, OP_PULL_RSPX):
            via = op == OP_PULL_RSPX
            if self.sync and worker in self.pushed.get(kid, ()):
                self.deferred.setdefault(kid, []).append((worker, via, buf))
            else:
                self._reply(kid, worker, via, buf)
            return None
        ev = None
        if op == OP_PUSH_RSPX and numel:
            ids, data, ev = self.plane.take_rsp(kid, worker - self.topo.num_servers, numel, dt, re)
        elif numel:
            ids, data = buf
        else:
            ids, data = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=dt)
        return OP_PUSH, RowSparse(ids, data.view(numel, re), (rows, re), _checked=True), ev

    def handle(self, worker: int, hdr: List[int], buf: Optional[torch.Tensor] = None) -> bool:
        op, kid, numel, dcode = hdr
        ev_rsp = None
        if op >= OP_INIT_RSP:
            got = self._rsp_request(worker, hdr, buf)
            if got is None:
                return True
            op, buf, ev_rsp = got
        if op in (OP_INIT, OP_PUSH, OP_OPT, OP_GC) and buf is None:
            buf = torch.empty(numel, dtype=_DTYPES[dcode])
            dist.recv(buf, worker, tag=TAG_DATA)
        if op == OP_GC:  # the workers' set_gradient_compression, shipped by rank 0 (kid: this server)
            self.gc = _gc_threshold(json.loads(bytes(buf.tolist()).decode()))
            parked, self.early_gc = self.early_gc, []
            for w, h, b in parked:
                self.handle(w, h, b)
            return True
        if op == OP_PUSH_C and buf is None:
            buf = torch.empty(_gc_words(numel), dtype=torch.int32)
            dist.recv(buf, worker, tag=TAG_DATA)
        if op in (OP_PUSH_C, OP_PUSH_CX) and self.gc is None:
            # raced ahead of rank 0's setting (sent before the workers' barrier, like an INIT): replay once it is here
            self.early_gc.append((worker, hdr, buf))
            return True
        via = op == OP_PULL_X
        if op in (OP_PUSH, OP_PULL, OP_PUSH_X, OP_PULL_X, OP_PUSH_C, OP_PUSH_CX) and kid not in self.values:
            # raced ahead of worker 0's INIT (it is sent before the workers' barrier, but the server
            # may poll this worker first): replay once the key exists.  A plane push is parked with its
            # raw header: the key has no window row in this server's layout until the INIT adds it, and
            # the worker does not rewrite that row before its next pull (DistKVStore._unread)
            self.early.setdefault(kid, []).append((worker, hdr, buf))
            return True
        ev = ev_rsp
        if op == OP_PUSH_X:  # the payload is in this worker's receive row of the window: take it now
            buf, ev = self.plane.take(kid, worker - self.topo.num_servers, numel, _DTYPES[dcode])
            op = OP_PUSH
        elif op == OP_PUSH_CX:  # 2-bit words in the row: the read decodes them
            buf, ev = self.plane.take(kid, worker - self.topo.num_servers, numel, torch.float32, self.gc)
            op = OP_PUSH
        elif op == OP_PUSH_C:  # 2-bit words over gloo: decoded on the value's device
            v = self.values[kid]
            if v.is_cuda:
                buf = _dequant2_gpu(buf.to(v.device), numel, self.gc)
            else:
                buf = _dequant2_torch(buf, numel, self.gc)
            op = OP_PUSH
        elif op == OP_PULL_X:
            op = OP_PULL
        if op in (OP_INIT, OP_PUSH, OP_OPT):
            if op == OP_INIT:
                if self.plane is not None and self.plane.add_key(kid, buf.numel() * buf.element_size()):
                    buf = buf.to(self.plane.device)  # the key's value lives on the server's GPU

                self.values[kid] = buf
                self.pushed[kid] = set()
                for w, h, b in self.early.pop(kid, []):
                    self.handle(w, h, b)
            elif op == OP_OPT:
                self.opt = Optimizer.from_json(bytes(buf.tolist()).decode())
            else:
                r = self.round.setdefault(kid, [])
                r.append((worker, len(r), buf, ev))
                if not self.sync:
                    self._finish_round(kid)
                    return True
                self.pushed[kid].add(worker)
                if len(self.pushed[kid]) == self.topo.num_workers:
                    self._finish_round(kid)
        elif op == OP_PULL:
            if self.sync and worker in self.pushed.get(kid, ()):
                self.deferred.setdefault(kid, []).append((worker, via, None))
            else:
                self._reply(kid, worker, via)
        elif op == OP_STOP:
            return False
        return True

    def serve(self) -> None:
        """Receive request headers from ANY worker (gloo recv-anysource) until all sent STOP."""
        live = self.topo.num_workers
        hdr = torch.empty(4, dtype=torch.int64)
        while live:
            w = dist.recv(hdr, tag=TAG_HDR)
            if not self.handle(w, [int(x) for x in hdr.tolist()]):
                live -= 1
                if self.plane is not None:  # a worker finished: nothing it sent may have timed out
                    self.plane.check()
            if len(self.sends) > 64:
                for s in self.sends:
                    s.wait()
                self.sends = []
        for s in self.sends:
            s.wait()


def run_server(sync: Optional[bool] = None) -> int:
    """The server role: own keys until every worker sent STOP."""
    topo = _Topology()
    store, _ = _init_group(topo)
    dev = None
    if torch.cuda.is_available():  # a server may share a worker's GPU (TonY's servers ask for none)
        dev = torch.device("cuda", _env_int("TONY_KV_DEVICE", topo.index % torch.cuda.device_count()))
    plane = _make_plane(topo, dev)
    if sync is None:  # every worker announces its kvstore type before its first request
        sync = store.get("tony/kv/type").decode() != "dist_async"
    _Server(topo, sync, plane).serve()
    dist.barrier()
    if plane is not None:
        plane.close()
    store.add(_EXIT_KEY, 1)
    return 0


class DistKVStore(KVStore):
    """Worker side of ``dist_sync`` / ``dist_async``."""

    def __init__(self, kind: str):
        super().__init__(kind)
        self.topo = _Topology()
        if self.topo.num_servers < 1:
            raise ValueError(f"{kind} needs DMLC_NUM_SERVER >= 1 server task")
        self.store, self.workers = _init_group(self.topo)
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        self.plane = _make_plane(self.topo, dev)
        self.store.set("tony/kv/type", kind)
        self._shapes: Dict[int, torch.Size] = {}
        self._unread: set = set()  # keys pushed on the plane and not pulled since (their row may be unread)
        self._replies: Dict[int, int] = {}  # kid -> reply copies counted on this worker's flag (target)
        # kid -> event after the last plane pull's copy out of the landing area: a repeat pull with no push
        # in between must not let the server overwrite that area before the copy read it
        self._landed: Dict[int, "torch.cuda.Event"] = {}
        self.plane_ops = [0, 0]  # pushes / pulls whose payload went over the GPU plane (tests)
        self._gc: Optional[float] = None  # 2-bit gradient compression threshold (set_gradient_compression)
        self._res = _Residuals()
        self._pushed = False
        self.compressed_ops = [0, 0]  # 2-bit pushes whose words went over the GPU plane / over gloo (tests)
        # row-sparse pushes on the plane / over gloo, row_sparse_pulls on the plane / over gloo (tests); a push or
        # pull of no rows moves no payload and is counted nowhere
        self.sparse_ops = [0, 0, 0, 0]
        self._rsp_dtype: Dict[int, torch.dtype] = {}  # sparse keys -> the dtype of their value
        self._closed = False

    @property
    def rank(self) -> int:
        return self.topo.index

    @property
    def num_workers(self) -> int:
        return self.topo.num_workers

    def _send(self, op: int, kid: int, payload: Optional[torch.Tensor] = None) -> int:
        srv = self.topo.server_of(kid) if op != OP_STOP else kid
        n, dc = (payload.numel(), _dcode(payload.dtype)) if payload is not None else (0, 0)
        dist.send(torch.tensor([op, kid, n, dc], dtype=torch.int64), srv, tag=TAG_HDR)
        if payload is not None:
            dist.send(payload, srv, tag=TAG_DATA)
        return srv

    def init(self, key, value) -> None:
        for k, v in zip(*self._keys_vals(key, value)):
            kid = self._key(k)
            t = _as_list(v)[0]
            sparse = isinstance(t, RowSparse)
            if sparse:  # a sparse key: the servers hold its dense value and learn its row count
                self._sparse[kid], self._rsp_dtype[kid] = t.shape, t.data.dtype
                t = t.to_dense()
            t = t.detach()
            self._shapes[kid] = t.shape
            if self.plane is not None:
                self.plane.add_key(kid, t.numel() * t.element_size())
            if self.rank == 0:
                srv = self._send(OP_INIT_RSP if sparse else OP_INIT, kid, t.reshape(-1).cpu().contiguous())
                if sparse:
                    dist.send(torch.tensor([t.shape[0]], dtype=torch.int64), srv, tag=TAG_DATA)
        self.barrier()

    def _on_plane(self, kid: int, t: torch.Tensor) -> bool:
        return self.plane is not None and kid in self.plane.keys and t.is_cuda

    def push(self, key, value, priority: int = 0) -> None:  # noqa: ARG002
        for k, v in zip(*self._keys_vals(key, value)):
            kid = self._key(k)
            if self._sparse_push(kid, _as_list(v)):  # (never compressed, as in MXNet)
                self._pushed = True
                self._push_rsp(kid, _rsp_merge(_as_list(v)))
                continue
            g = _merge(_as_list(v)).reshape(-1)
            self._pushed = True
            if self._gc is not None and g.dtype == torch.float32:
                self._push_2bit(kid, g)
                continue
            if self._on_plane(kid, g) and kid not in self._unread:
                srv, nbytes, row_off, _, slot = self.plane.keys[kid]
                g = g.to(self.plane.device).contiguous()
                if g.data_ptr() % 16:  # the copy kernel moves 16-B aligned addresses: a view at an odd offset
                    g = g.clone()
                # into this worker's row of the server's window, counted on the key's push flag there; the
                # header may overtake the bytes: the server's stream waits for the flag before reading
                self.plane.send(self.plane.peer[srv] + row_off + self.rank * _pad16(nbytes), g.data_ptr(), nbytes,
                                self.plane.peer_win[srv] + _push_flag(slot, self.rank))
                dist.send(torch.tensor([OP_PUSH_X, kid, g.numel(), _dcode(g.dtype)], dtype=torch.int64), srv,
                          tag=TAG_HDR)
                self._unread.add(kid)
                self.plane_ops[0] += 1
                continue
            self._send(OP_PUSH, kid, g.cpu().contiguous())

    def _push_rsp(self, kid: int, m: RowSparse) -> None:
        """A push of the merged row-sparse value ``m`` (module docstring)."""
        srv = self.topo.server_of(kid)
        nnz, re = m.nnz, _row_elems(m.shape)
        row_bytes = re * m.data.element_size()
        hdr = [kid, nnz, _dcode(m.data.dtype)]
        if nnz == 0:  # the header only: the server counts this worker's (empty) part of the round
            dist.send(torch.tensor([OP_PUSH_RSP] + hdr, dtype=torch.int64), srv, tag=TAG_HDR)
            return
        if (self._on_plane(kid, m.data) and kid not in self._unread and row_bytes % 16 == 0
                and nnz * row_bytes + _pad16(8 * nnz) <= _pad16(self.plane.keys[kid][1])):
            _, nbytes, row_off, _, slot = self.plane.keys[kid]
            rows = _aligned16(m.data.to(self.plane.device))
            ids = _aligned16(m.indices.to(self.plane.device))
            # the rows, then the ids behind them, into this worker's row of the server's window: two copies
            # counted on the key's push flag there (the server computes both counts from nnz)
            base = self.plane.peer[srv] + row_off + self.rank * _pad16(nbytes)
            flag = self.plane.peer_win[srv] + _push_flag(slot, self.rank)
            self.plane.send(base, rows.data_ptr(), nnz * row_bytes, flag)
            self.plane.send(base + nnz * row_bytes, ids.data_ptr(), 8 * nnz, flag)
            dist.send(torch.tensor([OP_PUSH_RSPX] + hdr, dtype=torch.int64), srv, tag=TAG_HDR)
            self._unread.add(kid)
            self.plane_ops[0] += 1
            self.sparse_ops[0] += 1
            return
        # off the plane, too many rows for the window row, a re-push before a pull or a CPU value: over gloo
        dist.send(torch.tensor([OP_PUSH_RSP] + hdr, dtype=torch.int64), srv, tag=TAG_HDR)
        dist.send(torch.cat([m.indices.cpu(), torch.tensor([re], dtype=torch.int64)]), srv, tag=TAG_DATA)
        dist.send(m.data.reshape(-1).cpu().contiguous(), srv, tag=TAG_DATA)
        self.sparse_ops[1] += 1

    def _rsp_shape(self, kid: int, dst: RowSparse) -> tuple:  # noqa: ARG002
        if kid not in self._sparse:
            raise TypeError(f"row_sparse_pull: key {kid} is not a row-sparse key of this store")
        return self._sparse[kid]

    def _pull_rows(self, kid: int, ids: torch.Tensor, shape: tuple, dtype, device) -> torch.Tensor:  # noqa: ARG002
        """Rows ``ids`` (sorted, unique, in range) of a sparse key from its server.  The ids go over gloo with the
        header (8 B per row against the row's bytes; the host needs their count anyway: one synchronisation per
        call); on the plane the server gathers the rows into this worker's landing area."""
        nnz, re, kdt = ids.numel(), _row_elems(shape), self._rsp_dtype[kid]
        if nnz == 0:
            return torch.empty((0,) + shape[1:], dtype=kdt, device=device)
        row_bytes = re * torch.empty((), dtype=kdt).element_size()
        hdr = torch.tensor([0, kid, nnz, _dcode(kdt)], dtype=torch.int64)
        cpu_ids = ids.cpu().contiguous()
        if (self.plane is not None and kid in self.plane.keys and device.type == "cuda" and kdt == torch.float32
                and row_bytes % 16 == 0):
            hdr[0] = OP_PULL_RSPX
            blocks = self.plane.L.tony_kv_rsp_gather_blocks(nnz, row_bytes)
            buf = self._plane_fetch(kid, hdr, cpu_ids, blocks, nnz * row_bytes, nnz * re, kdt)
            self.sparse_ops[2] += 1
        else:
            hdr[0] = OP_PULL_RSP
            srv = self.topo.server_of(kid)
            dist.send(hdr, srv, tag=TAG_HDR)
            dist.send(cpu_ids, srv, tag=TAG_DATA)
            buf = torch.empty(nnz * re, dtype=kdt)
            dist.recv(buf, srv, tag=TAG_REPLY)
            self._unread.discard(kid)
            self.sparse_ops[3] += 1
        return buf.view((nnz,) + shape[1:])

    def _plane_fetch(self, kid: int, hdr: torch.Tensor, ids: Optional[torch.Tensor], blocks: int, nbytes: int,
                     numel: int, dtype: torch.dtype) -> torch.Tensor:
        """Ask the key's server (``hdr``, then ``ids`` if any) for a reply into this worker's landing area and
        copy its ``nbytes`` out behind a device wait for the ``blocks`` counts the reply adds to the reply flag."""
        srv, _, _, land_off, slot = self.plane.keys[kid]
        prev = self._landed.pop(kid, None)
        if prev is not None and kid not in self._unread:
            # no push since the last pull: nothing orders the server's next reply store after that
            # pull's copy-out (a push would -- the server answers only after reading it, and the push
            # copy queues behind the copy-out); wait for the copy-out before asking again
            prev.synchronize()
        dist.send(hdr, srv, tag=TAG_HDR)
        if ids is not None:
            dist.send(ids, srv, tag=TAG_DATA)
        # the reply lands in this worker's landing area, counted on its reply flag: this stream waits
        # for it on the device, then copies it out -- the host moves on at once
        n = self._replies[kid] = self._replies.get(kid, 0) + blocks
        self.plane.wait(_reply_flag(self.topo, srv, slot), n)
        buf = torch.empty(numel, dtype=dtype, device=self.plane.device)
        self.plane.copy(buf.data_ptr(), self.plane.base + land_off, nbytes)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.plane.device))
        self._landed[kid] = ev
        self._unread.discard(kid)  # the server answered: it consumed this worker's earlier rows
        self.plane_ops[1] += 1
        return buf

    def _push_2bit(self, kid: int, g: torch.Tensor) -> None:
        """A push of the merged flat fp32 gradient with 2-bit compression on (module docstring)."""
        srv = self.topo.server_of(kid)
        hdr = [kid, g.numel(), _dcode(g.dtype)]
        if self._on_plane(kid, g) and kid not in self._unread:
            _, nbytes, row_off, _, slot = self.plane.keys[kid]
            g = _aligned16(g.to(self.plane.device))
            # one kernel: the residual updated in place, the words straight into this worker's row of the
            # server's window (they fit it: 4 B per 16 elements), counted on the key's push flag there
            _quant2_gpu(g, self._res.of(kid, g), self._gc, self.plane.peer[srv] + row_off + self.rank * _pad16(nbytes),
                        self.plane.peer_win[srv] + _push_flag(slot, self.rank))
            dist.send(torch.tensor([OP_PUSH_CX] + hdr, dtype=torch.int64), srv, tag=TAG_HDR)
            self._unread.add(kid)
            self.plane_ops[0] += 1
            self.compressed_ops[0] += 1
            return
        # off the plane, a re-push before a pull (the row may be unread) or a CPU tensor: the words over gloo
        words = self._res.quantise(kid, g, self._gc).cpu()
        dist.send(torch.tensor([OP_PUSH_C] + hdr, dtype=torch.int64), srv, tag=TAG_HDR)
        dist.send(words, srv, tag=TAG_DATA)
        self.compressed_ops[1] += 1

    def set_gradient_compression(self, params: dict) -> None:
        """Collective over the workers, like ``set_optimizer``: rank 0 ships the setting to every server.  Allowed
        until the first push (a residual and the servers' decoding must cover every push of a key alike)."""
        thr = _gc_threshold(params)
        if self._pushed:
            raise RuntimeError("set_gradient_compression must be called before the first push")
        if self.rank == 0:
            cfg = json.dumps({"type": "none" if thr is None else "2bit", "threshold": thr if thr else 0.5})
            payload = torch.tensor(list(cfg.encode()), dtype=torch.uint8)
            for s in range(self.topo.num_servers):
                self._send_to(s, OP_GC, payload)
        self._gc = thr
        self.barrier()

    def pull(self, key, out=None, priority: int = 0, ignore_sparse: bool = True):  # noqa: ARG002
        keys, outs = self._keys_vals(key, out)
        for k, o in zip(keys, outs):
            kid = self._key(k)
            if ignore_sparse and kid in self._sparse:
                continue
            first = _as_list(o)[0]
            if self._on_plane(kid, first):
                nbytes = self.plane.keys[kid][1]
                buf = self._plane_fetch(kid, torch.tensor([OP_PULL_X, kid, 0, 0], dtype=torch.int64), None,
                                        self.plane.L.tony_kv_copy_blocks(nbytes), nbytes, first.numel(), first.dtype)
            else:
                srv = self._send(OP_PULL, kid)
                buf = torch.empty(first.numel(), dtype=first.dtype)
                dist.recv(buf, srv, tag=TAG_REPLY)
                self._unread.discard(kid)
            for t in _as_list(o):
                t.copy_(buf.view(t.shape).to(t.device))

    def set_optimizer(self, optimizer: Optimizer) -> None:
        """Ship the optimizer to every server (MXNet pickles it; here it is a JSON config)."""
        if self.rank == 0:
            payload = torch.tensor(list(optimizer.to_json().encode()), dtype=torch.uint8)
            for s in range(self.topo.num_servers):
                self._send_to(s, OP_OPT, payload)
        self.barrier()

    def _send_to(self, srv: int, op: int, payload: torch.Tensor) -> None:
        dist.send(torch.tensor([op, srv, payload.numel(), _dcode(payload.dtype)], dtype=torch.int64), srv,
                  tag=TAG_HDR)
        dist.send(payload, srv, tag=TAG_DATA)

    def barrier(self) -> None:
        if self.plane is not None:
            self.plane.check()
        dist.barrier(group=self.workers)

    def save_optimizer_states(self, fname: str, dump_optimizer: bool = False) -> None:
        raise NotImplementedError("optimizer states live on the servers in dist modes")

    def close(self) -> None:
        """Tell every server this worker is done (MXNet does this at process exit)."""
        if self._closed:
            return
        self._closed = True
        self.barrier()
        for s in range(self.topo.num_servers):
            dist.send(torch.tensor([OP_STOP, s, 0, 0], dtype=torch.int64), s, tag=TAG_HDR)
        dist.barrier()
        if self.plane is not None:
            self.plane.close()
        self.store.add(_EXIT_KEY, 1)


class DeviceSyncKVStore(KVStore):
    """``dist_device_sync``: RCCL all-reduce of pushes among workers + replicated updater."""

    def __init__(self, kind: str = "dist_device_sync", group=None):
        super().__init__(kind)
        if not dist.is_initialized():
            from .bootstrap import init_from_env

            init_from_env()
        self.group = group
        self._gc: Optional[float] = None  # 2-bit gradient compression threshold (set_gradient_compression)
        self._res = _Residuals()
        self._pushed = False

    @property
    def rank(self) -> int:
        return dist.get_rank(self.group)

    @property
    def num_workers(self) -> int:
        return dist.get_world_size(self.group)

    def init(self, key, value) -> None:
        for k, v in zip(*self._keys_vals(key, value)):
            t = self._init_value(self._key(k), v)
            dist.broadcast(t, 0, group=self.group)
            self._store[self._key(k)] = t

    def push(self, key, value, priority: int = 0) -> None:  # noqa: ARG002
        for k, v in zip(*self._keys_vals(key, value)):
            if self._sparse_push(self._key(k), _as_list(v)):  # (never compressed, as in MXNet)
                self._pushed = True
                self._apply_rsp(self._key(k), self._allgather_rsp(_rsp_merge(_as_list(v))))
                continue
            g = _merge(_as_list(v))
            self._pushed = True
            if self._gc is not None and g.dtype == torch.float32:
                self._apply(self._key(k), self._allgather_2bit(self._key(k), g.reshape(-1)).view(g.shape))
                continue
            dist.all_reduce(g, group=self.group)
            self._apply(self._key(k), g)

    def _allgather_rsp(self, m: RowSparse) -> RowSparse:
        """The workers' row-sparse pushes merged in rank order, identically on every worker: the row counts
        all-gathered (one host synchronisation), then the ids and rows padded to the largest."""
        nw, dev, nnz = self.num_workers, m.data.device, m.nnz
        counts = torch.zeros(nw, 1, dtype=torch.int64, device=dev)
        dist.all_gather(list(counts.unbind(0)), torch.tensor([nnz], dtype=torch.int64, device=dev), group=self.group)
        counts = counts.reshape(-1).tolist()
        most, re = max(counts), _row_elems(m.shape)
        if most == 0:
            return m
        ids = torch.zeros(most, dtype=torch.int64, device=dev)
        rows = torch.zeros(most * re, dtype=m.data.dtype, device=dev)
        ids[:nnz].copy_(m.indices)
        rows[:nnz * re].copy_(m.data.reshape(-1))
        all_ids = torch.empty(nw, most, dtype=torch.int64, device=dev)
        all_rows = torch.empty(nw, most * re, dtype=m.data.dtype, device=dev)
        dist.all_gather(list(all_ids.unbind(0)), ids, group=self.group)
        dist.all_gather(list(all_rows.unbind(0)), rows, group=self.group)
        return _rsp_merge([RowSparse(all_ids[r, :n], all_rows[r, :n * re].view((n,) + m.shape[1:]), m.shape,
                                     _checked=True) for r, n in enumerate(counts)])

    def _allgather_2bit(self, kid: int, g: torch.Tensor) -> torch.Tensor:
        """The workers' 2-bit pushes of flat fp32 ``g``: the words all-gathered, the decoded values summed in
        rank order (``acc = v_0; acc += v_1; ...``), identically on every worker."""
        n, nw = g.numel(), self.num_workers
        words = self._res.quantise(kid, g, self._gc)
        gathered = torch.empty(nw, _gc_words(n), dtype=torch.int32, device=words.device)
        dist.all_gather(list(gathered.unbind(0)), words, group=self.group)
        if gathered.is_cuda:
            return _dequant2_gpu(gathered, n, self._gc, nsrc=nw)
        acc = _dequant2_torch(gathered[0], n, self._gc)
        for r in range(1, nw):
            acc += _dequant2_torch(gathered[r], n, self._gc)
        return acc

    def set_gradient_compression(self, params: dict) -> None:
        """Collective over the workers; allowed until the first push."""
        thr = _gc_threshold(params)
        if self._pushed:
            raise RuntimeError("set_gradient_compression must be called before the first push")
        self._gc = thr
        self.barrier()

    def barrier(self) -> None:
        dist.barrier(group=self.group)


def create(name: str = "local") -> KVStore:
    name = name.lower()
    if name in ("local", "device", "local_allreduce_cpu", "local_allreduce_device"):
        return KVStore(name)
    if name in ("dist_sync", "dist_async", "dist"):
        return DistKVStore("dist_sync" if name == "dist" else name)
    if name in ("dist_device_sync", "dist_sync_device"):
        return DeviceSyncKVStore("dist_device_sync")
    raise ValueError(f"unknown kvstore type {name!r}")


def run_role() -> bool:
    """Run the scheduler / server loop if this task is one; True when the caller should exit.

    ``import mxnet`` does this implicitly for non-worker roles (mxnet_dist_ex.py:10-13).
    """
    role = os.environ.get("DMLC_ROLE", "worker")
    if role == "scheduler":
        run_scheduler()
        return True
    if role == "server":
        run_server()
        return True
    return False


Value = Union[torch.Tensor, List[torch.Tensor]]
