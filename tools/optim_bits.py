#!/usr/bin/env python3
"""A bit pin of the flat optimizers: one sha256 per case over the bytes of everything a step writes.

    python tools/optim_bits.py [--out FILE]

Every case builds its master and gradients from integer arithmetic on ``torch.arange`` (no RNG: the same values
on any torch), runs 3 steps through the public ``Flat*`` API and hashes the master, every state tensor, the EMA
and the bf16 copy.  The updates are element-wise and the norms are stored in a fixed order (no atomics), so the
digests are exact: the same kernels give the same bits.  tests/golden/optim_bits.json holds the digests of the
commit before the kinds were folded onto one apply kernel; tests/test_optim_bits_gpu.py compares against it.

Cases: SGD (plain, Nesterov, and resync with elements of the bf16 copy overwritten between steps), Adam, AdamW,
Adagrad, RMSProp, RMSProp-TF, LARS and LAMB (three segments, one not adapted), each with a bf16 and an fp32
gradient, in three forms: defaults, ``clip_norm`` small enough to clip, ``ema_decay``.  The flat kinds update
1036 elements at offset 8 of a 1052-element shard (not a multiple of the workgroup, an offset range, untouched
elements on both sides).  SGD and RMSProp-TF also run, plain and clipped + EMA, at 8192 * 256 * 4 + 1024 elements,
the first size at which the 8192-workgroup grid takes a second grid-stride trip.
"""
import argparse
import functools
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

STEPS = 3
SMALL = (1052, 8, 1036)  # shard, lo, n
BIG = 8192 * 256 * 4 + 1024
FORMS = {"plain": {}, "clip": {"clip_norm": 0.5}, "ema": {"ema_decay": 0.9},
         "clip_ema": {"clip_norm": 0.5, "ema_decay": 0.9}}


def _ramp(n, mul, add, mod, scale):
    """((i * mul + add) mod ``mod``, centred) / scale: small integers over a power of two, exact in fp32."""
    i = torch.arange(n, dtype=torch.int64)
    return ((i * mul + add) % mod - mod // 2).to(torch.float32) / scale


@functools.lru_cache(maxsize=None)
def master(n):
    return _ramp(n, 7919, 13, 2003, 512.0)


@functools.lru_cache(maxsize=None)
def gradient(n, step, dtype):
    if dtype == torch.bfloat16:  # at most 7 significant bits: exact in bf16
        return _ramp(n, 104729, 31 * step + 7, 255, 256.0).to(torch.bfloat16)
    return _ramp(n, 104729, 31 * step + 7, 65521, 65536.0)


def _flat_kinds():
    from tony_amd.ops import FlatAdagrad, FlatAdam, FlatRMSProp, FlatSGD

    wd = dict(weight_decay=4e-5)
    return {
        "sgd": (lambda w, **kw: FlatSGD(w, 0.05, momentum=0.9, **wd, **kw), ["v"]),
        "sgd_nesterov": (lambda w, **kw: FlatSGD(w, 0.05, momentum=0.9, nesterov=True, **wd, **kw), ["v"]),
        "sgd_resync": (lambda w, **kw: FlatSGD(w, 0.05, momentum=0.9, resync=True, **wd, **kw), ["v"]),
        "adam": (lambda w, **kw: FlatAdam(w, 0.01, **wd, **kw), ["m", "v"]),
        "adamw": (lambda w, **kw: FlatAdam(w, 0.01, weight_decay=0.01, decoupled=True, **kw), ["m", "v"]),
        "adagrad": (lambda w, **kw: FlatAdagrad(w, 0.05, **wd, **kw), ["h"]),
        "rmsprop": (lambda w, **kw: FlatRMSProp(w, 0.01, momentum=0.9, **wd, **kw), ["ms", "mom"]),
        "rmsprop_tf": (lambda w, **kw: FlatRMSProp(w, 0.01, momentum=0.9, eps=1.0, tf_style=True, **wd, **kw),
                       ["ms", "mom"]),
    }


def _layer_kinds(n):
    from tony_amd.ops import FlatLAMB, FlatLARS, Segments

    def seg():
        return Segments([0, 400, 656, n], [0, 1, 2], [True, False, True])

    return {
        "lars": (lambda w, **kw: FlatLARS(w, 0.05, momentum=0.9, weight_decay=4e-5, trust_coef=0.02, segments=seg(),
                                          **kw), ["v"]),
        "lamb": (lambda w, **kw: FlatLAMB(w, 0.01, weight_decay=0.01, segments=seg(), **kw), ["m", "v"]),
    }


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(make, states, form, dtype, shard, lo, n, dev, whole=False, poke=False):
    opt = make(master(shard).to(dev), **FORMS[form])
    opt.grad_scale = 0.5
    out = opt.w[lo:lo + n].to(torch.bfloat16)
    for step in range(1, STEPS + 1):
        grad = gradient(n, step, dtype).to(dev)
        if poke and step > 1:  # the compute copy overwritten behind the optimizer: resync re-seeds those masters
            out[5::97] = 0.25 * step
        if whole:
            opt.step(grad, out_bf16=out)
            continue
        opt.begin_step()
        if opt.needs_norm:
            opt.accumulate_sumsq(grad, 0)
            opt.finish_norm(1)
        opt.apply_range(grad, lo, out_bf16=out)
    ema = [opt.ema] if opt.ema is not None else []
    return _digest([opt.w, *[getattr(opt, s) for s in states], *ema, out])


def digests(dev):
    res = {}
    dtypes = (("bf16", torch.bfloat16), ("fp32", torch.float32))
    shard, lo, n = SMALL
    for kind, (make, states) in _flat_kinds().items():
        for dname, dtype in dtypes:
            for form in ("plain", "clip", "ema"):
                res[f"{kind}/{dname}/{form}/n{n}"] = run_case(make, states, form, dtype, shard, lo, n, dev,
                                                              poke=kind == "sgd_resync")
    for kind, (make, states) in _layer_kinds(n).items():
        for dname, dtype in dtypes:
            for form in ("plain", "clip", "ema"):
                res[f"{kind}/{dname}/{form}/n{n}"] = run_case(make, states, form, dtype, n, 0, n, dev, whole=True)
    flat = _flat_kinds()
    for kind in ("sgd", "rmsprop_tf"):
        for dname, dtype in dtypes:
            for form in ("plain", "clip_ema"):
                res[f"{kind}/{dname}/{form}/n{BIG}"] = run_case(*flat[kind], form, dtype, BIG, 0, BIG, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the digests to this JSON file")
    a = ap.parse_args()
    res = digests(torch.device("cuda", 0))
    text = json.dumps(res, indent=0, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
