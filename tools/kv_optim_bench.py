#!/usr/bin/env python3
"""Device-event timing of the kvstore's fused optimizer kernels (csrc/kv_optim.hip: nag, adagrad, rmsprop plain and
centered, ftrl) beside the torch compositions of the same contract and beside plain copies of the same bytes, the
method of tools/kv_sparse_bench.py: 100 launches per window, the arms taking turns window by window so drift hits
all of them alike.

    python tools/kv_optim_bench.py [--launches 100] [--rounds 5] [--mb 64] [--sets 4] [--rows 4194304] [--nnz 65536]

Dense arms: a key of ``--mb`` MB of fp32.  Every kind walks ``--sets`` buffer sets (weight, states, gradient: 3 to 5
tensors of the key's size each, 0.75 to 1.25 GB in all by default, several times the 256 MB Infinity Cache) launch by
launch, so its bytes come from HBM; the kernel and the torch composition walk the same sets.  A ``tony_kv_copy`` of
the same number of bytes (half read, half written) rotates its source and destination through 1 GiB buffers.

Lazy arms: a table of ``--rows`` x 64 fp32 (1 GiB by default), ``--nnz`` random rows of it touched, the row sets
rotating launch by launch (32 sets of 16 MiB of rows, more than the cache holds).  Every kind runs beside the
gather / update / scatter of ``update_rows_generic`` and beside ``tony_kv_rsp_sgd`` with momentum.

The bytes an arm must move: per element 20 B for nag, adagrad and plain rmsprop (gradient read, weight and one state
read and written), 28 B for ftrl (two states), 36 B for centered rmsprop (three); a lazy launch adds its 8-byte ids.
Prints per arm the median / min / max ms per launch over the rounds and the rate those bytes imply, then the
kernels' times as ratios of the torch composition's, the copy's and lazy SGD's (scaled by the row streams moved).
Every process here is on one GPU: what the update costs a server that shares its GPU's HBM with a worker, or a key
reached over a link, is not visible and is not measured.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KINDS = [("nag", dict(momentum=0.9), 20), ("adagrad", {}, 20), ("rmsprop", {}, 20),
         ("rmsprop centered", dict(centered=True), 36), ("ftrl", {}, 28)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--nnz", type=int, default=65536)
    ap.add_argument("--id-sets", type=int, default=32)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.parallel import kvstore as K

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    n = a.mb * 1000 * 1000 // 4
    arms, copies = [], set()
    turn = {}

    def rotate(arm, count):
        turn[arm] = (turn.get(arm, -1) + 1) % count
        return turn[arm]

    def make(label, extra):
        name = label.split()[0]
        return K.Optimizer(name, learning_rate=0.01, wd=1e-4, rescale_grad=0.5, **extra)

    # -- dense: key k of an optimizer is buffer set k (the states live in the optimizer, one per key)
    for label, extra, per_elem in KINDS:
        opt_k, opt_t = make(label, extra), make(label, extra)
        ws = [torch.randn(n, device=dev, generator=gen) for _ in range(a.sets)]
        gs = [torch.randn(n, device=dev, generator=gen) for _ in range(a.sets)]

        def kernel(opt=opt_k, ws=ws, gs=gs, label=label):
            k = rotate(("dense", label), len(ws))
            opt.update(k, ws[k], gs[k])

        def composed(opt=opt_t, ws=ws, gs=gs, label=label):
            k = rotate(("torch", label), len(ws))
            st = opt.state.setdefault(k, {"t": 0})
            names = opt._state_names()
            for s in names:
                if s not in st:
                    st[s] = torch.zeros_like(ws[k])
            opt._update_torch(st, names, ws[k], gs[k])

        arms += [(f"dense {label}: tony_kv_opt_dense", per_elem * n, kernel, ("dense", label, "kernel")),
                 (f"dense {label}: torch composition", per_elem * n, composed, ("dense", label, "torch"))]
        copies.add(per_elem * n)

    # -- lazy
    R, D, nnz = a.rows, 64, a.nnz
    rb = 4 * D
    table = torch.randn(R, D, device=dev, generator=gen)
    id_sets = []
    for _ in range(a.id_sets):
        ids = torch.unique(torch.randint(0, R, (nnz,), device=dev, generator=gen))
        while ids.numel() < nnz:  # exactly nnz distinct rows
            ids = torch.unique(torch.cat([ids, torch.randint(0, R, (nnz - ids.numel(),), device=dev, generator=gen)]))
        id_sets.append(ids)
    grad = torch.randn(nnz, D, device=dev, generator=gen)
    for label, extra, per_elem in KINDS:
        opt_k, opt_g = make(label, extra), make(label, extra)
        moved = nnz * (per_elem // 4 * rb + 8)

        def rows(opt=opt_k, label=label):
            opt.update_rows(0, table, id_sets[rotate(("rows", label), len(id_sets))], grad)

        def generic(opt=opt_g, label=label):
            opt.update_rows_generic(0, table, id_sets[rotate(("generic", label), len(id_sets))], grad)

        arms += [(f"lazy {label}: tony_kv_opt_rows", moved, rows, ("lazy", label, "kernel")),
                 (f"lazy {label}: gather/update/scatter", moved, generic, ("lazy", label, "torch"))]
    sgd = K.Optimizer("sgd", learning_rate=0.01, momentum=0.9, wd=1e-4, rescale_grad=0.5)

    def lazy_sgd():
        sgd.update_rows(0, table, id_sets[rotate("sgd", len(id_sets))], grad)

    arms.append(("lazy sgd momentum: tony_kv_rsp_sgd", nnz * (5 * rb + 8), lazy_sgd, ("lazy", "sgd", "kernel")))

    # -- a plain copy moving the same bytes as each dense arm (half read, half written), from and to HBM
    pool = 1 << 30
    src_pool = torch.empty(pool, dtype=torch.uint8, device=dev)
    dst_pool = torch.empty(pool, dtype=torch.uint8, device=dev)
    for nbytes in sorted(copies):
        half = nbytes // 2 // 16 * 16
        at = [0]

        def copy(half=half, at=at):
            at[0] += 1
            s = src_pool.data_ptr() + at[0] * half % (pool - half) // 16 * 16
            d = dst_pool.data_ptr() + at[0] * half % (pool - half) // 16 * 16
            _lib.check(L.tony_kv_copy(d, s, half, None, stream), "copy")

        arms.append((f"tony_kv_copy {2 * half / 1e6:.0f} MB from HBM", 2 * half, copy, ("copy", nbytes, "kernel")))

    for _, _, fn, _ in arms:  # warm up: code objects loaded, clocks up, every state allocated
        for _ in range(max(5, a.sets)):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in arms}
    for _ in range(a.rounds):
        for name, _, fn, _ in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    print(f"dense key {n} fp32 ({4 * n / 1e6:.0f} MB) x {a.sets} buffer sets; table {R} x {D} fp32 "
          f"({R * rb / 2 ** 30:.2f} GiB), nnz {nnz}; {a.launches} launches per window, {a.rounds} rounds, arms "
          f"alternating")
    med = {}
    for name, nbytes, _, tag in arms:
        v = ms[name]
        med[tag] = m = statistics.median(v)
        rate = [nbytes / t / 1e9 for t in (m, max(v), min(v))]  # TB/s (bytes / ms / 1e9)
        print(f"{name:46s} {m:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {nbytes / 1e6:7.1f} MB  "
              f"{rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. {rate[2]:.2f})")
    print("ratios of the medians (kernel time / the other arm's time; below 1: the kernel is faster)")
    for label, _, per_elem in KINDS:
        k = med[("dense", label, "kernel")]
        print(f"dense {label:18s} / torch composition {k / med[('dense', label, 'torch')]:5.2f}   / copy of the same "
              f"bytes {k / med[('copy', per_elem * n, 'kernel')]:5.2f}")
    for label, _, per_elem in KINDS:
        k = med[("lazy", label, "kernel")]
        streams = per_elem // 4
        print(f"lazy  {label:18s} / gather/update/scatter {k / med[('lazy', label, 'torch')]:5.2f}   / lazy sgd x "
              f"{streams}/5 row streams {k / (med[('lazy', 'sgd', 'kernel')] * streams / 5):5.2f}")


if __name__ == "__main__":
    main()
