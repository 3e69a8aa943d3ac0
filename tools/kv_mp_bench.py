#!/usr/bin/env python3
"""Device-event timing of the kvstore's multi-precision round kernel (csrc/kv_mp.hip, ``tony_kv_mp_dense``) beside the
torch composition of the same contract on the same buffers, beside ``tony_kv_opt_dense`` of the fp32 kind with the
same state tensors and beside plain copies of the same bytes, the method of tools/kv_optim_bench.py: 100 launches per
window, the arms taking turns window by window so drift hits all of them alike.

    python tools/kv_mp_bench.py [--launches 100] [--rounds 5] [--mb 64] [--sets 4]

A bf16 key of ``--mb`` MB of fp32 elements (16 M by default) under lazy SGD with momentum and under centered rmsprop,
with 1 and 4 bf16 sources.  Every arm walks ``--sets`` buffer sets (stored value, master, states, sources) launch by
launch, several times the 256 MB Infinity Cache, so its bytes come from HBM.  The bytes a round must move, per
element: 2 per bf16 source read, 8 for the master and for each state (read and written), 2 for the stored value
written -- 20 and 26 B for SGD with momentum (one state), 36 and 42 B for centered rmsprop (three).  The fp32 arms move
20 B (nag with momentum: the fp32 kind with SGD's one state) and 36 B.  A ``tony_kv_copy`` of each byte count (half
read, half written) rotates through 1 GiB buffers.  Prints per arm the median / min / max ms per launch over the
rounds and the rate those bytes imply, then each kernel's rate as a fraction of its copy's, and whether the kernel's
slowest round beats the composition's fastest.  Every process here is on one GPU: the halving of the bytes a 16-bit
push and pull move over a link is not visible and is not measured.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KINDS = [("sgd momentum", "sgd", dict(momentum=0.9), 1, "nag"), ("rmsprop centered", "rmsprop", dict(centered=True), 3,
                                                                 "rmsprop")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.parallel import kvstore as K

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    n = a.mb * 1000 * 1000 // 4
    arms, copies, turn, mp_opts = [], set(), {}, []

    def rotate(arm, count):
        turn[arm] = (turn.get(arm, -1) + 1) % count
        return turn[arm]

    def make(name, extra, **kw):
        return K.Optimizer(name, learning_rate=0.01, wd=1e-4, rescale_grad=0.5, **extra, **kw)

    for label, name, extra, ns, fp32_name in KINDS:
        srcs = [[torch.randn(n, device=dev, generator=gen).bfloat16() for _ in range(4)] for _ in range(a.sets)]
        for k in (1, 4):
            per_elem = 2 * k + 8 + 8 * ns + 2
            opt_k, opt_t = make(name, extra, multi_precision=True), make(name, extra, multi_precision=True)
            mp_opts.append(opt_k)
            ws = [[torch.randn(n, device=dev, generator=gen).bfloat16() for _ in range(a.sets)] for _ in range(2)]

            def kernel(opt=opt_k, ws=ws[0], k=k, tag=("mp", label, k)):
                i = rotate(tag, len(ws))
                opt.update(i, ws[i], srcs[i][:k])

            def composed(opt=opt_t, ws=ws[1], k=k, tag=("torch", label, k)):
                i = rotate(tag, len(ws))
                names = opt._mp_names()
                opt._update_mp_torch(i, ws[i], opt._mp_state(i, ws[i], names), names, srcs[i][:k])

            arms += [(f"{label} x{k}: tony_kv_mp_dense", per_elem * n, kernel, ("mp", label, k)),
                     (f"{label} x{k}: torch composition", per_elem * n, composed, ("torch", label, k))]
            copies.add(per_elem * n)
        opt_f = make(fp32_name, extra)
        wf = [torch.randn(n, device=dev, generator=gen) for _ in range(a.sets)]
        gf = [torch.randn(n, device=dev, generator=gen) for _ in range(a.sets)]

        def fp32(opt=opt_f, tag=("fp32", label)):
            i = rotate(tag, len(wf))
            opt.update(i, wf[i], gf[i])

        arms.append((f"{label} fp32 ({fp32_name}): tony_kv_opt_dense", (12 + 8 * ns) * n, fp32, ("fp32", label, 0)))
        copies.add((12 + 8 * ns) * n)

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

        arms.append((f"tony_kv_copy {2 * half / 1e6:.0f} MB from HBM", 2 * half, copy, ("copy", nbytes, 0)))

    for _, _, fn, _ in arms:  # warm up: code objects loaded, clocks up, every master and state allocated
        for _ in range(max(5, a.sets)):
            fn()
    torch.cuda.synchronize()
    assert all(o.kernel_ops[2] > 0 for o in mp_opts)  # the kernel arms launch the kernel
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
    print(f"bf16 key of {n} elements ({4 * n / 1e6:.0f} MB of fp32) x {a.sets} buffer sets; {a.launches} launches per "
          f"window, {a.rounds} rounds, arms alternating")
    med, rng = {}, {}
    for name, nbytes, _, tag in arms:
        v = ms[name]
        med[tag], rng[tag] = statistics.median(v), (min(v), max(v))
        rate = [nbytes / t / 1e9 for t in (med[tag], max(v), min(v))]  # TB/s (bytes / ms / 1e9)
        print(f"{name:52s} {med[tag]:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {nbytes / 1e6:7.1f} MB  "
              f"{rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. {rate[2]:.2f})")
    print("fraction of the copy's rate (copy time / kernel time at the same bytes, medians); the kernel's slowest round "
          "against the composition's fastest")
    for label, _, _, ns, fp32_name in KINDS:
        for k in (1, 4):
            nb = (2 * k + 8 + 8 * ns + 2) * n
            beats = rng[("mp", label, k)][1] < rng[("torch", label, k)][0]
            print(f"{label:18s} x{k}  tony_kv_mp_dense {med[('copy', nb, 0)] / med[('mp', label, k)]:5.2f}   slowest "
                  f"{rng[('mp', label, k)][1]:.4f} ms {'<' if beats else '>='} composition's fastest "
                  f"{rng[('torch', label, k)][0]:.4f} ms   / composition {med[('mp', label, k)] / med[('torch', label, k)]:5.2f}")
        nb = (12 + 8 * ns) * n
        print(f"{label:18s} fp32 tony_kv_opt_dense ({fp32_name}) {med[('copy', nb, 0)] / med[('fp32', label, 0)]:5.2f}")


if __name__ == "__main__":
    main()
