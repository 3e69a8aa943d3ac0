#!/usr/bin/env python3
"""Device-event timing of the synchronised-BatchNorm kernels (csrc/syncbn.hip) beside their unsynchronised
counterparts (csrc/bn_act.hip) and a plain copy of the same bytes, the method of tools/adasum_bench.py: 100 launches
per window, the arms taking turns window by window so drift hits all of them alike.

    python tools/syncbn_bench.py [--launches 100] [--rounds 5] [--sets 8]

Shapes: ResNet-50 BN layers at per-GPU batch 32, bf16: [32*56*56, 256], [32*28*28, 512], [32*7*7, 2048].  Every arm
walks ``--sets`` sets of buffers launch by launch so the rows come from HBM (the small 7x7 layer stays cached whatever
one does: 6.4 MB a tensor).

  tony_syncbn_stats (+ fold)   reads x: M C e bytes       beside tony_bn_stats (also each of the two alone; the fold
                               reads the grid x 2C double partials)
  tony_syncbn_apply            reads x, writes y: 2 M C e  beside tony_bn_apply
  tony_syncbn_bwd_reduce       reads x, dy: 2 M C e        beside tony_bn_bwd_reduce
  tony_syncbn_bwd_apply        reads x, dy, writes dx: 3   beside tony_bn_bwd_apply
  tony_syncbn_merge / _bwd_merge at W = 1 and W = 8: latency, not bandwidth
  tony_kv_copy                 a plain copy moving the same number of bytes as each of the four row passes

Prints per arm the median / min / max ms per launch over the rounds and the rate its bytes imply.  One GPU: what the
two small all-gathers per BN layer cost on the links (latency-bound) is not visible here and is not measured.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [(32 * 56 * 56, 256), (32 * 28 * 28, 512), (32 * 7 * 7, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=8)
    a = ap.parse_args()
    from tony_amd.ops import _lib

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    s = _lib.stream_ptr(dev)
    bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64
    print(f"{a.launches} launches per window, {a.rounds} rounds, arms alternating, {a.sets} buffer sets")
    for M, C in SHAPES:
        sets = a.sets
        xs = [torch.randn(M, C, device=dev).to(bf) for _ in range(sets)]
        dys = [torch.randn(M, C, device=dev).to(bf) for _ in range(sets)]
        outs = [torch.empty(M, C, dtype=bf, device=dev) for _ in range(sets)]
        g, b = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        mean, invstd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        G = L.tony_syncbn_grid(M, C)
        part, packet, ab = (torch.empty(n, dtype=f64, device=dev) for n in (G * 2 * C, 1 + 2 * C, 2 * C))
        coef, tab = torch.empty(2 * C, device=dev), torch.empty(5 * C, device=dev)
        count = torch.empty(1, dtype=f64, device=dev)
        ws = torch.zeros(_lib.stat_floats(C) + 4, dtype=f32, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        turn = {}

        def nxt(arm):
            turn[arm] = (turn.get(arm, -1) + 1) % sets
            return turn[arm]

        def ck(rc, name):
            _lib.check(rc, name)

        def stats_new():
            x = xs[nxt("sn")]
            ck(L.tony_syncbn_stats(x.data_ptr(), M, C, C, 0, part.data_ptr(), s), "stats")
            ck(L.tony_syncbn_fold(part.data_ptr(), G, C, packet.data_ptr(), M, s), "fold")

        def stats_only():
            x = xs[nxt("s1")]
            ck(L.tony_syncbn_stats(x.data_ptr(), M, C, C, 0, part.data_ptr(), s), "stats")

        def fold_only():
            ck(L.tony_syncbn_fold(part.data_ptr(), G, C, packet.data_ptr(), M, s), "fold")

        def stats_old():
            x = xs[nxt("so")]
            ck(L.tony_bn_stats(x.data_ptr(), M, C, C, ws.data_ptr(), ws.data_ptr() + 4 * C, 2 * C, s), "bn_stats")

        def apply_new():
            i = nxt("an")
            ck(L.tony_syncbn_apply(xs[i].data_ptr(), M, C, C, 0, 0, outs[i].data_ptr(), C, 0, coef.data_ptr(), 1, s),
               "apply")

        def apply_old():
            i = nxt("ao")
            ck(L.tony_bn_apply(xs[i].data_ptr(), M, C, C, outs[i].data_ptr(), C, ws.data_ptr(), ws.data_ptr() + 4 * C,
                               2 * C, g.data_ptr(), b.data_ptr(), 0, 1e-5, 1, 0, mean.data_ptr(), invstd.data_ptr(),
                               rm.data_ptr(), rv.data_ptr(), 0.1, s), "bn_apply")

        def red_new():
            i = nxt("rn")
            ck(L.tony_syncbn_bwd_reduce(xs[i].data_ptr(), C, dys[i].data_ptr(), C, 0, 0, M, C, 0, mean.data_ptr(),
                                        invstd.data_ptr(), g.data_ptr(), b.data_ptr(), 0, 1, part.data_ptr(),
                                        ab.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, s), "bwd_reduce")

        def red_old():
            i = nxt("ro")
            ck(L.tony_bn_bwd_reduce(xs[i].data_ptr(), C, dys[i].data_ptr(), C, M, C, mean.data_ptr(), invstd.data_ptr(),
                                    g.data_ptr(), b.data_ptr(), 0, 1, ws.data_ptr(), ws.data_ptr() + 4 * C, 2 * C, s),
               "bn_bwd_reduce")

        def bapply_new():
            i = nxt("bn")
            ck(L.tony_syncbn_bwd_apply(xs[i].data_ptr(), C, dys[i].data_ptr(), C, 0, 0, 0, 0, outs[i].data_ptr(), C, M,
                                       C, 0, tab.data_ptr(), 1, s), "bwd_apply")

        def bapply_old():
            i = nxt("bo")
            ck(L.tony_bn_bwd_apply(xs[i].data_ptr(), C, dys[i].data_ptr(), C, outs[i].data_ptr(), C, M, C,
                                   mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), b.data_ptr(), 0, 1, ws.data_ptr(),
                                   ws.data_ptr() + 4 * C, 2 * C, dg.data_ptr(), db.data_ptr(), 0, s), "bn_bwd_apply")

        e = 2
        arms = [("tony_syncbn_stats + fold", M * C * e, stats_new), ("tony_syncbn_stats", M * C * e, stats_only),
                ("tony_syncbn_fold", G * 2 * C * 8, fold_only), ("tony_bn_stats", M * C * e, stats_old),
                ("tony_syncbn_apply", 2 * M * C * e, apply_new), ("tony_bn_apply", 2 * M * C * e, apply_old),
                ("tony_syncbn_bwd_reduce", 2 * M * C * e, red_new), ("tony_bn_bwd_reduce", 2 * M * C * e, red_old),
                ("tony_syncbn_bwd_apply", 3 * M * C * e, bapply_new), ("tony_bn_bwd_apply", 3 * M * C * e, bapply_old)]
        for W in (1, 8):
            gp = torch.rand(W, 1 + 2 * C, dtype=f64, device=dev) + 1
            gp[:, 0] = M
            gab = torch.rand(W, 2 * C, dtype=f64, device=dev)

            def merge(gp=gp, W=W):
                ck(L.tony_syncbn_merge(gp.data_ptr(), W, C, g.data_ptr(), b.data_ptr(), 0, 1e-5, 0.1, mean.data_ptr(),
                                       invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), coef.data_ptr(),
                                       count.data_ptr(), s), "merge")

            def bmerge(gab=gab, W=W):
                ck(L.tony_syncbn_bwd_merge(gab.data_ptr(), W, C, count.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                           g.data_ptr(), b.data_ptr(), 0, tab.data_ptr(), s), "bwd_merge")

            arms += [(f"tony_syncbn_merge W={W}", 0, merge), (f"tony_syncbn_bwd_merge W={W}", 0, bmerge)]
        for k in (1, 2, 3):  # a plain copy moving the same bytes as the row passes
            half = k * M * C * e // 2 // 16 * 16
            src = torch.empty(half * sets, dtype=torch.uint8, device=dev)
            dst = torch.empty(half * sets, dtype=torch.uint8, device=dev)
            at = [0]

            def copy(src=src, dst=dst, half=half, at=at):
                at[0] = (at[0] + 1) % sets
                ck(L.tony_kv_copy(dst.data_ptr() + at[0] * half, src.data_ptr() + at[0] * half, half, None, s), "copy")

            arms.append((f"tony_kv_copy {2 * half / 2 ** 20:.0f} MiB", 2 * half, copy))
        for _, _, fn in arms:  # warm up: code objects loaded, clocks up (merge first: the apply arms read its tables)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        for _ in range(a.rounds):
            for name, _, fn in arms:
                ws.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.launches)
        print(f"-- [{M}, {C}] bf16, {M * C * e / 2 ** 20:.1f} MiB a tensor, reduction grid {G}")
        for name, nbytes, _ in arms:
            v = ms[name]
            med = statistics.median(v)
            tail = ""
            if nbytes:
                rate = [nbytes / t / 1e9 for t in (med, max(v), min(v))]  # TB/s (bytes / ms / 1e9)
                tail = (f"{nbytes / 2 ** 20:7.1f} MiB  {rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. "
                        f"{rate[2]:.2f})")
            print(f"{name:28s} {med:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {tail}")
        del xs, dys, outs


if __name__ == "__main__":
    main()
