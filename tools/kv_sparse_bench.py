#!/usr/bin/env python3
"""Device-event timing of the kvstore's row-sparse kernels (csrc/ps_plane.hip) beside the torch compositions they
replace, the method of tools/kv_compress_bench.py: 100 launches per window, the arms taking turns window by window
so drift hits all of them alike.

    python tools/kv_sparse_bench.py [--launches 100] [--rounds 5] [--rows 4194304] [--nnz 65536]

The table is ``--rows`` x 64 fp32 (1 GiB by default) and ``--nnz`` random rows of it are touched.  The gather and
SGD arms rotate through ``--sets`` different row sets launch by launch (32 x 16 MiB of rows by default, more than
the 256 MB Infinity Cache holds), and the copy beside them rotates its source through the table and its destination
through a 512 MiB buffer, so their rows come from HBM.  The merge arms read the same compact sources every launch
(16 MiB each, as a server reads push buffers that have just arrived): those are served from the caches, and so is
the copy beside them.

  tony_kv_rsp_gather        rows out of the table                            against  torch.index_select
  tony_kv_rsp_merge x2, x8  the ordered sum of 2 / 8 sources of nnz rows     against  index_add_ into a zeroed
                            each into their union                                     union buffer (positions given)
  tony_kv_rsp_sgd           lazy SGD with momentum on the touched rows       against  gather / Optimizer.update /
                                                                                      scatter (the generic path)
  tony_kv_copy              a plain copy of the same number of bytes as each kernel moves

Prints per arm the median / min / max ms per launch over the rounds and the rate the bytes it must move imply.
Every process here is on one GPU: what row-sparse keys save on the link to a server (R / nnz of a dense push or
pull) is not visible and is not measured.
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--nnz", type=int, default=65536)
    ap.add_argument("--sets", type=int, default=32)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.parallel import kvstore as K

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    R, D, nnz = a.rows, 64, a.nnz
    rb = 4 * D
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(R, D, device=dev, generator=gen)
    id_sets = []
    for _ in range(a.sets):
        ids = torch.unique(torch.randint(0, R, (nnz,), device=dev, generator=gen))
        while ids.numel() < nnz:  # exactly nnz distinct rows
            ids = torch.unique(torch.cat([ids, torch.randint(0, R, (nnz - ids.numel(),), device=dev, generator=gen)]))
        id_sets.append(ids)
    turn = {}

    def next_ids(arm):  # every arm walks the row sets in the same order
        turn[arm] = (turn.get(arm, -1) + 1) % len(id_sets)
        return id_sets[turn[arm]]

    grad = torch.randn(nnz, D, device=dev, generator=gen)
    out = torch.empty(nnz, D, device=dev)
    arms = []

    def gather():
        ids = next_ids("gather")
        _lib.check(L.tony_kv_rsp_gather(out.data_ptr(), table.data_ptr(), ids.data_ptr(), nnz, rb, R, None, None,
                                        stream), "gather")

    def gather_torch():
        torch.index_select(table, 0, next_ids("gather_torch"), out=out)

    moved = 2 * nnz * rb + 8 * nnz
    arms += [("tony_kv_rsp_gather", moved, gather), ("torch.index_select", moved, gather_torch)]
    copies = {(moved, True)}

    for nsrc in (2, 8):
        srcs = []
        for _ in range(nsrc):  # each source nnz rows out of a pool of 2 nnz: about half of every pair overlaps
            pick = torch.randperm(2 * nnz, device=dev, generator=gen)[:nnz].sort().values
            srcs.append((pick.contiguous(), torch.randn(nnz, D, device=dev, generator=gen)))
        union = torch.unique(torch.cat([i for i, _ in srcs]))
        nu = union.numel()
        pos = [torch.searchsorted(union, i) for i, _ in srcs]
        dst = torch.empty(nu, D, device=dev)
        arr = ctypes.c_int64 * nsrc
        tabs = (arr(*[i.data_ptr() for i, _ in srcs]), arr(*[r.data_ptr() for _, r in srcs]), arr(*[nnz] * nsrc))

        def merge(dst=dst, union=union, nu=nu, tabs=tabs, nsrc=nsrc):
            _lib.check(L.tony_kv_rsp_merge(dst.data_ptr(), union.data_ptr(), nu, *tabs, nsrc, D, stream), "merge")

        def merge_torch(dst=dst, srcs=srcs, pos=pos):
            dst.zero_()
            for (_, rows), p in zip(srcs, pos):
                dst.index_add_(0, p, rows)

        moved = nsrc * nnz * (rb + 8) + nu * (rb + 8)
        arms += [(f"tony_kv_rsp_merge x{nsrc}", moved, merge), (f"zero_ + index_add_ x{nsrc}", moved, merge_torch)]
        copies.add((moved, False))

    opt = K.Optimizer("sgd", learning_rate=0.01, momentum=0.9, wd=1e-4, rescale_grad=0.5)

    def sgd():
        opt.update_rows(0, table, next_ids("sgd"), grad)

    def sgd_generic():
        opt.update_rows_generic(0, table, next_ids("sgd_generic"), grad)

    moved = nnz * (5 * rb + 8)  # gradient read, weight and momentum read and written
    arms += [("tony_kv_rsp_sgd", moved, sgd), ("gather/update/scatter", moved, sgd_generic)]
    copies.add((moved, True))
    far = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for nbytes, rotate in sorted(copies):  # a plain copy moving the same bytes (half read, half written)
        half = nbytes // 2 // 16 * 16
        src, dstc = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        at = [0]

        def copy(src=src, dstc=dstc, half=half, rotate=rotate, at=at):
            s, d = src.data_ptr(), dstc.data_ptr()
            if rotate:  # out of the table, into the far buffer, a fresh stretch of both every launch
                at[0] += 1
                s = table.data_ptr() + at[0] * half % (R * rb - half) // 16 * 16
                d = far.data_ptr() + at[0] * half % (far.numel() - half) // 16 * 16
            _lib.check(L.tony_kv_copy(d, s, half, None, stream), "copy")

        arms.append((f"tony_kv_copy {2 * half / 2 ** 20:.0f} MiB {'from HBM' if rotate else 'cached'}", 2 * half,
                     copy))
    for _, _, fn in arms:  # warm up: code objects loaded, clocks up, the momentum allocated
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, _, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    print(f"table {R} x {D} fp32 ({R * rb / 2 ** 30:.2f} GiB), nnz {nnz}; {a.launches} launches per window, "
          f"{a.rounds} rounds, arms alternating")
    for name, nbytes, _ in arms:
        v = ms[name]
        med = statistics.median(v)
        rate = [nbytes / t / 1e9 for t in (med, max(v), min(v))]  # TB/s (bytes / ms / 1e9)
        print(f"{name:30s} {med:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {nbytes / 2 ** 20:7.1f} MiB  "
              f"{rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. {rate[2]:.2f})")


if __name__ == "__main__":
    main()
