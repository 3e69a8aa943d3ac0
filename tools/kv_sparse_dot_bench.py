#!/usr/bin/env python3
"""Device-event timing of the kvstore's CSR dot kernels (csrc/kv_sparse_dot.hip) beside the torch compositions they
replace, the method of tools/kv_sparse_bench.py: 100 launches per window, the arms taking turns window by window so
drift hits all of them alike.

    python tools/kv_sparse_dot_bench.py [--launches 100] [--rounds 5]

Three shapes: the sparse linear job's (F = 100000, D = 16, 1024 samples x 8 active), the sparse bench's (a 4 M x 64
table, 8192 samples x 8 active drawn uniformly) and the second again with the columns drawn from a skewed
distribution (column = floor(F u^3), u uniform: the first columns occur hundreds of times in the batch).  ``w`` is
what a worker holds after ``row_sparse_pull``: the batch's unique rows.  Every launch reads the same operands (a
worker's pulled rows and its batch have just been written: they are served from the caches, and so is the copy
beside them).

  tony_kv_csr_dot       h = x . w                      against  searchsorted + index_select + view(B, active, D).sum(1)
  tony_kv_rows_segsum   the sums of from_rows behind   against  the loop of RowSparse.from_rows behind its sort, one
                        its sort, one launch                    host synchronisation and three or four launches a level
  tony_kv_copy          a plain copy of the same number of bytes as each kernel moves

Prints per arm the median / min / max ms per launch over the rounds and the rate the bytes it must move imply, and
per pair whether the kernel's slowest round is below the composition's fastest.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def from_rows_tail(rows, order, starts, counts):
    """The lines of ``RowSparse.from_rows`` behind its sort as they were before ``tony_kv_rows_segsum``."""
    acc = rows.index_select(0, order.index_select(0, starts)).float()
    for k in range(1, int(counts.max())):
        sel = (counts > k).nonzero().reshape(-1)
        nxt = rows.index_select(0, order.index_select(0, starts.index_select(0, sel) + k)).float()
        acc.index_copy_(0, sel, acc.index_select(0, sel) + nxt)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from tony_amd.ops import _lib
    from tony_amd.parallel import kvstore as K

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    arms, pairs, copies = [], [], set()
    for shape, F, D, B, active, skew in (("job", 100000, 16, 1024, 8, False), ("uniform", 4 << 20, 64, 8192, 8, False),
                                         ("skewed", 4 << 20, 64, 8192, 8, True)):
        E, rb = B * active, 4 * D
        if skew:
            cols = (F * torch.rand(E, device=dev, generator=gen) ** 3).long().clamp_(max=F - 1)
        else:
            cols = torch.randint(0, F, (E,), device=dev, generator=gen)
        x = K.CSR(torch.arange(B + 1, device=dev) * active, cols, shape=(B, F))
        uniq, starts, order, _ = x.plan()
        nu = uniq.numel()
        counts = starts[1:] - starts[:-1]
        w = K.RowSparse(uniq, torch.randn(nu, D, device=dev, generator=gen), (F, D), _checked=True)
        occ = torch.randn(E, D, device=dev, generator=gen)  # a gradient row per occurrence, as autograd leaves them
        print(f"{shape}: F {F}, D {D}, {B} samples x {active} active, {nu} unique columns, the most frequent "
              f"{int(counts.max())} times")

        def csr_dot(x=x, w=w):
            K.dot(x, w)

        def csr_dot_torch(x=x, w=w, B=B, active=active, D=D):
            pos = torch.searchsorted(w.indices, x.indices)
            w.data.index_select(0, pos).view(B, active, D).sum(1)

        def segsum(occ=occ, starts=starts, order=order, E=E, D=D):
            K._rows_segsum(occ, starts, order, None, None, E, D)

        def segsum_torch(occ=occ, order=order, first=starts[:-1].contiguous(), counts=counts):
            from_rows_tail(occ, order, first, counts)

        fwd = E * (rb + 8) + B * rb + 8 * (B + 1)     # ids and rows read per entry, indptr, the output
        tail = E * (rb + 8) + nu * (rb + 8)           # entry numbers and rows read per entry, starts, the output
        # both pairs compute the same thing (the composition's sum(1) has no fixed order: within rounding only)
        assert torch.allclose(K.dot(x, w), w.data.index_select(0, torch.searchsorted(w.indices, cols)).view(
            B, active, D).sum(1), rtol=1e-4, atol=1e-4)
        assert torch.equal(K._rows_segsum(occ, starts, order, None, None, E, D),
                           from_rows_tail(occ, order, starts[:-1].contiguous(), counts))
        arms += [(f"{shape}: tony_kv_csr_dot", fwd, csr_dot), (f"{shape}: searchsorted/select/sum", fwd, csr_dot_torch),
                 (f"{shape}: tony_kv_rows_segsum", tail, segsum), (f"{shape}: from_rows loop", tail, segsum_torch)]
        pairs += [(arms[-4][0], arms[-3][0]), (arms[-2][0], arms[-1][0])]
        copies |= {fwd, tail}
    for nbytes in sorted(copies):  # a plain copy moving the same bytes (half read, half written)
        half = nbytes // 2 // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)

        def copy(src=src, dst=dst, half=half):
            _lib.check(L.tony_kv_copy(dst.data_ptr(), src.data_ptr(), half, None, stream), "copy")

        arms.append((f"tony_kv_copy {2 * half / 2 ** 20:.2f} MiB", 2 * half, copy))
    for _, _, fn in arms:  # warm up: code objects loaded, clocks up, the allocator's blocks made
        for _ in range(3):
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
    print(f"{a.launches} launches per window, {a.rounds} rounds, arms alternating")
    for name, nbytes, _ in arms:
        v = ms[name]
        med = statistics.median(v)
        print(f"{name:38s} {med:9.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {nbytes / 2 ** 20:7.2f} MiB  "
              f"{nbytes / med / 1e9:6.3f} TB/s")
    for kern, comp in pairs:
        ok = max(ms[kern]) < min(ms[comp])
        print(f"{kern}: slowest round {max(ms[kern]):.4f} ms {'<' if ok else '>='} the composition's fastest "
              f"{min(ms[comp]):.4f} ms: {'faster' if ok else 'NOT faster'} ({min(ms[comp]) / max(ms[kern]):.1f}x)")


if __name__ == "__main__":
    main()
