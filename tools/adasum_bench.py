#!/usr/bin/env python3
"""Device-event timing of the Adasum kernels (csrc/adasum.hip) beside the torch composition of the same level and a
plain copy of the same bytes, the method of tools/kv_sparse_bench.py: 100 launches per window, the arms taking turns
window by window so drift hits all of them alike.

    python tools/adasum_bench.py [--launches 100] [--rounds 5]

Two layouts, each in fp32 and bf16: the Inception-v3 flat buffer (its 292 parameter tensors at the flat buffers'
alignment, 27.2 M elements) and one 8 MB bucket of it (the first tensors that fill 8 MB).  The whole-buffer arms
rotate through ``--sets`` pairs of buffers launch by launch (more than the 256 MB Infinity Cache holds), so both sides
come from HBM; the bucket arms read the same 8 MB pair every launch, as a level reads a bucket that backward has just
written and a side that has just arrived: served from the caches, and so is the copy beside them.

  tony_adasum_dots      reads both sides: 2 n e bytes (e the element size)
  tony_adasum_coef      reads the item triples, writes T coefficient pairs: latency, not bandwidth
  tony_adasum_combine   reads both sides, writes one: 3 n e bytes
  dots + coef + combine one level's three launches: 5 n e bytes
  torch composition     per tensor three torch.dot, the two ratios, two mul and one add (a tenth of the launches per
                        window: it is some 3000 launches for the whole buffer)
  tony_kv_copy          a plain copy of the same number of bytes as dots / combine / the three move

Prints per arm the median / min / max ms per launch over the rounds and the rate the bytes it must move imply.  Every
process here is on one GPU: what a level costs on the links (log2(N) exchanges of the whole buffer against a ring's
2 (N-1)/N) is not visible and is not measured.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    from tony_amd.models.inception_v3 import inception_v3
    from tony_amd.ops import _lib
    from tony_amd.ops.adasum import TINY, AdasumPlan, apply_, coef_, dots_
    from tony_amd.ops.optim import Segments

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    sizes = [p.numel() for p in inception_v3(fused=False).parameters() if p.requires_grad]
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + (n + 63) // 64 * 64)
    print(f"Inception-v3: {len(sizes)} tensors, {starts[-1]} elements; {a.launches} launches per window, {a.rounds} "
          f"rounds, arms alternating")
    for dtype in (torch.float32, torch.bfloat16):
        esz = dtype.itemsize
        k = next(i for i, s in enumerate(starts) if s * esz >= 8 << 20)
        for label, st, sets in ((f"whole buffer {dtype}", starts, a.sets), (f"8 MB bucket {dtype}", starts[:k + 1], 1)):
            n = st[-1]
            plan = AdasumPlan(Segments(st, list(range(len(st) - 1)), [True] * (len(st) - 1)), dtype, dev)
            pairs = [(torch.randn(n, device=dev).to(dtype), torch.randn(n, device=dev).to(dtype)) for _ in range(sets)]
            tmp = torch.empty(n, dtype=dtype, device=dev)
            turn = {}

            def nxt(arm):
                turn[arm] = (turn.get(arm, -1) + 1) % sets
                return pairs[turn[arm]]

            def dots():
                dots_(*nxt("dots"), plan)

            def coef():
                coef_(plan)

            def combine():
                x, y = nxt("combine")
                apply_(x, y, True, plan)

            def three():
                x, y = nxt("three")
                dots_(x, y, plan)
                coef_(plan)
                apply_(x, y, True, plan)

            one = torch.ones((), device=dev)

            def composed():
                x, y = nxt("torch")
                for lo, hi in zip(st, st[1:]):
                    xa, yb = x[lo:hi], y[lo:hi]
                    dot, na, nb = torch.dot(xa, yb), torch.dot(xa, xa), torch.dot(yb, yb)
                    ca = torch.where(na >= TINY, 1 - dot / (2 * na), one)
                    cb = torch.where(nb >= TINY, 1 - dot / (2 * nb), one)
                    torch.mul(yb, cb, out=tmp[lo:hi])
                    torch.mul(xa, ca, out=xa)
                    torch.add(xa, tmp[lo:hi], out=xa)

            arms = [("tony_adasum_dots", 2 * n * esz, dots), ("tony_adasum_coef", 0, coef),
                    ("tony_adasum_combine", 3 * n * esz, combine), ("dots + coef + combine", 5 * n * esz, three),
                    ("torch composition", 5 * n * esz, composed)]
            for nbytes in (2 * n * esz, 3 * n * esz, 5 * n * esz):  # a plain copy moving the same bytes
                half = nbytes // 2 // 16 * 16
                src = torch.empty(half * sets, dtype=torch.uint8, device=dev)
                dst = torch.empty(half * sets, dtype=torch.uint8, device=dev)
                at = [0]

                def copy(src=src, dst=dst, half=half, at=at):
                    at[0] = (at[0] + 1) % sets
                    _lib.check(L.tony_kv_copy(dst.data_ptr() + at[0] * half, src.data_ptr() + at[0] * half, half, None,
                                              stream), "copy")

                arms.append((f"tony_kv_copy {2 * half / 2 ** 20:.0f} MiB", 2 * half, copy))
            for _, _, fn in arms:  # warm up: code objects loaded, clocks up
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _, _ in arms}
            for _ in range(a.rounds):
                for name, _, fn in arms:
                    for p in pairs:  # keep the values finite: a combine scales its a side every launch
                        p[0].copy_(p[1])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches if name != "torch composition" else max(1, a.launches // 10)):
                        fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / (a.launches if name != "torch composition"
                                                           else max(1, a.launches // 10)))
            print(f"-- {label}: {n} elements, {plan.n_tensors} tensors, {plan.n_items} items, "
                  f"{'rotating over ' + str(sets) + ' pairs (from HBM)' if sets > 1 else 'one pair (cached)'}")
            for name, nbytes, _ in arms:
                v = ms[name]
                med = statistics.median(v)
                rate = [nbytes / t / 1e9 for t in (med, max(v), min(v))]  # TB/s (bytes / ms / 1e9)
                tail = f"{nbytes / 2 ** 20:7.1f} MiB  {rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. " \
                       f"{rate[2]:.2f})" if nbytes else ""
                print(f"{name:24s} {med:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {tail}")
            del pairs, tmp, plan


if __name__ == "__main__":
    main()
