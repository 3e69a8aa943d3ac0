#!/usr/bin/env python3
"""Device-event timing of the kvstore's 2-bit gradient-compression kernels (csrc/ps_plane.hip) beside the copy
kernels they replace, the method of tools/optim_bench.py: fp32 keys of 8 MB and 64 MB, a local destination, 100
launches per window, the arms taking turns window by window so drift hits all of them alike.

    python tools/kv_compress_bench.py [--launches 100] [--rounds 5] [--no-round]

  tony_kv_copy_flag   the gradient into a window row: what a compressed push replaces        8    B / element
  tony_kv_quant2      residual + gradient -> residual, packed words                           12.25 B / element
  (and the same without the flag hand-off at its end, the launch of a push whose words go over gloo)
  tony_kv_copy        the server's read of a row                                              8    B / element
  tony_kv_dequant2    the server's read of a packed row (nsrc = 1)                            4.25 B / element

Prints per arm the median / min / max ms per launch over the rounds and the rate its bytes imply, then (unless
--no-round) the wall time of one dist_sync round of 8 keys of 8 MB -- a scheduler, one server and two workers as
processes on this GPU -- with and without compression.  With every process on one GPU no byte crosses a link: the
16-fold cut of the bytes a push sends to the server is not visible here.
"""
import argparse
import multiprocessing as mp
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernels(launches: int, rounds: int) -> None:
    from tony_amd.ops import _lib

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    arms = []
    keep = []
    for mb in (8, 64):
        n = mb * (1 << 20) // 4
        nw = (n + 15) // 16
        thr = 0.5
        grad = 0.7 * thr * torch.randn(n, device=dev)
        res = torch.zeros(n, device=dev)
        row = torch.empty(n, device=dev)
        out = torch.empty(n, device=dev)
        words = torch.empty(nw, dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        keep += [grad, res, row, out, words, flag]

        def copy_flag(grad=grad, row=row, flag=flag, n=n):
            _lib.check(L.tony_kv_copy_flag(row.data_ptr(), grad.data_ptr(), 4 * n, flag.data_ptr(), stream),
                       "copy_flag")

        def quant(grad=grad, res=res, words=words, flag=flag, n=n):
            _lib.check(L.tony_kv_quant2(words.data_ptr(), grad.data_ptr(), res.data_ptr(), n, thr, flag.data_ptr(),
                                        stream), "quant2")

        def quant_noflag(grad=grad, res=res, words=words, n=n):  # the gloo path's launch: no hand-off at its end
            _lib.check(L.tony_kv_quant2(words.data_ptr(), grad.data_ptr(), res.data_ptr(), n, thr, None, stream),
                       "quant2")

        def copy(row=row, out=out, n=n):
            _lib.check(L.tony_kv_copy(out.data_ptr(), row.data_ptr(), 4 * n, None, stream), "copy")

        def dequant(words=words, out=out, n=n, nw=nw):
            _lib.check(L.tony_kv_dequant2(out.data_ptr(), words.data_ptr(), n, thr, 1, nw, None, stream), "dequant2")

        arms += [(f"tony_kv_copy_flag {mb:2d} MB", 8.0, n, copy_flag),
                 (f"tony_kv_quant2    {mb:2d} MB", 12.25, n, quant),
                 (f"tony_kv_quant2, no flag {mb:2d} MB", 12.25, n, quant_noflag),
                 (f"tony_kv_copy      {mb:2d} MB", 8.0, n, copy), (f"tony_kv_dequant2  {mb:2d} MB", 4.25, n, dequant)]
    for _, _, _, fn in arms:  # warm up: code objects loaded, clocks up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in arms}
    for _ in range(rounds):
        for name, _, _, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / launches)
    print(f"{launches} launches per window, {rounds} rounds, arms alternating")
    for name, bpe, n, _ in arms:
        v = ms[name]
        med = statistics.median(v)
        rate = [bpe * n / t / 1e9 for t in (med, max(v), min(v))]  # TB/s (bytes / ms / 1e9)
        print(f"{name:28s} {med:7.4f} ms  (min {min(v):.4f}, max {max(v):.4f})  {bpe:5.2f} B/elem  "
              f"{rate[0]:5.2f} TB/s  (over the rounds {rate[1]:.2f} .. {rate[2]:.2f})")


def round_rank(role, index, port, steps, keys, key_mb, compress):
    """One member of a dist_sync store on this GPU: per-step wall time of push-all + pull-all."""
    os.environ.update(DMLC_ROLE=role, DMLC_NUM_SERVER="1", DMLC_NUM_WORKER="2", DMLC_PS_ROOT_URI="127.0.0.1",
                      DMLC_PS_ROOT_PORT=str(port), TASK_INDEX=str(index), TONY_KV_WAIT_S="60",
                      TONY_KV_WINDOW_MB=str(2 * keys * key_mb + 64))
    import tony_amd.kv as kv

    if kv.run_role():
        return None
    store = kv.create("dist_sync")
    n = key_mb * (1 << 20) // 4
    vals = [torch.zeros(n, device="cuda") for _ in range(keys)]
    for k, v in enumerate(vals):
        store.init(k, v)
    store.set_optimizer(kv.create_optimizer("sgd", learning_rate=0.5, rescale_grad=0.5))
    if compress:
        store.set_gradient_compression({"type": "2bit", "threshold": 0.5})
    grads = [0.35 * torch.randn(n, device="cuda") for _ in range(keys)]
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(keys):
            store.push(k, grads[k])
        for k in range(keys):
            store.pull(k, out=vals[k])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res = (store.rank, times, list(store.plane_ops), list(store.compressed_ops))
    store.close()
    return res


def sync_round(steps: int = 6, keys: int = 8, key_mb: int = 8) -> None:
    ctx = mp.get_context("spawn")
    for compress in (False, True):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        args = [(role, i, port, steps, keys, key_mb, compress)
                for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
        with ctx.Pool(len(args)) as pool:
            outs = [r.get(170) for r in [pool.apply_async(round_rank, a) for a in args]]
        for rank, times, plane_ops, compressed_ops in sorted(o for o in outs if o is not None):
            steady = statistics.median(times[1:])
            print(f"dist_sync round of {keys} x {key_mb} MB push + pull, compression {'2bit' if compress else 'none'}: "
                  f"worker {rank} {steady * 1e3:.2f} ms; all rounds {[round(t * 1e3, 2) for t in times]}; "
                  f"plane_ops {plane_ops} compressed_ops {compressed_ops}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-round", action="store_true", help="skip the multi-process dist_sync round")
    a = ap.parse_args()
    if not a.no_round:  # first: the processes of the round start before this one has touched the GPU
        sync_round()
    kernels(a.launches, a.rounds)


if __name__ == "__main__":
    main()
