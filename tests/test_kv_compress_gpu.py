"""The kvstore's 2-bit gradient compression on the GPU: ``tony_kv_quant2`` / ``tony_kv_dequant2``
(csrc/ps_plane.hip) bit for bit against the numpy reference (tests/kv_compress_ref.py) with guarded
destinations, and the dist_sync / dist_async / dist_device_sync stores with compression on, their values
against the same reference run through the server's sgd."""
import ctypes
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_compress_ref as ref
import kv_compress_workers as W
from exact_helpers import SENT, Slab, assert_equal
from gpu_ranks import placement

pytestmark = pytest.mark.gpu

WORD_FILL = 0x5A5A5A5A  # the integer around the destination words
SIZES = [1, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4099, 262149, 1000003]


def _lib_and_stream():
    from tony_amd.ops import _lib

    dev = torch.device("cuda", 0)
    return _lib, _lib.lib(), dev, _lib.stream_ptr(dev)


def _blocks(n):
    return min(1024, -(-n // 4096))  # one workgroup per 4096 elements, capped


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("n", SIZES)
def test_quant2_bit_exact_in_guarded_surroundings(n, thr):
    _lib, L, dev, stream = _lib_and_stream()
    nw = ref.n_words(n)
    assert L.tony_kv_quant_blocks(n) == _blocks(n)
    # the words at a 4-B (not 16-B) aligned offset of an integer-filled allocation, the residual a slice of a
    # NaN-filled one, the gradient with NaN behind its last element
    words = Slab(1, nw, 1, torch.int32, WORD_FILL, dev, vector_rows=False)
    res = Slab(1, n, 4, torch.float32, float("nan"), dev, vector_rows=False)
    grad = Slab(1, n, 4, torch.float32, float("nan"), dev, vector_rows=False)
    assert res.ptr() % 16 == 0 and grad.ptr() % 16 == 0 and words.ptr() % 16 == 4
    rng = np.random.default_rng(n)
    r_ref = (np.float32(0.4 * thr) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    r_ref[:15] = 0  # the first copy of the special values meets a zero residual (the denormals stay denormal)
    res.view[0].copy_(_f32(r_ref, dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    counted = 0
    for push in range(3):
        g = ref.gradient(n, thr, seed=7 * n + push)
        grad.view[0].copy_(_f32(g, dev))
        grad_before = grad.alloc.clone()
        res_before = res.alloc.clone()
        words.view.fill_(WORD_FILL)
        fl = flag.data_ptr() if push else None  # the first launch without a flag (the gloo path's)
        _lib.check(L.tony_kv_quant2(words.ptr(), grad.ptr(), res.ptr(), n, thr, fl, stream), "tony_kv_quant2")
        words_ref, r_ref = ref.quantise(g, r_ref, thr)
        what = f"n {n} thr {thr} push {push}"
        assert_equal(words.view[0].cpu(), torch.from_numpy(words_ref.view(np.int32)), f"{what}: words")
        assert_equal(res.view[0].cpu().view(torch.int32), torch.from_numpy(r_ref.view(np.int32)),
                     f"{what}: residual bits")
        words.assert_surroundings_intact(f"{what}: words")
        # everything around the residual keeps its bits (NaN: compared as integers), the gradient is unchanged
        after = res.alloc.clone()
        res._inner(after).copy_(res._inner(res_before))
        assert torch.equal(after.view(torch.int32), res_before.view(torch.int32)), f"{what}: bytes around the residual"
        assert torch.equal(grad.alloc.view(torch.int32), grad_before.view(torch.int32)), f"{what}: the gradient"
        counted += _blocks(n) if push else 0
        assert int(flag.item()) == counted, f"{what}: flag adds"


def test_quant2_refuses_misaligned_and_empty_arguments():
    _lib, L, dev, stream = _lib_and_stream()
    g, r = torch.zeros(40, device=dev), torch.zeros(40, device=dev)
    w = torch.zeros(8, dtype=torch.int32, device=dev)
    assert g.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0
    assert L.tony_kv_quant2(w.data_ptr(), g.data_ptr() + 4, r.data_ptr(), 32, 0.5, None, stream) == -1
    assert L.tony_kv_quant2(w.data_ptr(), g.data_ptr(), r.data_ptr() + 8, 32, 0.5, None, stream) == -1
    assert L.tony_kv_quant2(w.data_ptr() + 2, g.data_ptr(), r.data_ptr(), 32, 0.5, None, stream) == -1
    assert L.tony_kv_quant2(w.data_ptr(), g.data_ptr(), r.data_ptr(), 0, 0.5, None, stream) == -1
    assert L.tony_kv_quant2(w.data_ptr(), g.data_ptr(), r.data_ptr(), 32, 0.0, None, stream) == -1
    assert L.tony_kv_quant_blocks(0) == 0 and L.tony_kv_quant_blocks(1 << 40) == 1024
    torch.cuda.synchronize()
    assert not w.any() and not r.any()  # nothing was launched


def _hand_words(nsrc, n, stride, seed):
    """Random u32 words (every code, 3 included) for ``nsrc`` sources ``stride`` words apart; the first word of
    every source holds the four codes in order."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, nsrc * stride, dtype=np.uint64).astype(np.uint32)
    w[::stride] = (w[::stride] & ~np.uint32(0xFF)) | np.uint32(0b11_10_01_00)
    return w


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 17, 1025, 4099, 262149])
def test_dequant2_bit_exact_ordered_sum(n, nsrc, thr):
    _lib, L, dev, stream = _lib_and_stream()
    stride = ref.n_words(n) + 3  # larger than the word count
    w = _hand_words(nsrc, n, stride, seed=n + nsrc)
    words = torch.from_numpy(w.view(np.int32)).to(dev)
    dst = Slab(1, n, 4, torch.float32, SENT, dev, vector_rows=False)
    assert dst.ptr() % 16 == 0
    _lib.check(L.tony_kv_dequant2(dst.ptr(), words.data_ptr(), n, thr, nsrc, stride, None, stream), "tony_kv_dequant2")
    want = ref.merge([w[s * stride:s * stride + ref.n_words(n)] for s in range(nsrc)], n, thr)
    assert_equal(dst.view[0].cpu().view(torch.int32), torch.from_numpy(want.view(np.int32)), f"n {n} nsrc {nsrc}")
    dst.assert_surroundings_intact(f"n {n} nsrc {nsrc}")
    if n >= 4:  # code 3 decodes to 0.0 like code 0
        assert dst.view[0][:4].tolist() == ([0.0, np.float32(thr), -np.float32(thr), 0.0] if nsrc == 1 else
                                            want[:4].tolist())


def test_dequant2_writes_nothing_behind_a_timed_out_wait():
    """With a window whose error word is set (a bounded wait that ran out of its zero budget) the decode is
    skipped, like ``tony_kv_copy``: the destination keeps its bytes."""
    _lib, L, dev, stream = _lib_and_stream()
    torch.cuda.init()
    win = ctypes.c_void_p()
    handle = (ctypes.c_uint8 * L.tony_xgmi_handle_bytes())()
    _lib.check(L.tony_ps_window_alloc(4096, ctypes.byref(win), handle), "tony_ps_window_alloc")
    try:
        n = 1025
        words = torch.from_numpy(_hand_words(1, n, ref.n_words(n), seed=1).view(np.int32)).to(dev)
        dst = Slab(1, n, 4, torch.float32, SENT, dev, vector_rows=False)
        # a clean window: decoded
        _lib.check(L.tony_kv_dequant2(dst.ptr(), words.data_ptr(), n, 0.5, 1, ref.n_words(n), win.value, stream),
                   "tony_kv_dequant2")
        torch.cuda.synchronize()
        assert not (dst.view == SENT).any()
        dst.view.fill_(SENT)
        # the counter in the window's payload is 0 and never reaches 1: the wait gives up at once and records it
        flag = win.value + L.tony_ps_header_bytes()
        _lib.check(L.tony_kv_wait(flag, 1, win.value, 0.0, stream), "tony_kv_wait")
        _lib.check(L.tony_kv_dequant2(dst.ptr(), words.data_ptr(), n, 0.5, 1, ref.n_words(n), win.value, stream),
                   "tony_kv_dequant2")
        torch.cuda.synchronize()
        err = ctypes.c_int(0)
        _lib.check(L.tony_ps_error(win.value, ctypes.byref(err)), "tony_ps_error")  # reads and clears
        assert err.value == 1
        assert bool((dst.alloc == SENT).all()), "the decode ran behind a timed-out wait"
    finally:
        torch.cuda.synchronize()
        L.tony_xgmi_free(win.value)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("kind", ["dist_sync", "dist_async"])
def test_kvstore_plane_pushes_compressed(kind, monkeypatch):
    """A scheduler, one server and two workers on the GPU plane, three steps of keys of 3 and 1000003 fp32
    elements and a bf16 key; at step 1 every worker pushes the big key a second time before pulling it -- that
    push finds its window row possibly unread and must go compressed over gloo.  Every other fp32 push is
    quantised straight into the server's window."""
    monkeypatch.setenv("TONY_KV_WAIT_S", "60")
    port, steps, big_n = _port(), 3, 1000003
    thr = 0.3 if kind == "dist_sync" else 0.5  # (dist_async sums in arrival order: exact at a power of two)
    args = [(role, i, 1, 2, port, kind, steps, "cuda", thr, big_n, 1)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(110) for r in [pool.apply_async(W.kv_gc_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    want = W.predict(steps, 2, thr, [("a", 3), ("big", big_n)], extra_step=1)
    for o in workers:
        # 2 fp32 keys x 3 steps on the plane, the one re-push over gloo; the bf16 pushes ride the plane uncompressed
        assert o["compressed_ops"] == [2 * steps, 1], o["compressed_ops"]
        assert o["plane_ops"] == [3 * steps, 3 * steps], o["plane_ops"]
        assert o["late"] == "RuntimeError", o["late"]
    if kind == "dist_sync":
        for o in workers:
            for s in range(steps):
                for key in ("a", "big"):
                    np.testing.assert_allclose(o["seen"][s][key], want[key][s], rtol=1e-6, atol=0,
                                               err_msg=f"worker {o['rank']} step {s} key {key}")
                assert o["seen"][s]["h"] == [-0.75 * (s + 1)] * W.HALF_N
    else:
        for key in ("a", "big"):
            assert any(np.array_equal(o["seen"][-1][key], want[key][-1]) for o in workers), key
    assert np.abs(want["big"][-1]).max() > 0


def test_device_sync_all_gathers_the_words():
    """dist_device_sync with compression on two ranks: both hold the value the reference predicts (the decoded
    pushes summed in rank order, through sgd), bit-identical to each other."""
    world, thr, n, steps = 2, 0.3, 4099, 3
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=W.device_sync_rank, args=(r, world, port, q, thr, n, steps)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=110) for _ in range(world))
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert "error" not in out[r], f"[{placement(world)}] rank {r}: {out[r].get('error')}"
    want = W.predict(steps, world, thr, [("w", n)])["w"]
    for s in range(steps):
        assert np.array_equal(out[0]["seen"][s].view(np.uint32), out[1]["seen"][s].view(np.uint32)), f"step {s}"
        np.testing.assert_allclose(out[0]["seen"][s], want[s], rtol=1e-6, atol=0, err_msg=f"step {s}")
    assert np.abs(want[-1]).max() > 0
