"""Row-sparse keys of the kvstore on the GPU: ``tony_kv_rsp_gather`` / ``tony_kv_rsp_merge`` / ``tony_kv_rsp_sgd``
(csrc/ps_plane.hip) bit for bit against the numpy contract (tests/kv_sparse_ref.py) with guarded destinations, and
the local, dist_sync / dist_async (GPU payload plane) and dist_device_sync stores against the same reference."""
import ctypes
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_sparse_ref as ref
import kv_sparse_workers as W
from exact_helpers import SENT, Slab, assert_equal
from gpu_ranks import placement

pytestmark = pytest.mark.gpu

R = 64
ROW_ELEMS = [4, 36, 1028]  # 16 B, 144 B and a row longer than the 1 KiB one pass of a wave covers
I64 = ctypes.c_int64


def _lib_and_stream():
    from tony_amd.ops import _lib

    dev = torch.device("cuda", 0)
    return _lib, _lib.lib(), dev, _lib.stream_ptr(dev)


def _flat(n, fill, dev, re):
    """``n`` fp32 elements 16 B into an allocation filled with ``fill`` (guards sized by the row)."""
    s = Slab(1, n, 4, torch.float32, fill, dev, guard_ld=re, vector_rows=False)
    assert s.ptr() % 16 == 0
    return s


def _blocks(nnz, re):
    return min(1024, -(-(nnz * -(-(re // 4) // 64)) // 4))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    """Bit equality of the fp32 tensor ``got`` with the numpy ``want``; where the contract gives a NaN any NaN will
    do (its sign and payload differ between instruction sets and are no part of the contract)."""
    got = got.detach().cpu().contiguous()
    want = torch.from_numpy(np.ascontiguousarray(want, np.float32)).view(got.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs are not where the contract has them"
    assert_equal(_bits(torch.where(nan, torch.zeros_like(got), got)),
                 _bits(torch.where(nan, torch.zeros_like(want), want)), what)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _table(re, dev, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((R, re)).astype(np.float32)
    slab = _flat(R * re, float("nan"), dev, re)
    slab.view[0].copy_(_dev(t.reshape(-1), dev))
    return t, slab


def _id_sets(nnz):
    if nnz == 1:
        return [[0], [R - 1]]
    if nnz == 3:
        return [[0, 31, R - 1]]
    return [list(range(R))]


@pytest.mark.parametrize("nnz", [1, 3, 64])
@pytest.mark.parametrize("re", ROW_ELEMS)
def test_gather_bit_exact_in_guarded_surroundings(re, nnz):
    _lib, L, dev, stream = _lib_and_stream()
    t, table = _table(re, dev, seed=re + nnz)
    assert L.tony_kv_rsp_gather_blocks(nnz, 4 * re) == _blocks(nnz, re)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    counted = 0
    for k, ids in enumerate(_id_sets(nnz) * 2):
        dst = _flat(nnz * re, SENT, dev, re)
        d_ids = _dev(np.asarray(ids, np.int64), dev)
        fl = flag.data_ptr() if k % 2 else None
        _lib.check(L.tony_kv_rsp_gather(dst.ptr(), table.ptr(), d_ids.data_ptr(), nnz, 4 * re, R, fl, None, stream),
                   "tony_kv_rsp_gather")
        what = f"row {re} nnz {nnz} ids {ids[:3]}"
        assert_equal(_bits(dst.view[0]).cpu(), _bits(_dev(t[ids].reshape(-1), "cpu")), what)
        dst.assert_surroundings_intact(what)
        counted += _blocks(nnz, re) if k % 2 else 0
        assert int(flag.item()) == counted, f"{what}: flag adds"


def _sources(layout, nsrc, re, seed):
    rng = np.random.default_rng(seed)
    if nsrc == 1:
        sets = {"identical": [[0, 5, R - 1]], "disjoint": [[0, 1, 2, R - 1]], "one-empty": [[0]]}[layout]
    else:
        sets = {"identical": [[0, 5, R - 1]] * 3, "disjoint": [[0, 1], [5], [R - 2, R - 1]],
                "one-empty": [[0, 5, R - 1], [], [5, 7]]}[layout]
    srcs = []
    for s, ids in enumerate(sets):
        rows = rng.standard_normal((len(ids), re)).astype(np.float32)
        if len(ids):
            rows[:, 0] = [1e8, 1.0, -1e8][s]  # fp32 addition order matters: (1e8 + 1) - 1e8 = 0, (1e8 - 1e8) + 1 = 1
        srcs.append((np.asarray(ids, np.int64), rows))
    return srcs


@pytest.mark.parametrize("layout", ["identical", "disjoint", "one-empty"])
@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("re", ROW_ELEMS)
def test_merge_bit_exact_ordered_sum(re, nsrc, layout):
    _lib, L, dev, stream = _lib_and_stream()
    srcs = _sources(layout, nsrc, re, seed=re + nsrc)
    union, want = ref.merge(srcs)
    if nsrc == 3 and layout == "identical":
        assert want[0, 0] == 0.0  # the ordered sum, not the exact one
    d_union = _dev(union, dev)
    d_ids = [_dev(i, dev) for i, _ in srcs]
    d_rows = [_flat(max(1, r.size), float("nan"), dev, re) for _, r in srcs]
    for slab, (_, r) in zip(d_rows, srcs):
        if r.size:
            slab.view[0].copy_(_dev(r.reshape(-1), dev))
    dst = _flat(union.size * re, SENT, dev, re)
    arr = I64 * nsrc
    rc = L.tony_kv_rsp_merge(dst.ptr(), d_union.data_ptr(), union.size,
                             arr(*[i.data_ptr() if i.numel() else 0 for i in d_ids]),
                             arr(*[s.ptr() if r.size else 0 for s, (_, r) in zip(d_rows, srcs)]),
                             arr(*[i.size for i, _ in srcs]), nsrc, re, stream)
    _lib.check(rc, "tony_kv_rsp_merge")
    what = f"row {re} nsrc {nsrc} {layout}"
    assert_equal(_bits(dst.view[0]).cpu(), _bits(_dev(want.reshape(-1), "cpu")), what)
    dst.assert_surroundings_intact(what)


SGD_CASES = [dict(lr=0.1), dict(lr=0.1, momentum=0.9), dict(lr=0.1, wd=0.01, rescale=0.3, clip=2.0),
             dict(lr=0.1, momentum=0.9, wd=0.01, rescale=0.3, clip=2.0)]


@pytest.mark.parametrize("hp", SGD_CASES, ids=["plain", "momentum", "wd-clip", "momentum-wd-clip"])
@pytest.mark.parametrize("re", ROW_ELEMS)
def test_sgd_apply_bit_exact_and_lazy(re, hp):
    _lib, L, dev, stream = _lib_and_stream()
    w = np.random.default_rng(re + 1).standard_normal((R, re)).astype(np.float32)
    weight = _flat(R * re, SENT, dev, re)
    weight.view[0].copy_(_dev(w.reshape(-1), dev))
    momentum = hp.get("momentum", 0.0)
    m = np.zeros_like(w) if momentum else None
    mom = _flat(R * re, SENT, dev, re) if momentum else None
    if mom is not None:
        mom.view[0].zero_()
    rng = np.random.default_rng(re)
    for step, ids in enumerate([[0, 5, 31, R - 1], [5, 6], [0, 7, R - 1]]):
        ids = np.asarray(ids, np.int64)
        g = (rng.standard_normal((ids.size, re)) * 3).astype(np.float32)
        g[0, 1], g[-1, 2], g[0, 3] = np.nan, 100.0, -100.0  # a NaN, and elements the clip (if any) cuts on both sides
        d_ids, d_g = _dev(ids, dev), _dev(g, dev)
        rc = L.tony_kv_rsp_sgd(weight.ptr(), None if mom is None else mom.ptr(), d_ids.data_ptr(), d_g.data_ptr(),
                               ids.size, re, R, hp["lr"], momentum, hp.get("wd", 0.0), hp.get("rescale", 1.0),
                               int("clip" in hp), hp.get("clip", 0.0), stream)
        _lib.check(rc, "tony_kv_rsp_sgd")
        before_w, before_m = w, m
        w, m, _, _ = ref.sgd(w, m, ids, g, **hp)
        what = f"row {re} {hp} step {step}"
        rest = np.setdiff1d(np.arange(R), ids)
        assert np.isnan(w[ids[0], 1]) and np.array_equal(ref.bits(w[rest]), ref.bits(before_w[rest]))
        _assert_bits(weight.view[0], w.reshape(-1), f"{what}: weight")  # (every untouched row among them)
        weight.assert_surroundings_intact(f"{what}: weight")
        if mom is not None:
            _assert_bits(mom.view[0], m.reshape(-1), f"{what}: momentum")
            mom.assert_surroundings_intact(f"{what}: momentum")
            assert np.array_equal(ref.bits(m[rest]), ref.bits(before_m[rest]))


def test_launchers_refuse_null_misaligned_and_odd_rows():
    _lib, L, dev, stream = _lib_and_stream()
    table = torch.ones(R * 8, device=dev)
    dst = torch.zeros(4 * 8, device=dev)
    mom = torch.zeros(R * 8, device=dev)
    ids = torch.tensor([0, 1, 2, 3], device=dev)
    t, d, i, m = table.data_ptr(), dst.data_ptr(), ids.data_ptr(), mom.data_ptr()
    assert t % 16 == 0 and d % 16 == 0 and i % 16 == 0
    for args in ((None, t, i, 4, 32, R), (d, None, i, 4, 32, R), (d, t, None, 4, 32, R), (d + 4, t, i, 4, 32, R),
                 (d, t + 8, i, 4, 32, R), (d, t, i + 4, 4, 32, R), (d, t, i, 4, 24, R), (d, t, i, 4, 0, R),
                 (d, t, i, -1, 32, R), (d, t, i, 4, 32, 0)):
        assert L.tony_kv_rsp_gather(*args, None, None, stream) == -1, args
    assert L.tony_kv_rsp_gather(d, t, i, 4, 32, R, d + 2, None, stream) == -1  # a misaligned flag
    assert L.tony_kv_rsp_gather(d, t, i, 0, 32, R, None, None, stream) == 0  # no rows: nothing to launch
    assert L.tony_kv_rsp_gather_blocks(0, 32) == 0 and L.tony_kv_rsp_gather_blocks(4, 24) == 0
    assert L.tony_kv_rsp_gather_blocks(1 << 40, 32) == 1024
    one = I64 * 1
    for args in ((None, i, 4, one(i), one(t), one(4), 1, 8), (d, None, 4, one(i), one(t), one(4), 1, 8),
                 (d + 4, i, 4, one(i), one(t), one(4), 1, 8), (d, i + 4, 4, one(i), one(t), one(4), 1, 8),
                 (d, i, 4, one(0), one(t), one(4), 1, 8), (d, i, 4, one(i), one(0), one(4), 1, 8),
                 (d, i, 4, one(i), one(t + 4), one(4), 1, 8), (d, i, 4, one(i + 2), one(t), one(4), 1, 8),
                 (d, i, 4, one(i), one(t), one(-1), 1, 8), (d, i, 4, one(i), one(t), one(4), 0, 8),
                 (d, i, 4, one(i), one(t), one(4), 65, 8), (d, i, 4, one(i), one(t), one(4), 1, 6)):
        assert L.tony_kv_rsp_merge(*args, stream) == -1, args
    hp = (0.1, 0.0, 0.0, 1.0, 0, 0.0)
    for args in ((None, None, i, d, 4, 8, R), (t, None, None, d, 4, 8, R), (t, None, i, None, 4, 8, R),
                 (t + 4, None, i, d, 4, 8, R), (t, None, i, d + 8, 4, 8, R), (t, None, i + 4, d, 4, 8, R),
                 (t, None, i, d, 4, 6, R), (t, None, i, d, 4, 8, 0), (t, m, i, d, 4, 8, R)):  # a momentum buffer at momentum 0
        assert L.tony_kv_rsp_sgd(*args, *hp, stream) == -1, args
    assert L.tony_kv_rsp_sgd(t, None, i, d, 4, 8, R, 0.1, 0.9, 0.0, 1.0, 0, 0.0, stream) == -1  # momentum, no buffer
    assert L.tony_kv_rsp_sgd(t, m + 4, i, d, 4, 8, R, 0.1, 0.9, 0.0, 1.0, 0, 0.0, stream) == -1
    torch.cuda.synchronize()
    assert bool((table == 1).all()) and not dst.any() and not mom.any()  # nothing was launched


def test_gather_writes_nothing_behind_a_timed_out_wait():
    """With a window whose error word is set (a bounded wait that ran out of its zero budget) the gather is skipped,
    like ``tony_kv_copy``: the destination keeps its bytes."""
    _lib, L, dev, stream = _lib_and_stream()
    torch.cuda.init()
    win = ctypes.c_void_p()
    handle = (ctypes.c_uint8 * L.tony_xgmi_handle_bytes())()
    _lib.check(L.tony_ps_window_alloc(4096, ctypes.byref(win), handle), "tony_ps_window_alloc")
    try:
        re, ids = 36, [0, 31, R - 1]
        _, table = _table(re, dev, seed=3)
        d_ids = _dev(np.asarray(ids, np.int64), dev)
        dst = _flat(len(ids) * re, SENT, dev, re)
        args = (dst.ptr(), table.ptr(), d_ids.data_ptr(), len(ids), 4 * re, R, None, win.value, stream)
        _lib.check(L.tony_kv_rsp_gather(*args), "tony_kv_rsp_gather")  # a clean window: gathered
        torch.cuda.synchronize()
        assert not (dst.view == SENT).any()
        dst.view.fill_(SENT)
        # the counter in the window's payload is 0 and never reaches 1: the wait gives up at once and records it
        flag = win.value + L.tony_ps_header_bytes()
        _lib.check(L.tony_kv_wait(flag, 1, win.value, 0.0, stream), "tony_kv_wait")
        _lib.check(L.tony_kv_rsp_gather(*args), "tony_kv_rsp_gather")
        torch.cuda.synchronize()
        err = ctypes.c_int(0)
        _lib.check(L.tony_ps_error(win.value, ctypes.byref(err)), "tony_ps_error")  # reads and clears
        assert err.value == 1
        assert bool((dst.alloc == SENT).all()), "the gather ran behind a timed-out wait"
    finally:
        torch.cuda.synchronize()
        L.tony_xgmi_free(win.value)


def test_local_store_on_the_gpu_runs_the_kernels_exactly():
    """A local store with its value on the GPU: the merge, the lazy SGD and the row reads go through the kernels and
    equal the numpy contract bit for bit; out-of-range ids never reach a kernel."""
    import tony_amd.kv as kv

    dev = torch.device("cuda", 0)
    Rl, D = 12, 4
    cfg = dict(learning_rate=0.1, momentum=0.9, wd=0.01, rescale_grad=0.3, clip_gradient=2.0)
    opt = kv.create_optimizer("sgd", **cfg)
    store = kv.create("local")
    w = W.table0(Rl, D, False)
    store.init("emb", kv.RowSparse(torch.arange(Rl, device=dev), _dev(w, dev), (Rl, D)))
    store.set_optimizer(opt)
    m = np.zeros_like(w)
    out = kv.RowSparse(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, D, device=dev), (Rl, D))
    for step in range(3):
        pushes = W.pushes_of(0, step, Rl, D, False) + W.pushes_of(1, step, Rl, D, False)
        store.push("emb", [W._rsp(kv, p, (Rl, D), dev) for p in pushes])
        ids, rows = ref.merge(pushes)
        w, m, _, _ = ref.sgd(w, m, ids, rows, lr=0.1, momentum=0.9, wd=0.01, rescale=0.3, clip=2.0)
        store.row_sparse_pull("emb", out=out, row_ids=_dev(W.pull_ids(0, step, Rl), dev))
        want_ids = np.unique(W.pull_ids(0, step, Rl))
        assert out.indices.tolist() == want_ids.tolist()
        assert_equal(_bits(out.data).cpu(), _bits(_dev(w[want_ids], "cpu")), f"step {step}: pulled rows")
        got = torch.empty(Rl, D, device=dev)
        store.pull("emb", out=got, ignore_sparse=False)
        assert_equal(_bits(got).cpu(), _bits(_dev(w, "cpu")), f"step {step}: weight")
        assert_equal(_bits(opt.state[store._key("emb")]["mom"]).cpu(), _bits(_dev(m, "cpu")), f"step {step}: momentum")
    # no rows: a push of empty values changes nothing, a pull of no ids returns none (no kernel sees an empty tensor)
    none = (np.zeros(0, np.int64), np.zeros((0, D), np.float32))
    store.push("emb", [W._rsp(kv, none, (Rl, D), dev), W._rsp(kv, none, (Rl, D), dev)])
    store.pull("emb", out=got, ignore_sparse=False)
    assert_equal(_bits(got).cpu(), _bits(_dev(w, "cpu")), "after an empty push")
    store.row_sparse_pull("emb", out=out, row_ids=torch.zeros(0, dtype=torch.int64, device=dev))
    assert out.nnz == 0 and out.data.shape == (0, D)
    with pytest.raises(ValueError):
        kv.RowSparse(torch.tensor([0, Rl], device=dev), torch.zeros(2, D, device=dev), (Rl, D))
    with pytest.raises(ValueError):
        store.row_sparse_pull("emb", out=out, row_ids=torch.tensor([Rl], device=dev))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


SGD = {"dist_sync": dict(learning_rate=0.1, momentum=0.9, wd=0.01, rescale_grad=0.3, clip_gradient=2.0),
       # dist_async applies the workers' pushes one by one: on small integers with power-of-two hyper-parameters
       "dist_async": dict(learning_rate=0.5, rescale_grad=0.5)}


@pytest.mark.parametrize("kind", ["dist_sync", "dist_async"])
def test_kvstore_plane_moves_sparse_pushes_and_pulls(kind, monkeypatch):
    """A scheduler, one server and two workers on the GPU plane, four steps of a [12, 4] fp32 sparse key under SGD:
    the pushes' rows and ids go into the server's window, the pulled rows come back through the gather kernel, and
    the value equals the reference bit for bit (the kernel SGD is exact).  Worker 1 pushes no rows at step 2 (the
    header only) and every row at step 3: more than its window row holds beside the ids, so that push takes gloo."""
    monkeypatch.setenv("TONY_KV_WAIT_S", "60")
    port, steps, Rl, D = _port(), 4, 12, 4
    exact = kind == "dist_async"
    args = [(role, i, 1, W.NW, port, kind, "cuda", SGD[kind], steps, exact, Rl, D)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(110) for r in [pool.apply_async(W.kv_rsp_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    seen, final, _ = W.predict(kind, SGD[kind], steps, exact, Rl, D)
    for o in workers:
        r = o["rank"]
        assert o["sparse_ops"] == ([4, 0, 4, 0] if r == 0 else [2, 1, 4, 0]), o["sparse_ops"]
        assert o["errors"] == {"dense_to_sparse": "TypeError", "sparse_to_dense": "TypeError",
                               "out_of_range": "ValueError"}, o["errors"]
        for s in range(steps):
            ids = np.unique(W.pull_ids(r, s, Rl))
            assert o["seen"][s][0].tolist() == ids.tolist()
            assert np.array_equal(ref.bits(o["seen"][s][1]), ref.bits(seen[s][r][ids])), f"worker {r} step {s}"
        assert np.array_equal(ref.bits(o["final"]), ref.bits(final)), f"worker {r}: final value"
        assert bool((o["skipped"] == 7.0).all()) and o["dense"] == [0.0, 0.0, 0.0]
    assert not np.array_equal(final, W.table0(Rl, D, exact))


def test_device_sync_merges_in_rank_order_on_the_gpu():
    world, steps, Rl, D = 2, 4, 12, 4
    opt = SGD["dist_sync"]
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=W.device_sync_rank, args=(r, world, port, q, "cuda", opt, steps, False, Rl, D))
             for r in range(world)]
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
    seen, final, _ = W.predict("dist_device_sync", opt, steps, False, Rl, D)
    for r in range(world):
        for s in range(steps):
            ids = np.unique(W.pull_ids(r, s, Rl))
            assert np.array_equal(ref.bits(out[r]["seen"][s][1]), ref.bits(seen[s][r][ids])), f"rank {r} step {s}"
        assert np.array_equal(ref.bits(out[r]["final"]), ref.bits(final)), f"rank {r}: final value"
