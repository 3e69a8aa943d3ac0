"""Row-sparse keys of the kvstore on the CPU (tony_amd/parallel/kvstore.py): ``RowSparse`` and ``from_rows``, the
``local`` store against the numpy contract (tests/kv_sparse_ref.py), the sparse / dense key rules, and the dist
stores over gloo in spawned CPU processes."""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_sparse_ref as ref
import kv_sparse_workers as W
import tony_amd.kv as kv

R, D = 12, 4


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(ref.bits(got), ref.bits(want)), f"{what}: {int((ref.bits(got) != ref.bits(want)).sum())} differ"


@pytest.mark.parametrize("ids", [[3, 1], [1, 1], [-1, 2], [0, R]])
def test_rowsparse_refuses_unsorted_duplicate_and_out_of_range_ids(ids):
    with pytest.raises(ValueError):
        kv.RowSparse(torch.tensor(ids), torch.zeros(len(ids), D), (R, D))


def test_rowsparse_refuses_mismatched_data_and_takes_no_rows():
    with pytest.raises(ValueError):
        kv.RowSparse(torch.tensor([1, 2]), torch.zeros(3, D), (R, D))
    with pytest.raises(ValueError):
        kv.RowSparse(torch.tensor([1, 2], dtype=torch.int32), torch.zeros(2, D), (R, D))
    empty = kv.RowSparse(torch.zeros(0, dtype=torch.int64), torch.zeros(0, D), (R, D))
    assert empty.nnz == 0 and not empty.to_dense().any() and empty.to_dense().shape == (R, D)
    v = kv.RowSparse(torch.tensor([0, R - 1]), torch.ones(2, D), (R, D))
    assert v.to_dense().sum() == 2 * D and v.to_dense()[R - 1, 0] == 1


def test_from_rows_equals_the_reference_bit_for_bit():
    rng = np.random.default_rng(0)
    ids = np.asarray([5, 2, 5, 11, 2, 5, 0, 5], np.int64)
    rows = rng.standard_normal((ids.size, D)).astype(np.float32)
    rows[0, 0], rows[2, 0], rows[5, 0], rows[7, 0] = 1e8, 1.0, -1e8, 1.0  # the order of the adds shows: 1, not 0 or 2
    v = kv.RowSparse.from_rows(_t(ids).view(2, 4), _t(rows), (R, D))
    want_ids, want = ref.from_rows(ids, rows)
    assert v.indices.tolist() == want_ids.tolist() == [0, 2, 5, 11]
    _same_bits(v.data.numpy(), want, "from_rows")
    assert v.data[2, 0] == 1.0
    none = kv.RowSparse.from_rows(torch.zeros(0, dtype=torch.int64), torch.zeros(0, D), (R, D))
    assert none.nnz == 0
    with pytest.raises(ValueError):
        kv.RowSparse.from_rows(torch.tensor([0, R]), torch.zeros(2, D), (R, D))


def _local_steps():
    """Three pushes to a local store: a list whose members overlap, one value, a list with an empty member."""
    return [W.pushes_of(0, 0, R, D, False), W.pushes_of(1, 1, R, D, False),
            W.pushes_of(0, 2, R, D, False) + W.pushes_of(1, 2, R, D, False)]


def _local_store(opt):
    store = kv.create("local")
    w0 = W.table0(R, D, False)
    store.init("emb", kv.RowSparse(torch.arange(R), _t(w0.copy()), (R, D)))
    if opt is not None:
        store.set_optimizer(opt)
    return store, w0


def test_local_store_without_an_optimizer_takes_the_ordered_merge():
    store, _ = _local_store(None)
    for pushes in _local_steps():
        store.push("emb", [W._rsp(kv, p, (R, D), "cpu") for p in pushes])
        ids, rows = ref.merge(pushes)
        got = torch.empty(R, D)
        store.pull("emb", out=got, ignore_sparse=False)
        _same_bits(got.numpy(), ref.assign((R, D), ids, rows), "value after a push")  # rows not pushed are zero


def test_merge_order_is_the_list_order():
    a = (np.asarray([1, 4], np.int64), np.asarray([[1e8] * D, [1.0] * D], np.float32))
    b = (np.asarray([1], np.int64), np.asarray([[1.0] * D], np.float32))
    c = (np.asarray([1, 7], np.int64), np.asarray([[-1e8] * D, [2.0] * D], np.float32))
    for order, row1 in (([a, b, c], 0.0), ([a, c, b], 1.0)):
        store, _ = _local_store(None)
        store.push("emb", [W._rsp(kv, p, (R, D), "cpu") for p in order])
        got = torch.empty(R, D)
        store.pull("emb", out=got, ignore_sparse=False)
        ids, rows = ref.merge(order)
        _same_bits(got.numpy(), ref.assign((R, D), ids, rows), "ordered merge")
        assert got[1].tolist() == [row1] * D and got[7].tolist() == [2.0] * D


SGD_CASES = [dict(learning_rate=0.1), dict(learning_rate=0.1, momentum=0.9),
             dict(learning_rate=0.1, wd=0.01, rescale_grad=0.5, clip_gradient=2.0),
             dict(learning_rate=0.1, momentum=0.9, wd=0.01, rescale_grad=0.5, clip_gradient=2.0)]


@pytest.mark.parametrize("cfg", SGD_CASES, ids=["plain", "momentum", "wd-clip", "momentum-wd-clip"])
def test_local_store_lazy_sgd_follows_the_contract(cfg):
    """Each of three steps from the store's own state: untouched rows of weight and momentum keep their bits,
    touched rows are within the counted-rounding bound of the step (kv_sparse_ref.py)."""
    opt = kv.create_optimizer("sgd", **cfg)
    store, w = _local_store(opt)
    mom = np.zeros_like(w) if cfg.get("momentum") else None
    for step, pushes in enumerate(_local_steps()):
        store.push("emb", [W._rsp(kv, p, (R, D), "cpu") for p in pushes])
        ids, rows = ref.merge(pushes)
        want_w, want_m, bw, bm = ref.sgd(w, mom, ids, rows, lr=cfg["learning_rate"], momentum=cfg.get("momentum", 0.0),
                                         wd=cfg.get("wd", 0.0), rescale=cfg.get("rescale_grad", 1.0),
                                         clip=cfg.get("clip_gradient"))
        got = torch.empty(R, D)
        store.pull("emb", out=got, ignore_sparse=False)
        got = got.numpy()
        rest = np.setdiff1d(np.arange(R), ids)
        assert rest.size and ids.size
        _same_bits(got[rest], w[rest], f"step {step}: untouched rows of the weight")
        ref.within(got[ids], want_w[ids], bw, f"step {step}: touched rows of the weight")
        assert not np.array_equal(got[ids], w[ids])
        if mom is not None:
            got_m = opt.state[store._key("emb")]["mom"].numpy()
            assert got_m.shape == (R, D)
            _same_bits(got_m[rest], mom[rest], f"step {step}: untouched rows of the momentum")
            ref.within(got_m[ids], want_m[ids], bm, f"step {step}: touched rows of the momentum")
            mom = got_m.copy()
        w = got.copy()  # the next step starts from the store's own state


def test_local_store_lazy_adam_follows_the_contract():
    cfg = dict(learning_rate=0.05, wd=0.01, rescale_grad=0.5)
    opt = kv.create_optimizer("adam", **cfg)
    store, w = _local_store(opt)
    m, v = np.zeros_like(w), np.zeros_like(w)
    for step, pushes in enumerate(_local_steps()):
        store.push("emb", [W._rsp(kv, p, (R, D), "cpu") for p in pushes])
        ids, rows = ref.merge(pushes)
        want = ref.adam(w, m, v, step + 1, ids, rows, lr=cfg["learning_rate"], wd=cfg["wd"], rescale=cfg["rescale_grad"])
        got = torch.empty(R, D)
        store.pull("emb", out=got, ignore_sparse=False)
        st = opt.state[store._key("emb")]
        assert st["t"] == step + 1  # t counts updates of the key
        rest = np.setdiff1d(np.arange(R), ids)
        for name, g, before, wanted, bound in (("weight", got.numpy(), w, want[0], want[3]),
                                               ("m", st["m"].numpy(), m, want[1], want[4]),
                                               ("v", st["v"].numpy(), v, want[2], want[5])):
            _same_bits(g[rest], before[rest], f"step {step}: untouched rows of {name}")
            ref.within(g[ids], wanted[ids], bound, f"step {step}: touched rows of {name}")
        w, m, v = got.numpy().copy(), st["m"].numpy().copy(), st["v"].numpy().copy()


def test_pull_skips_sparse_keys_unless_asked_and_kinds_do_not_mix():
    store, w0 = _local_store(None)
    store.init("d", torch.arange(3.0))
    out = torch.full((R, D), 7.0)
    store.pull("emb", out=out)  # ignore_sparse=True
    assert bool((out == 7.0).all())
    store.pull("emb", out=out, ignore_sparse=False)
    _same_bits(out.numpy(), w0, "dense pull of a sparse key")
    for flag in (True, False):
        d = torch.zeros(3)
        store.pull("d", out=d, ignore_sparse=flag)
        assert d.tolist() == [0.0, 1.0, 2.0]
    one = kv.RowSparse(torch.tensor([1]), torch.ones(1, D), (R, D))
    with pytest.raises(TypeError):
        store.push("d", one)
    with pytest.raises(TypeError):
        store.push("emb", torch.zeros(R, D))
    with pytest.raises(TypeError):
        store.push("emb", [one, torch.zeros(R, D)])
    store.pull("emb", out=out, ignore_sparse=False)
    _same_bits(out.numpy(), w0, "a refused push changes nothing")


def test_row_sparse_pull_returns_the_sorted_unique_rows():
    store, w0 = _local_store(None)
    store.init("e2", kv.RowSparse(torch.tensor([2]), torch.ones(1, D), (R, D)))
    out = kv.RowSparse(torch.zeros(0, dtype=torch.int64), torch.zeros(0, D), (R, D))
    store.row_sparse_pull("emb", out=out, row_ids=torch.tensor([[R - 1, 3], [0, 3]]))
    assert out.indices.tolist() == [0, 3, R - 1]
    _same_bits(out.data.numpy(), w0[[0, 3, R - 1]], "pulled rows")
    o1, o2 = (kv.RowSparse(torch.zeros(0, dtype=torch.int64), torch.zeros(0, D), (R, D)) for _ in range(2))
    store.row_sparse_pull(["emb", "e2"], out=[o1, o2], row_ids=[torch.tensor([5]), torch.tensor([2, 1])])
    _same_bits(o1.data.numpy(), w0[[5]], "first key")
    assert o2.indices.tolist() == [1, 2] and o2.data.tolist() == [[0.0] * D, [1.0] * D]
    store.row_sparse_pull("emb", out=out, row_ids=torch.zeros(0, dtype=torch.int64))
    assert out.nnz == 0 and out.data.shape == (0, D)
    for bad in ([0, R], [-1]):
        with pytest.raises(ValueError):
            store.row_sparse_pull("emb", out=out, row_ids=torch.tensor(bad))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(kind, opt, steps, exact):
    port = _port()
    args = [(role, i, 1, W.NW, port, kind, "cpu", opt, steps, exact, R, D)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(150) for r in [pool.apply_async(W.kv_rsp_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    return workers


# power-of-two hyper-parameters on small integers: every operation of the update is exact, fused or not, so the sum
# of the steps' bounds covers the final value of a run whose intermediate states the test does not see
EXACT_SGD = {"dist_sync": dict(learning_rate=0.5, momentum=0.5, wd=0.25, rescale_grad=0.5, clip_gradient=4.0),
             "dist_async": dict(learning_rate=0.5, rescale_grad=0.5)}


@pytest.mark.parametrize("with_opt", [False, True], ids=["assign", "sgd"])
@pytest.mark.parametrize("kind", ["dist_sync", "dist_async"])
def test_dist_stores_over_gloo_follow_the_reference(kind, with_opt):
    """1 scheduler + 1 server + 2 workers over gloo, four steps: overlapping, disjoint, one worker's empty and a
    whole-table push.  With no optimizer the value is the reference's ordered merge bit for bit; with SGD it is
    within the reference's bound; every row_sparse_pull after a push sees the finished round."""
    opt = EXACT_SGD[kind] if with_opt else None
    steps = 4
    workers = _run(kind, opt, steps, exact=with_opt)
    seen, final, tol = W.predict(kind, opt, steps, with_opt, R, D)
    for o in workers:
        r = o["rank"]
        assert o["errors"] == {"dense_to_sparse": "TypeError", "sparse_to_dense": "TypeError",
                               "out_of_range": "ValueError"}, o["errors"]
        # every push and pull over gloo, but worker 1's push of no rows at step 2 (the header only)
        assert o["sparse_ops"] == [0, steps - (r == 1), 0, steps], o["sparse_ops"]
        for s in range(steps):
            ids = np.unique(W.pull_ids(r, s, R))
            assert o["seen"][s][0].tolist() == ids.tolist()
            if with_opt:
                ref.within(o["seen"][s][1], seen[s][r][ids], tol[ids], f"worker {r} step {s}")
            else:
                _same_bits(o["seen"][s][1], seen[s][r][ids], f"worker {r} step {s}")
        if with_opt:
            ref.within(o["final"], final, tol, f"worker {r}: final value")
        else:
            _same_bits(o["final"], final, f"worker {r}: final value")
        assert bool((o["skipped"] == 7.0).all()) and o["dense"] == [0.0, 0.0, 0.0]
    assert np.abs(final).max() > 0 and not np.array_equal(final, W.table0(R, D, with_opt))


@pytest.mark.parametrize("with_opt", [False, True], ids=["assign", "sgd"])
def test_device_sync_over_gloo_is_identical_on_both_ranks(with_opt):
    opt = EXACT_SGD["dist_sync"] if with_opt else None
    steps, port = 4, _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=W.device_sync_rank, args=(r, W.NW, port, q, "cpu", opt, steps, with_opt, R, D))
             for r in range(W.NW)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=150) for _ in range(W.NW))
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    for r in range(W.NW):
        assert "error" not in out[r], f"rank {r}: {out[r].get('error')}"
    seen, final, tol = W.predict("dist_device_sync", opt, steps, with_opt, R, D)
    _same_bits(out[0]["final"], out[1]["final"], "the two ranks")
    for r in range(W.NW):
        for s in range(steps):
            ids = np.unique(W.pull_ids(r, s, R))
            assert out[r]["seen"][s][0].tolist() == ids.tolist()
            ref.within(out[r]["seen"][s][1], seen[s][r][ids], tol[ids], f"rank {r} step {s}")
        if with_opt:
            ref.within(out[r]["final"], final, tol, f"rank {r}: final value")
        else:
            _same_bits(out[r]["final"], final, f"rank {r}: final value")
