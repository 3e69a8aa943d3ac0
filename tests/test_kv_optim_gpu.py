"""The kvstore's fused optimizer kinds on the GPU: ``tony_kv_opt_dense`` / ``tony_kv_opt_rows`` (csrc/kv_optim.hip)
bit for bit against the numpy contract (tests/kv_optim_ref.py) in guarded allocations, the launchers' refusals, and
the local and dist_sync (GPU payload plane) stores against the same reference."""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_optim_ref as ref
import kv_optim_workers as W
import kv_sparse_ref as sref
import kv_sparse_workers as SW
from exact_helpers import SENT, Slab, assert_equal

pytestmark = pytest.mark.gpu

R = 64
ROW_ELEMS = [4, 36, 1028]  # 16 B, 144 B and a row longer than the 1 KiB one pass of a wave covers
# tail only, one chunk, chunks and a tail, and (4 MB) a workgroup's second trip of the grid-stride loop
DENSE_N = [3, 4, 1027, (1 << 20) + 1027]
KIND = {"nag": 0, "adagrad": 1, "rmsprop": 2, "ftrl": 4}

PLAIN = {"nag0": ("nag", dict(learning_rate=0.1)),
         "nag": ("nag", dict(learning_rate=0.1, momentum=0.9)),
         "adagrad": ("adagrad", dict(learning_rate=0.1)),
         "rmsprop": ("rmsprop", dict(learning_rate=0.01)),
         "rmsprop-centered": ("rmsprop", dict(learning_rate=0.01, centered=True, gamma1=0.95, gamma2=0.8)),
         "ftrl": ("ftrl", dict(learning_rate=0.1, lamda1=0.5))}
EXTRA = dict(wd=0.01, rescale_grad=0.3, clip_gradient=2.0)
CASES = {**PLAIN, **{k + "-wd-clip": (n, dict(c, **EXTRA)) for k, (n, c) in PLAIN.items()}}


def _lib_and_stream():
    from tony_amd.ops import _lib

    dev = torch.device("cuda", 0)
    return _lib, _lib.lib(), dev, _lib.stream_ptr(dev)


def _hp(name, cfg):
    """The kind and the hyperparameter arguments of the two entry points."""
    c = dict(ref.DEFAULTS, **cfg)
    eps = c["epsilon"] if c["epsilon"] is not None else (1e-7 if name == "adagrad" else 1e-8)
    clip = c["clip_gradient"]
    return 3 if c["centered"] else KIND[name], (c["learning_rate"], c["wd"], c["rescale_grad"], int(clip is not None),
                                                0.0 if clip is None else clip, c["momentum"], eps, c["gamma1"],
                                                1 - c["gamma1"], c["gamma2"], c["lamda1"], c["beta"])


def _flat(n, fill, dev, re=4):
    """``n`` fp32 elements 16 B into an allocation filled with ``fill``."""
    s = Slab(1, n, 4, torch.float32, fill, dev, guard_ld=re, vector_rows=False)
    assert s.ptr() % 16 == 0
    return s


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    """Bit equality of the fp32 tensor ``got`` with the numpy ``want``; where the contract gives a NaN any NaN will
    do (its sign and payload are no part of the contract)."""
    got = got.detach().cpu().contiguous()
    want = torch.from_numpy(np.ascontiguousarray(want, np.float32)).view(got.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs are not where the contract has them"
    assert_equal(_bits(torch.where(nan, torch.zeros_like(got), got)),
                 _bits(torch.where(nan, torch.zeros_like(want), want)), what)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _slabs(name, cfg, w, dev, re=4):
    """The weight (its values) and one zeroed slab per state of the setting, in SENT-filled allocations, and the
    three state pointers of a launch."""
    weight = _flat(w.size, SENT, dev, re)
    weight.view[0].copy_(_dev(w.reshape(-1), dev))
    states = {}
    for k in ref.state_names(name, dict(ref.DEFAULTS, **cfg)):
        states[k] = _flat(w.size, SENT, dev, re)
        states[k].view[0].zero_()
    ptrs = [s.ptr() for s in states.values()] + [None] * (3 - len(states))
    return weight, states, ptrs


def _check(weight, states, w, st, what):
    _assert_bits(weight.view[0], w.reshape(-1), f"{what}: weight")
    weight.assert_surroundings_intact(f"{what}: weight")
    assert sorted(states) == sorted(st)
    for k, slab in states.items():
        _assert_bits(slab.view[0], st[k].reshape(-1), f"{what}: {k}")
        slab.assert_surroundings_intact(f"{what}: {k}")


def _radicand_positive(name, cfg, st, finite, what):
    """Centered rmsprop takes the root of ``n - g^2 + eps``: positive in the reference wherever no NaN entered."""
    if cfg.get("centered"):
        e = ref.rmsprop_radicand(st["n"], st["g"], dict(ref.DEFAULTS, **cfg)["epsilon"] or 1e-8)
        assert np.all(e[finite] > 0), f"{what}: the reference's radicand is not positive"


@pytest.mark.parametrize("n", DENSE_N)
@pytest.mark.parametrize("case", sorted(CASES))
def test_dense_kernel_bit_exact_in_guarded_surroundings(case, n):
    name, cfg = CASES[case]
    _lib, L, dev, stream = _lib_and_stream()
    kind, hp = _hp(name, cfg)
    rng = np.random.default_rng(n % 1000 + len(case))
    w = rng.standard_normal(n).astype(np.float32)
    weight, states, ptrs = _slabs(name, cfg, w, dev)
    grad = _flat(n, float("nan"), dev)
    st = {}
    for step in range(3):
        g = (rng.standard_normal(n) * 3).astype(np.float32)
        g[0], g[1], g[n - 1] = np.nan, 100.0, -100.0  # a NaN, and elements the clip (if any) cuts on both sides
        grad.view[0].copy_(_dev(g, dev))
        _lib.check(L.tony_kv_opt_dense(kind, weight.ptr(), *ptrs, grad.ptr(), n, *hp, stream), "tony_kv_opt_dense")
        w, st, _ = ref.step(name, w, st, None, g, **cfg)
        what = f"{case} n {n} step {step}"
        _check(weight, states, w, st, what)
        finite = np.ones(n, bool)
        finite[0] = False
        _radicand_positive(name, cfg, st, finite, what)
    assert np.isnan(w[0]) and 1 <= int(np.isnan(w).sum()) <= 3


@pytest.mark.parametrize("re", ROW_ELEMS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_kernel_bit_exact_and_lazy(case, re):
    name, cfg = CASES[case]
    _lib, L, dev, stream = _lib_and_stream()
    kind, hp = _hp(name, cfg)
    rng = np.random.default_rng(re + len(case))
    w = rng.standard_normal((R, re)).astype(np.float32)
    weight, states, ptrs = _slabs(name, cfg, w, dev, re)
    st = {}
    finite = np.ones((R, re), bool)
    for step, ids in enumerate([[0, 5, 31, R - 1], [5, 6], [0, 7, R - 1]]):
        ids = np.asarray(ids, np.int64)
        g = (rng.standard_normal((ids.size, re)) * 3).astype(np.float32)
        g[0, 1], g[-1, 2], g[0, 3] = np.nan, 100.0, -100.0
        finite[ids[0], 1] = False
        d_ids, d_g = _dev(ids, dev), _dev(g, dev)
        rc = L.tony_kv_opt_rows(kind, weight.ptr(), *ptrs, d_ids.data_ptr(), d_g.data_ptr(), ids.size, re, R, *hp,
                                stream)
        _lib.check(rc, "tony_kv_opt_rows")
        before_w, before_s = w, st
        w, st, _ = ref.step(name, w, st, ids, g, **cfg)
        what = f"{case} row {re} step {step}"
        rest = np.setdiff1d(np.arange(R), ids)
        assert np.array_equal(ref.bits(w[rest]), ref.bits(before_w[rest]))
        for k in st:
            was = before_s.get(k, np.zeros_like(w))
            assert np.array_equal(ref.bits(st[k][rest]), ref.bits(was[rest]))
        _check(weight, states, w, st, what)  # (every untouched row of the weight and of each state among them)
        _radicand_positive(name, cfg, st, finite, what)
    assert 1 <= int(np.isnan(w).sum()) <= 3


@pytest.mark.parametrize("case", sorted(k for k in CASES if k.endswith("-wd-clip")))
def test_rows_kernel_past_one_trip_of_the_grid(case):
    """4100 rows of 4 elements, every row pushed: more items than the 1024 workgroups' 4096 waves take in one trip."""
    name, cfg = CASES[case]
    _lib, L, dev, stream = _lib_and_stream()
    kind, hp = _hp(name, cfg)
    Rb, re = 4100, 4
    rng = np.random.default_rng(len(case))
    w = rng.standard_normal((Rb, re)).astype(np.float32)
    weight, states, ptrs = _slabs(name, cfg, w, dev, re)
    ids = np.arange(Rb, dtype=np.int64)
    d_ids = _dev(ids, dev)
    st = {}
    for step in range(2):
        g = (rng.standard_normal((Rb, re)) * 3).astype(np.float32)
        g[0, 1], g[-1, 2], g[4097, 3] = np.nan, 100.0, -100.0
        d_g = _dev(g, dev)
        _lib.check(L.tony_kv_opt_rows(kind, weight.ptr(), *ptrs, d_ids.data_ptr(), d_g.data_ptr(), Rb, re, Rb, *hp,
                                      stream), "tony_kv_opt_rows")
        w, st, _ = ref.step(name, w, st, ids, g, **cfg)
        _check(weight, states, w, st, f"{case} step {step}")
        finite = np.ones((Rb, re), bool)
        finite[0, 1] = False
        _radicand_positive(name, cfg, st, finite, f"{case} step {step}")
    assert int(np.isnan(w).sum()) == 1


def test_rows_kernel_skips_ids_outside_the_table():
    name, cfg = CASES["adagrad-wd-clip"]
    _lib, L, dev, stream = _lib_and_stream()
    kind, hp = _hp(name, cfg)
    w = np.random.default_rng(1).standard_normal((R, 4)).astype(np.float32)
    weight, states, ptrs = _slabs(name, cfg, w, dev)
    ids = np.asarray([-3, 2, R, R + 5], np.int64)
    g = np.ones((4, 4), np.float32)
    d_ids, d_g = _dev(ids, dev), _dev(g, dev)
    _lib.check(L.tony_kv_opt_rows(kind, weight.ptr(), *ptrs, d_ids.data_ptr(), d_g.data_ptr(), 4, 4, R, *hp, stream),
               "tony_kv_opt_rows")
    w, st, _ = ref.step(name, w, {}, ids[1:2], g[1:2], **cfg)
    _check(weight, states, w, st, "ids outside [0, R)")


def test_launchers_refuse_null_misaligned_missing_states_and_odd_rows():
    _lib, L, dev, stream = _lib_and_stream()
    n = R * 8
    w = torch.ones(n, device=dev)
    s = [torch.zeros(n, device=dev) for _ in range(3)]
    g = torch.ones(n, device=dev)
    ids = torch.tensor([0, 1, 2, 3], device=dev)
    W_, G, IDS = w.data_ptr(), g.data_ptr(), ids.data_ptr()
    S0, S1, S2 = (t.data_ptr() for t in s)
    assert all(p % 16 == 0 for p in (W_, G, IDS, S0, S1, S2))
    hp = (0.1, 0.0, 1.0, 0, 0.0, 0.0, 1e-7, 0.9, 0.1, 0.9, 0.01, 1.0)
    mom = (0.1, 0.0, 1.0, 0, 0.0, 0.9, 1e-7, 0.9, 0.1, 0.9, 0.01, 1.0)
    N = None
    dense_bad = [
        (1, N, S0, N, N, G, n), (1, W_, S0, N, N, N, n), (1, W_ + 4, S0, N, N, G, n), (1, W_, S0, N, N, G + 8, n),
        (1, W_, S0 + 4, N, N, G, n),                      # null and misaligned pointers
        (1, W_, N, N, N, G, n), (4, W_, S0, N, N, G, n), (3, W_, S0, S1, N, G, n), (3, W_, S0, N, S2, G, n),
        (2, W_, N, N, N, G, n),                           # a missing state
        (1, W_, S0, S1, N, G, n), (2, W_, S0, N, S2, G, n), (4, W_, S0, S1, S2, G, n),  # a state the kind does not take
        (0, W_, S0, N, N, G, n),                          # a momentum buffer at momentum 0
        (5, W_, S0, N, N, G, n), (-1, W_, S0, N, N, G, n), (1, W_, S0, N, N, G, -1)]
    for args in dense_bad:
        assert L.tony_kv_opt_dense(*args, *hp, stream) == -1, args
    assert L.tony_kv_opt_dense(0, W_, N, N, N, G, n, *mom, stream) == -1  # momentum, no buffer
    assert L.tony_kv_opt_dense(1, W_, S0, N, N, G, 0, *hp, stream) == 0  # no element: nothing to launch
    rows_bad = [
        (1, N, S0, N, N, IDS, G, 4, 8, R), (1, W_, S0, N, N, N, G, 4, 8, R), (1, W_, S0, N, N, IDS, N, 4, 8, R),
        (1, W_ + 4, S0, N, N, IDS, G, 4, 8, R), (1, W_, S0 + 8, N, N, IDS, G, 4, 8, R),
        (1, W_, S0, N, N, IDS + 4, G, 4, 8, R), (1, W_, S0, N, N, IDS, G + 4, 4, 8, R),
        (1, W_, N, N, N, IDS, G, 4, 8, R), (4, W_, S0, N, N, IDS, G, 4, 8, R), (3, W_, S0, S1, N, IDS, G, 4, 8, R),
        (2, W_, S0, S1, N, IDS, G, 4, 8, R), (4, W_, S0, S1, S2, IDS, G, 4, 8, R), (0, W_, S0, N, N, IDS, G, 4, 8, R),
        (1, W_, S0, N, N, IDS, G, 4, 6, R), (1, W_, S0, N, N, IDS, G, 4, 0, R), (1, W_, S0, N, N, IDS, G, 4, 8, 0),
        (1, W_, S0, N, N, IDS, G, -1, 8, R), (7, W_, S0, N, N, IDS, G, 4, 8, R)]
    for args in rows_bad:
        assert L.tony_kv_opt_rows(*args, *hp, stream) == -1, args
    assert L.tony_kv_opt_rows(0, W_, N, N, N, IDS, G, 4, 8, R, *mom, stream) == -1
    assert L.tony_kv_opt_rows(1, W_, S0, N, N, IDS, G, 0, 8, R, *hp, stream) == 0  # no rows: nothing to launch
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and not any(bool(t.any()) for t in s)  # nothing was launched


@pytest.mark.parametrize("case", ["adagrad-wd-clip", "ftrl", "rmsprop-centered", "nag"])
def test_local_store_on_the_gpu_runs_the_kernels_exactly(case):
    """A local store with its values on the GPU, through the public API: a dense key, a sparse key whose rows the
    rows kernel takes and one of 6-element rows (gathered, the dense kernel, scattered) equal the contract bit for
    bit."""
    import tony_amd.kv as kv

    name, cfg = CASES[case]
    dev = torch.device("cuda", 0)
    Rl, N = 12, 1027
    store = kv.create("local")
    tabs = {D: SW.table0(Rl, D, False) for D in (4, 6)}
    dense = W.dense0(N)
    for D, t in tabs.items():
        store.init(f"emb{D}", kv.RowSparse(torch.arange(Rl, device=dev), _dev(t, dev), (Rl, D)))
    store.init("d", _dev(dense, dev))
    opt = kv.create_optimizer(name, **cfg)
    store.set_optimizer(opt)
    ts, ds = {4: {}, 6: {}}, {}
    for step in range(3):
        for D in tabs:
            pushes = SW.pushes_of(0, step, Rl, D, False) + SW.pushes_of(1, step, Rl, D, False)
            store.push(f"emb{D}", [SW._rsp(kv, p, (Rl, D), dev) for p in pushes])
            ids, rows = sref.merge(pushes)
            tabs[D], ts[D], _ = ref.step(name, tabs[D], ts[D], ids, rows, **cfg)
            got = torch.empty(Rl, D, device=dev)
            store.pull(f"emb{D}", out=got, ignore_sparse=False)
            _assert_bits(got, tabs[D], f"{case} step {step}: table of {D}-element rows")
            for k in ts[D]:
                _assert_bits(opt.state[store._key(f"emb{D}")][k], ts[D][k], f"{case} step {step}: {k} of emb{D}")
        g = [W.dense_grad(r, step, N) for r in range(2)]
        store.push("d", [_dev(x, dev) for x in g])
        dense, ds, _ = ref.step(name, dense, ds, None, (g[0] + g[1]).astype(np.float32), **cfg)
        got = torch.empty(N, device=dev)
        store.pull("d", out=got)
        _assert_bits(got, dense, f"{case} step {step}: dense key")
        # the kernels ran, not the bit-identical torch composition: per step one rows launch (emb4) and one dense
        # launch (d) of this optimizer; emb6's dense launch is counted by the gather / update / scatter's own
        assert opt.kernel_ops == [step + 1, step + 1], opt.kernel_ops


@pytest.mark.parametrize("layout", ["bf16", "strided"])
@pytest.mark.parametrize("case", sorted(PLAIN))
def test_torch_composition_on_the_gpu_equals_the_reference(case, layout):
    """Keys the kernels do not take, on the GPU: a bf16 key (computed in fp32, rounded once on the store) and an fp32
    key that is every other element of its allocation run the torch composition, whose ``/`` and ``sqrt`` on the
    device are held to the contract here; no kernel is launched."""
    import tony_amd.kv as kv

    name, cfg = CASES[case + "-wd-clip"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    n = 1027
    w = rng.standard_normal(n).astype(np.float32)
    if layout == "bf16":
        wt = _dev(w, dev).to(torch.bfloat16)
    else:
        wt = torch.full((2 * n,), SENT, device=dev)[::2]
        wt.copy_(_dev(w, dev))
        assert not wt.is_contiguous()
    opt = kv.create_optimizer(name, **cfg)
    st = {}
    for step in range(3):
        g = (rng.standard_normal(n) * 3).astype(np.float32)
        g[0], g[1], g[n - 1] = np.nan, 100.0, -100.0
        gt = _dev(g, dev).to(wt.dtype)
        want, st, _ = ref.step(name, wt.float().cpu().numpy(), st, None, gt.float().cpu().numpy(), **cfg)
        opt.update(0, wt, gt)
        if layout == "bf16":
            want = torch.from_numpy(want).to(torch.bfloat16).float().numpy()  # rounded once on the store
        _assert_bits(wt.float(), want, f"{case} {layout} step {step}: weight")
        for k in st:
            assert opt.state[0][k].dtype == torch.float32
            _assert_bits(opt.state[0][k], st[k], f"{case} {layout} step {step}: {k}")
    assert opt.kernel_ops == [0, 0]
    if layout == "strided":
        assert bool((wt._base[1::2] == SENT).all())  # the elements between the key's keep their bytes


def test_a_missized_gradient_raises_before_any_launch():
    """The kernels read the gradient to the key's length: a gradient of another element count, or rows that do not
    match their ids, is a ``ValueError`` on the host and nothing is written."""
    import tony_amd.kv as kv

    dev = torch.device("cuda", 0)
    opt = kv.create_optimizer("adagrad", learning_rate=0.1)
    w, tab = torch.ones(1024, device=dev), torch.ones(R, 4, device=dev)
    for g in (torch.ones(1020, device=dev), torch.ones(1028, device=dev)):
        with pytest.raises(ValueError):
            opt.update(0, w, g)
    for ids, rows in ((torch.tensor([1, 2], device=dev), torch.ones(1, 4, device=dev)),
                      (torch.tensor([1], device=dev), torch.ones(2, 4, device=dev)),
                      (torch.tensor([1, 2], device=dev), torch.ones(2, 8, device=dev))):
        with pytest.raises(ValueError):
            opt.update_rows(1, tab, ids, rows)
    store = kv.create("local")
    store.init("d", w)
    store.set_optimizer(opt)
    with pytest.raises(ValueError):
        store.push("d", torch.ones(512, device=dev))
    torch.cuda.synchronize()
    assert opt.kernel_ops == [0, 0] and bool((w == 1).all()) and bool((tab == 1).all())
    assert all(not bool(t.any()) for st in opt.state.values() for k, t in st.items() if k != "t")
    opt.update(0, w, torch.ones(1024, device=dev))  # the right size goes through the kernel
    assert opt.kernel_ops == [1, 0] and not bool((w == 1).any())


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_kvstore_plane_applies_adagrad_to_dense_and_sparse_keys(monkeypatch):
    """A scheduler, one server and two workers on the GPU plane, four steps of a dense [1027] key and a [12, 4]
    sparse key under adagrad: the server applies each merged push in one launch on its stream, and every pull equals
    the reference of the ordered merge followed by the update, bit for bit."""
    monkeypatch.setenv("TONY_KV_WAIT_S", "60")
    name, cfg = CASES["adagrad-wd-clip"]
    port, steps, Rl, D, N = _port(), 4, 12, 4, 1027
    args = [(role, i, 1, W.NW, port, "dist_sync", "cuda", name, cfg, steps, Rl, D, N)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(110) for r in [pool.apply_async(W.kv_opt_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    seen, dense, table = W.predict(name, cfg, steps, Rl, D, N)
    for o in workers:
        r = o["rank"]
        assert o["sparse_ops"] == ([4, 0, 4, 0] if r == 0 else [2, 1, 4, 0]), o["sparse_ops"]
        assert o["plane_ops"][0] >= steps and o["plane_ops"][1] >= 2 * steps, o["plane_ops"]
        for s in range(steps):
            ids = np.unique(SW.pull_ids(r, s, Rl))
            assert o["seen"][s][1].tolist() == ids.tolist()
            assert np.array_equal(ref.bits(o["seen"][s][0]), ref.bits(seen[s][0])), f"worker {r} step {s}: dense key"
            assert np.array_equal(ref.bits(o["seen"][s][2]), ref.bits(seen[s][1][ids])), f"worker {r} step {s}: rows"
        assert np.array_equal(ref.bits(o["table"]), ref.bits(table)), f"worker {r}: final table"
        assert np.array_equal(ref.bits(o["dense"]), ref.bits(dense)), f"worker {r}: final dense key"
    assert not np.array_equal(table, SW.table0(Rl, D, False))
