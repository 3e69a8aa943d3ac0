"""The kvstore's fused optimizer kinds on the CPU (tony_amd/parallel/kvstore.py: nag, adagrad, rmsprop plain and
centered, ftrl): the numpy contract (tests/kv_optim_ref.py) against a float64 evaluation within its counted bounds,
its fixed points, the torch composition bit for bit against it (dense, lazy, bf16 / fp16 keys), the settings' JSON
round trip, a local store and one dist_sync run over gloo in spawned CPU processes."""
import json
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_optim_ref as ref
import kv_optim_workers as W
import kv_sparse_ref as sref
import kv_sparse_workers as SW
import tony_amd.kv as kv

R, D = 12, 4

# every kind plain and with wd, rescale_grad and clip_gradient (the learning rates no power of two: they round)
PLAIN = {"nag0": ("nag", dict(learning_rate=0.1)),
         "nag": ("nag", dict(learning_rate=0.1, momentum=0.9)),
         "adagrad": ("adagrad", dict(learning_rate=0.1)),
         "rmsprop": ("rmsprop", dict(learning_rate=0.01)),
         "rmsprop-centered": ("rmsprop", dict(learning_rate=0.01, centered=True, gamma1=0.95, gamma2=0.8)),
         "ftrl": ("ftrl", dict(learning_rate=0.1, lamda1=0.5))}
EXTRA = dict(wd=0.01, rescale_grad=0.3, clip_gradient=2.0)
CASES = {**PLAIN, **{k + "-wd-clip": (n, dict(c, **EXTRA)) for k, (n, c) in PLAIN.items()}}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs are not where the contract has them"
    g, w = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    assert np.array_equal(ref.bits(g), ref.bits(w)), f"{what}: {int((ref.bits(g) != ref.bits(w)).sum())} differ"


def _states(name, cfg, shape, seed):
    """Non-trivial exact fp32 states: the second moments positive, centered rmsprop's ``n`` well above ``g^2``."""
    rng = np.random.default_rng(seed)
    st = {}
    for k in ref.state_names(name, dict(ref.DEFAULTS, **cfg)):
        st[k] = rng.standard_normal(shape).astype(np.float32)
    if "history" in st:
        st["history"] = np.abs(st["history"])
    if name == "ftrl":
        st["n"] = np.abs(st["n"])
    if name == "rmsprop":
        st["n"] = (np.abs(st["n"]) + (st["g"] ** 2 if "g" in st else 0) + np.float32(0.5)).astype(np.float32)
    return st


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_is_within_its_counted_bound_of_float64(case):
    name, cfg = CASES[case]
    rng = np.random.default_rng(len(case))
    w = rng.standard_normal((64, 8)).astype(np.float32)
    g = (rng.standard_normal((64, 8)) * 10.0 ** rng.integers(-3, 3, (64, 1))).astype(np.float32)
    g[0, 0] = 0.0
    for st in ({}, _states(name, cfg, w.shape, 5)):  # zero states (the first update of a key) and states in use
        w32, s32, bounds = ref.step(name, w, st, None, g, **cfg)
        w64, s64 = ref.step64(name, w, st, g, **cfg)
        ref.within(w32, w64, bounds["w"], f"{case}: weight")
        assert sorted(s32) == sorted(s64) == sorted(ref.state_names(name, dict(ref.DEFAULTS, **cfg)))
        for k in s32:
            ref.within(s32[k], s64[k], bounds[k], f"{case}: state {k}")
        assert np.abs(w32 - w).max() > 0 and np.isfinite(bounds["w"]).all()


def test_ftrl_inside_lamda1_gives_exactly_plus_zero():
    w = np.full((4, 4), -0.75, np.float32)
    g = np.asarray([[0.1, -0.2, 0.0, 0.3]] * 4, np.float32)
    got, st, _ = ref.step("ftrl", w, {}, None, g, learning_rate=0.1, lamda1=10.0)
    assert np.all(np.abs(st["z"]) <= 10.0)
    assert np.array_equal(ref.bits(got), np.zeros((4, 4), np.uint32))  # +0.0, not -0.0
    opt = kv.create_optimizer("ftrl", learning_rate=0.1, lamda1=10.0)
    wt = _t(w.copy())
    opt.update(0, wt, _t(g))
    assert np.array_equal(ref.bits(wt.numpy()), np.zeros((4, 4), np.uint32))
    z = st["z"].copy()
    z[0, 0] = np.nan  # a NaN z takes the division branch
    got, _, _ = ref.step("ftrl", w, {"z": z, "n": st["n"]}, None, np.zeros_like(g), learning_rate=0.1, lamda1=10.0)
    assert np.isnan(got[0, 0]) and np.isnan(got).sum() == 1


@pytest.mark.parametrize("cfg", [dict(lr=0.1), dict(lr=0.1, wd=0.01, rescale=0.3, clip=2.0)])
def test_nag_at_momentum_zero_is_lazy_sgd_bit_for_bit(cfg):
    rng = np.random.default_rng(3)
    w = rng.standard_normal((R, D)).astype(np.float32)
    ids = np.asarray([0, 5, R - 1], np.int64)
    g = (rng.standard_normal((3, D)) * 3).astype(np.float32)
    g[0, 1] = np.nan
    a, m, _, _ = ref.nag(w, None, ids, g, momentum=0.0, **cfg)
    b, _, _, _ = sref.sgd(w, None, ids, g, momentum=0.0, **cfg)
    assert m is None
    _same_bits(a, b, "nag at momentum 0 against lazy SGD")


def test_adagrad_first_step_moves_by_lr_sign_g():
    g = np.asarray([3.0, -0.02, 0.5, -50.0], np.float32)
    w = np.zeros(4, np.float32)
    got, st, _ = ref.step("adagrad", w, {}, None, g, learning_rate=0.1)
    assert np.allclose(got, -0.1 * np.sign(g), rtol=1e-3, atol=0)  # g / sqrt(g^2 + 1e-7): 1e-7 << g^2
    assert np.array_equal(st["history"], (g * g).astype(np.float32))


def _torch_states(opt, key):
    return {k: v for k, v in opt.state[key].items() if k != "t"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_path_equals_the_reference_bit_for_bit_dense_and_lazy(case):
    """Three steps of the dense update of a [37] key and of the lazy update of a [R, D] key: weight and every state
    equal the contract bit for bit, a NaN where it has one, and untouched rows keep their bits."""
    name, cfg = CASES[case]
    rng = np.random.default_rng(11)
    opt = kv.create_optimizer(name, **cfg)
    w = rng.standard_normal(37).astype(np.float32)
    wt, st = _t(w.copy()), {}
    tab = rng.standard_normal((R, D)).astype(np.float32)
    tt, ts = _t(tab.copy()), {}
    for step, ids in enumerate([[0, 5, 7, R - 1], [5, 6], [0, 7, R - 1]]):
        g = (rng.standard_normal(37) * 3).astype(np.float32)
        g[1], g[2], g[3] = np.nan, 100.0, -100.0
        opt.update(1, wt, _t(g))
        w, st, _ = ref.step(name, w, st, None, g, **cfg)
        _same_bits(wt.numpy(), w, f"{case} step {step}: dense weight")
        assert sorted(_torch_states(opt, 1)) == sorted(st)
        for k in st:
            _same_bits(opt.state[1][k].numpy(), st[k], f"{case} step {step}: dense {k}")
        ids = np.asarray(ids, np.int64)
        gr = (rng.standard_normal((ids.size, D)) * 3).astype(np.float32)
        gr[0, 1], gr[-1, 2], gr[0, 3] = np.nan, 100.0, -100.0
        before_w, before_s = tab, ts
        opt.update_rows(2, tt, _t(ids), _t(gr))
        tab, ts, _ = ref.step(name, tab, ts, ids, gr, **cfg)
        rest = np.setdiff1d(np.arange(R), ids)
        _same_bits(tt.numpy(), tab, f"{case} step {step}: lazy weight")
        assert np.array_equal(ref.bits(tt.numpy()[rest]), ref.bits(before_w[rest]))
        for k in ts:
            got = opt.state[2][k].numpy()
            assert got.shape == (R, D) and got.dtype == np.float32
            _same_bits(got, ts[k], f"{case} step {step}: lazy {k}")
            was = before_s.get(k, np.zeros_like(tab))
            assert np.array_equal(ref.bits(got[rest]), ref.bits(was[rest])), f"{case}: untouched rows of {k}"
    assert np.isnan(w[1]) and np.isnan(w).sum() == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(PLAIN))
def test_half_keys_equal_the_reference_rounded_once(case, dtype):
    """A bf16 / fp16 key with a gradient of its dtype: the update runs in fp32 from the key's values and is rounded
    once on the store; the states stay fp32."""
    name, cfg = CASES[case + "-wd-clip"]
    rng = np.random.default_rng(5)
    wt = _t(rng.standard_normal((R, D)).astype(np.float32)).to(dtype)
    opt = kv.create_optimizer(name, **cfg)
    st = {}
    for step in range(3):
        g = _t((rng.standard_normal((R, D)) * 3).astype(np.float32)).to(dtype)
        want, st, _ = ref.step(name, wt.float().numpy(), st, None, g.float().numpy(), **cfg)
        opt.update(0, wt, g)
        assert wt.dtype == dtype
        assert torch.equal(wt, _t(want).to(dtype)), f"{case} {dtype} step {step}"
        for k in st:
            assert opt.state[0][k].dtype == torch.float32
            _same_bits(opt.state[0][k].numpy(), st[k], f"{case} {dtype} step {step}: {k}")


def test_settings_round_trip_through_json_and_bad_ones_are_refused():
    new = dict(gamma1=0.95, gamma2=0.8, centered=True, epsilon=1e-6, lamda1=0.25, beta=2.0)
    opt = kv.create_optimizer("rmsprop", learning_rate=0.3, wd=0.01, **new)
    back = kv.Optimizer.from_json(opt.to_json())
    assert back.cfg == opt.cfg and back.name == "rmsprop"
    for k, v in new.items():
        assert json.loads(opt.to_json())[k] == v
    for name in ("nag", "adagrad", "ftrl"):
        o = kv.create_optimizer(name, lamda1=0.25, beta=2.0, momentum=0.5)
        assert kv.Optimizer.from_json(o.to_json()).cfg == o.cfg
    # epsilon takes a per-kind default when it is not given
    assert kv.create_optimizer("adagrad").cfg["epsilon"] == 1e-7
    assert kv.create_optimizer("rmsprop").cfg["epsilon"] == 1e-8
    assert kv.create_optimizer("adagrad", epsilon=1e-3).cfg["epsilon"] == 1e-3
    # sgd and adam keep exactly the keys they had
    old = ["name", "learning_rate", "momentum", "wd", "rescale_grad", "clip_gradient", "beta1", "beta2", "epsilon"]
    for name in ("sgd", "adam"):
        assert list(json.loads(kv.create_optimizer(name).to_json())) == old
        assert kv.create_optimizer(name).cfg["epsilon"] == 1e-8
    for name, bad in (("sgd", dict(centered=True)), ("sgd", dict(lamda1=-1.0)), ("adam", dict(gamma1=0.5)),
                      ("sgd", dict(beta=2.0)), ("adam", dict(gamma2=0.5)), ("adagrad", dict(centered=True)),
                      ("ftrl", dict(lamda1=-0.1)),
                      ("adagrad", dict(epsilon=-1e-7)), ("rmsprop", dict(gamma1=-0.5)),
                      ("rmsprop", dict(gamma2=-0.5)), ("lamb", {}), ("adadelta", {})):
        with pytest.raises(ValueError):
            kv.create_optimizer(name, **bad)
    assert sorted(kv.Optimizer._ROW_STATE) == ["adagrad", "adam", "ftrl", "nag", "rmsprop", "sgd"]
    o = kv.create_optimizer("ftrl")
    o.update(3, torch.ones(4), torch.ones(4))
    assert sorted(k for k in o.state_dict()["state"][3] if k != "t") == ["n", "z"]


@pytest.mark.parametrize("case", ["adagrad", "ftrl", "nag0"])
def test_a_missized_gradient_raises_and_writes_nothing(case):
    """A gradient of another element count than the key (dense), or rows that do not match their ids (lazy), is a
    ``ValueError`` before anything is touched, through the optimizer and through a local store's push."""
    name, cfg = CASES[case]
    opt = kv.create_optimizer(name, **cfg)
    w, tab = torch.ones(8), torch.ones(R, D)
    for g in (torch.ones(7), torch.ones(9), torch.ones(2, 8)):
        with pytest.raises(ValueError):
            opt.update(0, w, g)
    for ids, rows in ((torch.tensor([1, 2]), torch.ones(1, D)), (torch.tensor([1]), torch.ones(2, D)),
                      (torch.tensor([1, 2]), torch.ones(2, D + 1)), (torch.tensor([[1, 2]]), torch.ones(2, D))):
        with pytest.raises(ValueError):
            opt.update_rows(1, tab, ids, rows)
    store = kv.create("local")
    store.init("d", w)
    store.set_optimizer(opt)
    with pytest.raises(ValueError):
        store.push("d", torch.ones(4))
    got = torch.zeros(8)
    store.pull("d", out=got)
    assert bool((w == 1).all()) and bool((tab == 1).all()) and bool((got == 1).all())
    assert all(not bool(t.any()) for st in opt.state.values() for k, t in st.items() if k != "t")


@pytest.mark.parametrize("case", ["adagrad-wd-clip", "ftrl", "rmsprop-centered", "nag"])
def test_local_store_with_dense_and_sparse_keys(case):
    name, cfg = CASES[case]
    N = 10
    store = kv.create("local")
    tab, dense = SW.table0(R, D, False), W.dense0(N)
    store.init("emb", kv.RowSparse(torch.arange(R), _t(tab.copy()), (R, D)))
    store.init("d", _t(dense.copy()))
    store.set_optimizer(kv.create_optimizer(name, **cfg))
    ts, ds = {}, {}
    for step in range(3):
        pushes = SW.pushes_of(0, step, R, D, False) + SW.pushes_of(1, step, R, D, False)
        store.push("emb", [SW._rsp(kv, p, (R, D), "cpu") for p in pushes])
        g = [W.dense_grad(r, step, N) for r in range(2)]
        store.push("d", [_t(x) for x in g])
        ids, rows = sref.merge(pushes)
        tab, ts, _ = ref.step(name, tab, ts, ids, rows, **cfg)
        dense, ds, _ = ref.step(name, dense, ds, None, (g[0] + g[1]).astype(np.float32), **cfg)
        got_t, got_d = torch.empty(R, D), torch.empty(N)
        store.pull("emb", out=got_t, ignore_sparse=False)
        store.pull("d", out=got_d)
        _same_bits(got_t.numpy(), tab, f"{case} step {step}: table")
        _same_bits(got_d.numpy(), dense, f"{case} step {step}: dense key")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dist_sync_over_gloo_follows_the_reference():
    """1 scheduler + 1 server + 2 workers over gloo, four steps of a dense and a sparse key under ftrl: the setting
    reaches the server as JSON, and every pull after a push sees the round's ordered merge followed by the update,
    bit for bit."""
    name, cfg = CASES["ftrl-wd-clip"]
    steps, N, port = 4, 10, _port()
    args = [(role, i, 1, W.NW, port, "dist_sync", "cpu", name, cfg, steps, R, D, N)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(150) for r in [pool.apply_async(W.kv_opt_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    seen, dense, table = W.predict(name, cfg, steps, R, D, N)
    for o in workers:
        r = o["rank"]
        for s in range(steps):
            ids = np.unique(SW.pull_ids(r, s, R))
            assert o["seen"][s][1].tolist() == ids.tolist()
            _same_bits(o["seen"][s][0], seen[s][0], f"worker {r} step {s}: dense key")
            _same_bits(o["seen"][s][2], seen[s][1][ids], f"worker {r} step {s}: pulled rows")
        _same_bits(o["table"], table, f"worker {r}: final table")
        _same_bits(o["dense"], dense, f"worker {r}: final dense key")
    assert not np.array_equal(table, SW.table0(R, D, False))
