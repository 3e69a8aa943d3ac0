"""Multi-precision kvstore keys on the GPU: ``tony_kv_mp_dense`` / ``tony_kv_mp_rows`` (csrc/kv_mp.hip) through
``Optimizer.update`` / ``update_rows`` and the stores, bit for bit against the numpy contract (tests/kv_mp_ref.py).
Every run asserts the launch counters, so a silent fall-back to the torch path fails."""
import multiprocessing as mp_
import socket

import numpy as np
import pytest
import torch

import kv_mp_ref as mp
import kv_mp_workers as W
from test_kv_mp_cpu import bits16, f32, problem, run_dense, source, t16

pytestmark = pytest.mark.gpu

TURN = 256 * 8  # one workgroup turn: 256 lanes of 8 elements
# tony_kv_mp_dense launches at most 1024 workgroups: past 1024 * TURN elements the grid stride takes a second turn
SECOND_TURN = 1024 * TURN + TURN + 5
SIZES = [1, 7, 8, 9, TURN - 1, TURN + 5]
DENSE = [(n, k) for n in SIZES + [SECOND_TURN] for k in (1, 3, 8)]


@pytest.mark.parametrize("n,nsrc", DENSE)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(mp.KINDS))
def test_dense_kernel_bit_exact(case, dtype, n, nsrc):
    import tony_amd.kv as kv

    run_dense(kv, case, n, nsrc, dtype, torch.device("cuda", 0), 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(mp.KINDS))
def test_nine_sources_take_the_torch_path_with_the_same_bits(case, dtype):
    import tony_amd.kv as kv

    run_dense(kv, case, TURN + 5, 9, dtype, torch.device("cuda", 0), 0)


P = 2.0 ** np.arange(-30, 1)[::-1]  # P[k] = 2^-k
ROUNDING = {  # dtype, w, g, the exact w - g, the stored value
    "bf16-tie-down": ("bf16", 1.0, -P[8], 1 + P[8], 1.0),
    "bf16-tie-up": ("bf16", 1 + P[7], -P[8], 1 + 3 * P[8], 1 + P[6]),
    "fp16-tie-down": ("fp16", 1.0, -P[11], 1 + P[11], 1.0),
    "fp16-tie-up": ("fp16", 1 + P[10], -P[11], 1 + 3 * P[11], 1 + P[9]),
    "fp16-overflow": ("fp16", 65504.0, -32.0, 65536.0, np.inf),
    "fp16-subnormal-tie": ("fp16", P[24], P[25], P[25], 0.0),
    "bf16-nan": ("bf16", 1.0, np.nan, np.nan, np.nan),
    "fp16-nan": ("fp16", 1.0, np.nan, np.nan, np.nan),
}


@pytest.mark.parametrize("row", sorted(ROUNDING))
def test_rounding_by_construction(row):
    """Plain SGD with lr 1, wd 0, rescale 1 and one fp32 source: ``w32' = w - g`` is exact, the stored value its
    rounding to nearest even.  9 elements: a chunk of the vector path and one of the element-wise tail."""
    import tony_amd.kv as kv

    dtype, w, g, exact, stored = ROUNDING[row]
    dev = torch.device("cuda", 0)
    wt = torch.full((9,), w, dtype=torch.float32).to(mp_dtype(dtype)).to(dev)
    assert float(wt[0]) == w  # the stored value holds w exactly
    opt = kv.create_optimizer("sgd", learning_rate=1.0, multi_precision=True)
    opt.update(0, wt, torch.full((9,), g, dtype=torch.float32, device=dev))
    assert opt.kernel_ops == [0, 0, 1, 0]
    mp.same_bits(f32(opt.state[0]["w32"]), np.full(9, exact, np.float32), f"{row}: w32")
    want = np.full(9, stored, np.float32)
    want16 = want.astype(np.float16).view(np.uint16) if dtype == "fp16" else (want.view(np.uint32) >> 16).astype(np.uint16)
    mp.same_bits(bits16(wt), want16, f"{row}: stored value", dtype)


def mp_dtype(dtype):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]


def test_updates_below_half_an_ulp_are_kept_by_the_master_only():
    """64 updates of 2^-10 on a bf16 1.0 (ulp below it: 2^-8): the master ends at exactly 1 - 2^-4, the stored value
    at 0.9375; the same key without the flag never moves."""
    import tony_amd.kv as kv

    dev = torch.device("cuda", 0)
    g = torch.full((9,), 2.0 ** -10, dtype=torch.bfloat16, device=dev)
    keys = {}
    for flag in (True, False):
        opt = kv.create_optimizer("sgd", learning_rate=1.0, **({"multi_precision": True} if flag else {}))
        keys[flag] = torch.ones(9, dtype=torch.bfloat16, device=dev)
        for _ in range(64):
            opt.update(0, keys[flag], g)
        if flag:
            assert opt.kernel_ops == [0, 0, 64, 0]
            assert bool((opt.state[0]["w32"] == 1 - 2.0 ** -4).all())
    assert bool((keys[True].float() == 0.9375).all()) and bool((keys[False].float() == 1.0).all())


@pytest.mark.parametrize("D,launches", [(8, 1), (24, 1), (12, 0)])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ["sgd-mom", "rmsprop-centered", "ftrl"])
def test_lazy_rows(case, dtype, D, launches):
    """Two lazy updates (a 16-bit, then an fp32 merged gradient) of a [16, D] table filled with random bits' worth of
    values: rows of 8 and 24 elements take ``tony_kv_mp_rows``, 12 the gather / update / scatter; the touched rows
    equal the contract and every other row of the table, the master and the states keeps its bits."""
    import tony_amd.kv as kv

    name, cfg = mp.KINDS[case]
    dev, R = torch.device("cuda", 0), 16
    rng = np.random.default_rng(D)
    tbits = mp.rne16(rng.standard_normal((R, D)).astype(np.float32), dtype)
    table = t16(tbits, dtype, dev)
    opt = kv.create_optimizer(name, multi_precision=True, **cfg)
    w32, st = mp.widen(tbits, dtype).reshape(R, D), {}
    for step, ids in enumerate(([0, 3, 7, R - 1], [0, 5, R - 1])):
        ids = np.asarray(ids, np.int64)
        g = (rng.standard_normal((ids.size, D)) * 3).astype(np.float32)
        src = g if step else (mp.rne16(g, dtype), dtype)
        opt.update_rows(0, table, torch.from_numpy(ids).to(dev), source(src, dtype, dev))
        w32, st, stored = mp.step(case, w32, st, ids, [src], dtype)
        what = f"{case} {dtype} D {D} step {step}"
        mp.same_bits(bits16(table), stored, f"{what}: table", dtype)
        mp.same_bits(f32(opt.state[0]["w32"]), w32, f"{what}: w32")
        for k in st:
            mp.same_bits(f32(opt.state[0][k]), st[k], f"{what}: {k}")
        assert opt.kernel_ops == [0, 0, 0, launches * (step + 1)], opt.kernel_ops
    assert opt.update_rows(0, table, torch.zeros(0, dtype=torch.int64, device=dev),
                           torch.zeros(0, D, device=dev)) is None  # no ids: nothing is launched
    assert opt.kernel_ops[3] == 2 * launches


def test_dist_sync_server_applies_the_round_in_one_launch(monkeypatch):
    """A scheduler, one server and two workers sharing the GPU, one dist_sync round of a bf16 key on the plane under
    nag: the pulled value is the contract's for the sources [worker 0's push, worker 1's push], and the server made one
    ``tony_kv_mp_dense`` launch."""
    monkeypatch.setenv("TONY_KV_WAIT_S", "60")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    name, cfg = mp.KINDS["nag"]
    args = [(role, i, 2, port, name, cfg) for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    with mp_.get_context("spawn").Pool(len(args)) as pool:
        outs = [r.get(110) for r in [pool.apply_async(W.kv_mp_rank, a) for a in args]]
    server = next(o for o in outs if o["role"] == "server")
    assert server["kernel_ops"] == [0, 0, 1, 0], server
    srcs = [(mp.rne16(W.push_of(r), "bf16"), "bf16") for r in range(2)]
    _, _, stored = mp.step("nag", W.key0(), {}, None, srcs, "bf16")
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    for o in workers:
        assert o["plane_ops"] == [1, 1], o["plane_ops"]
        mp.same_bits(o["pulled"], stored, f"worker {o['rank']}: pulled value", "bf16")
