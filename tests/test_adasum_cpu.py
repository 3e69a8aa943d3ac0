"""Adasum without a GPU: the identities of the combine, the torch fallback of ``tony_amd.ops.adasum`` against the
numpy contract (tests/adasum_ref.py), the numpy contract inside the derived bound against the float64 tree, and gloo
ranks on CPU tensors through ``hvd.allreduce`` / ``grouped_allreduce`` / ``DistributedOptimizer`` with
``op=hvd.Adasum`` (tests/adasum_worker.py is the rank body)."""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import adasum_ref as R

pytestmark = pytest.mark.timeout(240)


def _plan(segs, dtype=torch.float32):
    from tony_amd.ops.adasum import AdasumPlan
    from tony_amd.ops.optim import Segments

    return AdasumPlan(Segments([0] + [hi for _, hi in segs], list(range(len(segs))), [True] * len(segs)), dtype, "cpu")


def _combine(a, b, segs, dtype=torch.float32, dst_is_a=True):
    from tony_amd.ops.adasum import combine_

    ta, tb = torch.from_numpy(a.copy()).to(dtype), torch.from_numpy(b.copy()).to(dtype)
    dst, other = (ta, tb) if dst_is_a else (tb, ta)
    keep = other.clone()
    out = combine_(dst, other, dst_is_a, _plan(segs, dtype))
    assert out is dst and torch.equal(other, keep)
    return dst.float().numpy()


def _vec(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_identities(dtype):
    bf = dtype == torch.bfloat16
    n, segs = 256, [(0, 128), (128, 256)]
    x, zero = _vec(n, 1), np.zeros(n, dtype=np.float32)
    x = R.to_bf16(x) if bf else x
    # orthogonal tensors add: disjoint supports inside each tensor; every sum has one non-zero term, so it is exact
    a, b = x.copy(), x.copy()
    a[1::2] = 0
    b[0::2] = 0
    assert np.array_equal(_combine(a, b, segs, dtype), a + b)
    # equal tensors return themselves, a zero side returns the other side, two zero sides give zero: bit for bit
    assert np.array_equal(_combine(x, x.copy(), segs, dtype), x)
    for dst_is_a in (True, False):
        assert np.array_equal(_combine(x, zero, segs, dtype, dst_is_a), x)
        assert np.array_equal(_combine(zero, x, segs, dtype, dst_is_a), x)
    out = _combine(zero, zero.copy(), segs, dtype)
    assert np.array_equal(out, zero) and not np.signbit(out).any()
    # one tensor zero, the other not: each tensor has its own coefficients
    half = x.copy()
    half[128:] = 0
    assert np.array_equal(_combine(x, half, segs, dtype), x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_torch_fallback_is_the_numpy_contract(dtype):
    bf = dtype == torch.bfloat16
    (a, b), segs = R.make_grads(2, seed=5, bf16=bf)
    want = R.combine_np(a, b, segs, bf)
    assert np.array_equal(_combine(a, b, segs, dtype, True), want)
    assert np.array_equal(_combine(a, b, segs, dtype, False), want)   # the b side computes the same bits
    for lo, hi in segs:  # the padding stays zero
        ln = R.LENGTHS[[s[0] for s in segs].index(lo)]
        assert not want[lo + ln:hi].any()
    # per tensor, not over the buffer: one segment over everything gives other coefficients and another result
    assert not np.array_equal(R.combine_np(a, b, [(0, a.size)], bf), want)


def test_plan_refuses_what_it_cannot_combine():
    from tony_amd.ops.adasum import AdasumPlan, check_world, combine_
    from tony_amd.ops.optim import Segments

    with pytest.raises(TypeError):
        AdasumPlan(Segments.whole(8), torch.int32, "cpu")
    plan = AdasumPlan(Segments.whole(8), torch.float32, "cpu")
    with pytest.raises(ValueError):
        combine_(torch.zeros(12), torch.zeros(12), True, plan)
    t = torch.zeros(8)
    with pytest.raises(ValueError):
        combine_(t, t, True, plan)
    for n in (3, 6, 0):
        with pytest.raises(ValueError):
            check_world(n)
    for n in (1, 2, 8):
        check_world(n)
    packed = AdasumPlan.packed([7, 4, 9], torch.bfloat16, "cpu")
    assert packed.offsets == [0, 8, 16] and packed.numel == 32


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_numpy_contract_stays_inside_the_derived_bound(world, bf16):
    """The emulation alone, against the float64 tree: measured error / (2^-24 mag) beside the bound K, per tensor."""
    lengths = R.LENGTHS + [5, 100003]
    grads, segs = R.make_grads(world, lengths=lengths, seed=3, bf16=bf16)
    ref = R.tree_ref(grads, segs, bf16)
    assert all(0.1 <= c <= 1.5 for pair in ref.coefs for c in pair)
    got = R.tree_np(grads, segs, bf16)
    m = R.measured(got, ref, segs)
    print(f"world {world} bf16 {bf16}: measured {[round(x, 2) for x in m]} bound K {[round(k, 2) for k in ref.K]}")
    assert all(x <= k for x, k in zip(m, ref.K))
    assert (np.abs(got.astype(np.float64) - ref.val) <= ref.bound(segs)).all()
    levels = world.bit_length() - 1
    base = (3 + (R.R_BF16 if bf16 else 0)) * levels  # the count without the sensitivities
    assert all(base <= k for k in ref.K)
    # and it is not loose by orders of magnitude (tensors of a handful of elements aside: their coefficients are
    # the most sensitive, every element carrying a large share of the sums)
    assert all(k <= 100 * base for k, n in zip(ref.K, lengths) if n >= 4096)
    if bf16:
        assert np.array_equal(R.to_bf16(got), got)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks(world):
    import adasum_worker as W

    port = _port()
    ctx = mp.get_context("spawn")
    with ctx.Pool(world) as pool:
        res = [pool.apply_async(W.cpu_rank, (r, world, port)) for r in range(world)]
        return [r.get(200) for r in res]


def _f32(b):
    return np.frombuffer(b, dtype=np.float32)


def check_api(outs, world, bf16=False):
    """What every rank's ``adasum_worker.api_body`` returned, against the references (shared with the GPU test)."""
    grads, segs = R.make_grads(world, seed=11)
    offs = [lo for lo, _ in segs]
    api = [o["api"] for o in outs]
    for o in api[1:]:  # all ranks bit-identical
        assert o == api[0]
    a = api[0]
    bad = [k for k, v in a.items() if v is False]
    assert not bad, bad
    per_tensor = [[g[o:o + n] for g in grads] for o, n in zip(offs, R.LENGTHS)]
    refs = [R.tree_ref(gs, [(0, len(gs[0]))]) for gs in per_tensor]

    def inside(bits, t):
        got, ref = _f32(bits), refs[t]
        assert got.shape == ref.val.shape
        m = R.measured(got, ref, [(0, got.size)])
        print(f"tensor {t}: measured {m[0]:.2f} bound K {ref.K[0]:.2f}")
        assert (np.abs(got.astype(np.float64) - ref.val) <= ref.bound([(0, got.size)])).all()

    for t in (1, 4):
        inside(a[f"single{t}"], t)
    assert len(a["grouped"]) == len(R.LENGTHS)
    for t, bits in enumerate(a["grouped"]):
        inside(bits, t)
    # a tensor's result does not depend on what it was packed with; the scaled call and the async forms agree too
    assert a["grouped"][1] == a["single1"] and a["grouped"][4] == a["single4"]
    assert a["scaled"] == a["grouped"]
    assert a["async"] == a["grouped"][3] and a["async_copy"] == a["grouped"][3] and a["inplace"] == a["grouped"][2]


def check_opt(outs, world, name="opt", bf16=False, want_fused=False):
    """What every rank's ``adasum_worker.opt_body`` returned: the gradient buffers of every step bit-identical over
    the ranks, inside the bound against the float64 tree of the returned local gradients, far from their sum and
    from their average; the variables after the last step bit-identical."""
    import adasum_worker as W

    res = [o[name] for o in outs]
    _, segs, n = R.layout()
    for r, o in enumerate(res):
        assert o["buckets"] > 3 and o["reduce"] == "adasum" and o["layout_matches"], (r, o["buckets"])
        assert o["fused"] == want_fused and o["launches"] == W.STEPS * o["buckets"]
        assert o["grad"] == res[0]["grad"] and o["vars"] == res[0]["vars"]
        assert len(o["vars"]) == 4 * n
    for s in range(W.STEPS):
        local = [_f32(o["local"][s]) for o in res]
        want, _ = R.make_grads(world, seed=1000 + s)
        for r in range(world):  # the loss is built so: this rank's gradient, to the bit
            assert np.array_equal(local[r], want[r])
        leaves = [R.to_bf16(g) for g in local] if bf16 else local
        ref = R.tree_ref(leaves, segs, bf16)
        got = _f32(res[0]["grad"][s])
        m = R.measured(got, ref, segs)
        print(f"{name} step {s}: measured {[round(x, 2) for x in m]} bound K {[round(k, 2) for k in ref.K]}")
        bound = ref.bound(segs)
        assert (np.abs(got.astype(np.float64) - ref.val) <= bound).all()
        # a plain all-reduce must not be able to pass: the sum and the average lie far outside the bound.  The large
        # tensors have cosines about 0.5 and coefficients about 0.75, so where the ranks' elements share a sign the
        # result is about 0.75 (two ranks) or 0.56 (four) of the sum, off the sum and off the average by 0.33 to 0.78
        # of mag; the bound is K 2^-24 of mag, 2e-7 to 1e-6 in fp32 and 0.004 (two ranks) to 0.025 (four) in bf16:
        # a factor above 10^5 in fp32 and of 22 to 83 in bf16
        total = np.sum([g.astype(np.float64) for g in leaves], axis=0)
        live = bound > 0
        for what, alt in (("sum", total), ("average", total / world)):
            far = np.abs(alt - ref.val)[live] / bound[live]
            print(f"{name} step {s}: the {what} is {far.max():.1f} bounds away")
            assert far.max() > (10 if bf16 else 100), (name, s, what, far.max())
    assert np.isfinite(_f32(res[0]["vars"])).all()


@pytest.mark.parametrize("world", [2, 4])
def test_gloo_ranks(world):
    outs = _ranks(world)
    check_api(outs, world)
    check_opt(outs, world)


def test_three_ranks_raise_value_error():
    for o in _ranks(3):
        for name, what in o["refusals"].items():
            assert what.startswith("ValueError") and "power-of-two" in what, (name, what)


def test_distributed_optimizer_constructs_on_one_rank():
    """One rank is the identity: the operator is accepted with the plain path, rejects a predivide factor, and a step
    leaves the gradient as it was."""
    import tony_amd.hvd as hvd

    hvd.init()
    try:
        net = torch.nn.Linear(4, 3)
        opt = hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1), op=hvd.Adasum,
                                       backward_passes_per_step=2)
        assert opt.groups[0][1].reduce == "adasum"
        net(torch.ones(2, 4)).sum().backward()
        g = opt.groups[0][0].grad.clone()
        opt.step()
        assert torch.equal(opt.groups[0][0].grad, g)
        with pytest.raises(ValueError):
            hvd.DistributedOptimizer(torch.optim.SGD(torch.nn.Linear(4, 3).parameters(), lr=0.1), op=hvd.Adasum,
                                     gradient_predivide_factor=2.0)
        x = torch.arange(6.0)
        assert torch.equal(hvd.allreduce(x, op=hvd.Adasum, prescale_factor=0.5, postscale_factor=4.0), 2 * x)
        with pytest.raises(TypeError):
            hvd.allreduce(torch.arange(6), op=hvd.Adasum)
    finally:
        hvd.shutdown()
