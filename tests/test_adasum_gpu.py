"""The Adasum kernels (csrc/adasum.hip through tony_amd.ops.adasum) in one process, at the smallest shapes at which they
can go wrong: one buffer of tensors of 4, 7, 4096 (exactly one work item), 4100 (an item and a 4-element tail) and
3 * 4096 + 8 elements, each padded to the flat buffers' alignment, in fp32 and in bf16, with poisoned guards before and
after the buffer.  tests/adasum_ref.py holds the contract, the float64 reference and the bound."""
import numpy as np
import pytest
import torch

import adasum_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = 1234.5  # exact in bf16
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _segments(segs):
    from tony_amd.ops.optim import Segments

    return Segments([0] + [hi for _, hi in segs], list(range(len(segs))), [True] * len(segs))


def _guarded(x, dtype, dev):
    """``x`` on the device between two poisoned guards: (the whole allocation, the view of ``x``)."""
    big = torch.full((GUARD + x.size + GUARD,), POISON, dtype=dtype, device=dev)
    big[GUARD:GUARD + x.size] = torch.from_numpy(x).to(dev)
    return big, big[GUARD:GUARD + x.size]


def _guards_intact(big):
    return bool((big[:GUARD] == POISON).all() and (big[-GUARD:] == POISON).all())


def _np(t):
    return t.detach().float().cpu().numpy()


class Case:
    """The two sides, their layout and the references of one dtype, computed once."""

    def __init__(self, name, dev):
        from tony_amd.ops.adasum import AdasumPlan

        self.bf16 = name == "bf16"
        self.dtype, self.dev = DTYPES[name], dev
        (self.a, self.b), self.segs = R.make_grads(2, seed=21, bf16=self.bf16)
        self.offs = [lo for lo, _ in self.segs]
        self.plan = AdasumPlan(_segments(self.segs), self.dtype, dev)
        self.ref = R.tree_ref([self.a, self.b], self.segs, self.bf16)
        self.want = R.combine_np(self.a, self.b, self.segs, self.bf16)

    def sides(self):
        return _guarded(self.a, self.dtype, self.dev), _guarded(self.b, self.dtype, self.dev)


_CASES = {}


@pytest.fixture(params=list(DTYPES))
def case(request, cuda):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param, cuda)
    return _CASES[request.param]


def _tensor_triples(plan):
    """Every tensor's (a.b, a.a, b.b) from the item triples, summed on the host in item order."""
    part = plan.partials.cpu().numpy()
    order, tstart = plan.order.cpu().numpy(), plan.tstart.cpu().numpy()
    return [[sum(float(part[j, k]) for j in order[tstart[t]:tstart[t + 1]]) for k in range(3)]
            for t in range(plan.n_tensors)]


def test_work_list_cuts_every_tensor_from_its_own_start(case):
    vec = 4 if not case.bf16 else 8
    items = case.plan.items.cpu().numpy()
    counts = [1, 1, 1, 2, 4]  # 64, 64, 4096, 4160 and 12352 padded elements in items of at most 4096
    assert [int((items[:, 2] == t).sum()) for t in range(5)] == counts
    for (lo, hi), t in zip(case.segs, range(5)):
        mine = items[items[:, 2] == t]
        assert mine[0, 0] * vec == lo and mine[-1, 1] * vec == hi
        assert ((mine[:, 1] - mine[:, 0]) * vec <= 4096).all() and (mine[1:, 0] == mine[:-1, 1]).all()


def test_dots_against_fsum(case):
    from tony_amd.ops.adasum import coef_, dots_

    (biga, ta), (bigb, tb) = case.sides()
    dots_(ta, tb, case.plan)
    coef_(case.plan)
    torch.cuda.synchronize()
    got = _tensor_triples(case.plan)
    coef = case.plan.coef.cpu().numpy()
    for t, ((lo, hi), n) in enumerate(zip(case.segs, R.LENGTHS)):
        exact, mags = R.fsum_triple(case.a[lo:hi], case.b[lo:hi])
        for k in range(3):
            tol = n * 2.0 ** -53 * mags[k]  # the products are exact: only the additions round
            print(f"tensor {t} sum {k}: error {abs(got[t][k] - exact[k]):.3e} tolerance {tol:.3e}")
            assert abs(got[t][k] - exact[k]) <= tol
        for side, nn in ((0, exact[1]), (1, exact[2])):
            c = 1.0 - exact[0] / (2.0 * nn)
            assert abs(float(coef[t, side]) - c) <= 2.0 ** -24 * abs(c) + 1e-12  # formed in double, rounded once
    assert _guards_intact(biga) and _guards_intact(bigb)
    assert np.array_equal(_np(ta), case.a) and np.array_equal(_np(tb), case.b)  # reads only


def test_combine_is_the_contract_bit_for_bit_from_either_side(case):
    from tony_amd.ops.adasum import apply_

    table = np.random.default_rng(4).uniform(0.1, 1.5, size=(5, 2)).astype(np.float32)
    table[0] = (1.0, 1.0)
    want = np.empty_like(case.a)
    for t, (lo, hi) in enumerate(case.segs):
        want[lo:hi] = R.apply_np(case.a[lo:hi], case.b[lo:hi], table[t, 0], table[t, 1], case.bf16)
    case.plan.coef.copy_(torch.from_numpy(table))
    (biga, ta), (bigb, tb) = case.sides()
    apply_(ta, tb, True, case.plan)          # dst is the a side
    torch.cuda.synchronize()
    from_a = _np(ta)
    assert np.array_equal(_np(tb), case.b) and _guards_intact(biga) and _guards_intact(bigb)
    (biga, ta), (bigb, tb) = case.sides()
    apply_(tb, ta, False, case.plan)         # dst is the b side
    torch.cuda.synchronize()
    from_b = _np(tb)
    assert np.array_equal(_np(ta), case.a) and _guards_intact(biga) and _guards_intact(bigb)
    assert np.array_equal(from_a.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(from_b.view(np.uint32), from_a.view(np.uint32))


def test_zero_tensors_take_coefficient_one(case):
    """sqrt(DBL_MIN): a side whose squared norm is below it (for these formats: a zero side) has coefficient 1, not
    1 - 0/0, and the combine returns the other side."""
    from tony_amd.ops.adasum import combine_

    a, b = case.a.copy(), case.b.copy()
    (l0, h0), (l2, h2), (l3, h3) = case.segs[0], case.segs[2], case.segs[3]
    a[l0:h0] = 0          # a zero, b not
    b[l2:h2] = 0          # b zero, a not
    a[l3:h3] = 0          # both zero
    b[l3:h3] = 0
    (biga, ta), (bigb, tb) = _guarded(a, case.dtype, case.dev), _guarded(b, case.dtype, case.dev)
    combine_(ta, tb, True, case.plan)
    torch.cuda.synchronize()
    coef, out = case.plan.coef.cpu().numpy(), _np(ta)
    for t in (0, 2, 3):
        assert coef[t, 0] == 1.0 and coef[t, 1] == 1.0
    assert np.array_equal(out[l0:h0], b[l0:h0]) and np.array_equal(out[l2:h2], a[l2:h2])
    assert not out[l3:h3].any() and not np.signbit(out[l3:h3]).any()
    assert np.isfinite(out).all() and _guards_intact(biga) and _guards_intact(bigb)


def test_whole_pipeline_inside_the_bound_grouping_independent_and_deterministic(case):
    from tony_amd.ops.adasum import AdasumPlan, combine_
    from tony_amd.ops.optim import Segments

    runs = []
    for _ in range(2):
        (biga, ta), (bigb, tb) = case.sides()
        combine_(ta, tb, True, case.plan)
        torch.cuda.synchronize()
        assert _guards_intact(biga) and _guards_intact(bigb) and np.array_equal(_np(tb), case.b)
        runs.append((_np(ta), case.plan.partials.cpu().numpy().copy(), case.plan.coef.cpu().numpy().copy()))
    for x, y in zip(*runs):  # two runs, the same bits: the result, the item triples, the coefficients
        assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64),
                              y.view(np.uint32 if y.dtype == np.float32 else np.uint64))
    got = runs[0][0]
    (bigb, tb), (biga, ta) = _guarded(case.b, case.dtype, case.dev), _guarded(case.a, case.dtype, case.dev)
    combine_(tb, ta, False, case.plan)       # the partner's call: dst is the b side
    torch.cuda.synchronize()
    assert np.array_equal(_np(tb).view(np.uint32), got.view(np.uint32))
    m = R.measured(got, case.ref, case.segs)
    print(f"measured {[round(x, 2) for x in m]} bound K {[round(k, 2) for k in case.ref.K]}; "
          f"{int((got.view(np.uint32) != case.want.view(np.uint32)).sum())} elements differ from the numpy contract")
    assert (np.abs(got.astype(np.float64) - case.ref.val) <= case.ref.bound(case.segs)).all()
    for (lo, hi), n in zip(case.segs, R.LENGTHS):  # the padding stays zero
        assert not got[lo + n:hi].any()
    # every tensor alone, in a buffer of its own: the same bits as in the shared buffer
    for (lo, hi) in case.segs:
        plan = AdasumPlan(Segments.whole(hi - lo), case.dtype, case.dev)
        (biga, ta), (bigb, tb) = _guarded(case.a[lo:hi], case.dtype, case.dev), \
            _guarded(case.b[lo:hi], case.dtype, case.dev)
        combine_(ta, tb, True, plan)
        torch.cuda.synchronize()
        assert np.array_equal(_np(ta).view(np.uint32), got[lo:hi].view(np.uint32)), (lo, hi)
        assert _guards_intact(biga) and _guards_intact(bigb)


def test_native_plan_refuses_misaligned_segments_and_foreign_tensors(cuda):
    from tony_amd.ops.adasum import AdasumPlan, combine_
    from tony_amd.ops.optim import Segments

    with pytest.raises(ValueError):
        AdasumPlan(Segments([0, 4, 16], [0, 1], [True, True]), torch.bfloat16, cuda)  # 4 bf16 are 8 bytes
    plan = AdasumPlan(Segments([0, 4, 16], [0, 1], [True, True]), torch.float32, cuda)
    good = torch.zeros(16, device=cuda)
    for bad in (torch.zeros(16), torch.zeros(20, device=cuda), torch.zeros(16, device=cuda, dtype=torch.bfloat16),
                torch.zeros(32, device=cuda)[::2]):
        with pytest.raises(ValueError):
            combine_(good, bad, True, plan)
    half = AdasumPlan(Segments.whole(16), torch.float16, cuda)  # no kernel for fp16: the torch ops of the contract
    assert not half.native
    x = torch.arange(16, device=cuda, dtype=torch.float16)
    assert torch.equal(combine_(x.clone(), x.clone(), True, half), x)
