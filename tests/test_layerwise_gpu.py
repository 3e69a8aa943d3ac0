"""LARS and LAMB on the GPU (csrc/layerwise.hip): exact per-tensor sums inside poisoned guards and the ratio against
the float64 formula, determinism, bit-identity of a never-adapted FlatLARS to FlatSGD, the kernels against each class's
CPU fallback and against an independent float64 per-tensor loop (tests/layerwise_ref.py) with clipping and the EMA on
and off, the skip, resync, a graph replay and the Horovod wrapper.

Tolerances are the project's two (tests/test_optim_family_gpu.py): FALLBACK kernel vs CPU class over 3 steps,
VS_TORCH GPU vs the float64 loop over 5 steps.
"""
import math
import struct

import pytest
import torch

from layerwise_ref import RefLAMB, RefLARS, segs_of

pytestmark = pytest.mark.gpu

FALLBACK = dict(rtol=1e-5, atol=1e-5)
VS_TORCH = dict(rtol=1e-4, atol=1e-5)
GUARD = 512
SIZES = [64, 64, 4 * (3 * 256 + 1), 8192 * 2 + 64, 4]  # 16448 floats: five work items, the last one partial
ADAPT = [True, False, True, True, False]
N = sum(SIZES)
CLIP = 30.0                # 0.5 * randn(19656) has norm ~70
SCALES = [1.0, 0.2, 1.5, 0.3, 0.8]  # steps 0, 2, 4 clip at 30, steps 1 and 3 do not
LARS_KW = dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True, trust_coef=0.02, eps=1e-9)
LAMB_KW = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-3)
GS = 0.5


def _segments(sizes=SIZES, adapt=ADAPT):
    from tony_amd.ops import Segments

    return Segments(segs_of(sizes)[1], list(range(len(sizes))), list(adapt))


def _make(kind, w, segments=None, **kw):
    from tony_amd.ops import FlatLAMB, FlatLARS

    cls, base = (FlatLARS, LARS_KW) if kind == "lars" else (FlatLAMB, LAMB_KW)
    opt = cls(w, segments=segments or _segments(), **{**base, **kw})
    opt.grad_scale = GS
    return opt


def _ref(kind, w0, sizes=SIZES, adapt=ADAPT, **kw):
    cls, base = (RefLARS, LARS_KW) if kind == "lars" else (RefLAMB, LAMB_KW)
    return cls(w0, segs_of(sizes)[0], adapt, grad_scale=GS, **{**base, **kw})


def _states(opt):
    return [opt.v] if opt.layer_kind == 0 else [opt.m, opt.v]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(a, b, **tol), f"{what}: max abs err {err}"


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _f32_bits(x: float) -> int:
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _ulps(got: float, want: float) -> int:
    """Distance in fp32 units in the last place between two positive finite fp32 values."""
    return abs(_f32_bits(got) - _f32_bits(want))


def _poisoned(cuda, numel, dtype=torch.float32):
    if dtype == torch.float32:
        big = torch.full((numel + 2 * GUARD,), 0x7FC0BEEF, dtype=torch.int32, device=cuda).view(torch.float32)
    else:
        big = torch.full((numel + 2 * GUARD,), 0x7FC5, dtype=torch.int16, device=cuda).view(torch.bfloat16)
    return big, big[GUARD:GUARD + numel]


def _guards_intact(big, before, numel):
    return (torch.equal(_bits(big[:GUARD]), _bits(before[:GUARD])) and
            torch.equal(_bits(big[GUARD + numel:]), _bits(before[GUARD + numel:])))


def _poison_state(cuda, opt):
    """Move w's neighbours -- every state, the EMA, the per-item pairs, tsum and the table -- into poisoned buffers."""
    bigs = {}
    for name in ("v", "m", "ema", "_item_part", "tsum", "table"):
        t = getattr(opt, name, None)
        if t is None:
            continue
        big, view = _poisoned(cuda, t.numel())
        view.copy_(t.reshape(-1))
        setattr(opt, name, view.view(t.shape))
        bigs[name] = (big, t.numel())
    return bigs


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
def test_per_tensor_sums_are_exact_inside_poisoned_guards(cuda, grad_dtype):
    """w and g from {-0.5, 0, 0.5}: every partial sum is a multiple of 0.25 far below 2^24 units, exact in fp32 in
    any order, so tsum must be count/4 exactly for every tensor.  The first and the last float4 of every segment are
    non-zero throughout, so a boundary off by one float4 changes two tensors' sums.  The ratio is rounded once from
    exact sums: within 1 ulp of the float64 formula.  The grid is one workgroup per item and never capped, so there
    is no grid-stride trip; the longest segment spans 17 items and its last item is partial."""
    from tony_amd.ops.optim import ITEM_FLOATS

    sizes = [4, 64, 4 * (3 * 256 + 1), ITEM_FLOATS + 4, 16 * ITEM_FLOATS + 8, 8]
    adapt = [True, True, False, True, True, True]
    segs, starts = segs_of(sizes)
    n = starts[-1]
    g = torch.Generator().manual_seed(5)
    wv = (torch.randint(0, 3, (n,), generator=g).float() - 1.0) * 0.5
    gv = (torch.randint(0, 3, (n,), generator=g).float() - 1.0) * 0.5
    gv[(torch.rand(n, generator=g) < 0.3)] = 0.0  # other counts than w's
    for lo, hi, _ in segs:
        for x in (wv, gv):
            x[lo:lo + 4] = 0.5
            x[hi - 4:hi] = -0.5
    wbig, w = _poisoned(cuda, n)
    w.copy_(wv)
    gbig, grad = _poisoned(cuda, n, grad_dtype)
    grad.copy_(gv)
    opt = _make("lars", w, _segments(sizes, adapt))
    assert opt.w.data_ptr() == w.data_ptr() and opt._items.shape[0] == 1 + 1 + 1 + 2 + 17 + 1
    bigs = _poison_state(cuda, opt)
    before = {k: b.clone() for k, (b, _) in bigs.items()}
    wbefore, gbefore = wbig.clone(), gbig.clone()
    opt.begin_step()
    opt.norm_range(grad, 0)
    opt.fold_norms()
    opt.finish_ratios()
    torch.cuda.synchronize()
    assert torch.equal(_bits(wbig), _bits(wbefore)) and torch.equal(_bits(gbig), _bits(gbefore))  # read only
    for k, (big, numel) in bigs.items():
        assert _guards_intact(big, before[k], numel), k
    assert torch.equal(_bits(bigs["v"][0]), _bits(before["v"]))  # the norm stages do not touch the momentum
    tsum, table = opt.tsum.cpu(), opt.table.cpu()
    counts = []
    for (lo, hi, t), ad in zip(segs, adapt):
        cw, cg = int((wv[lo:hi] != 0).sum()), int((gv[lo:hi] != 0).sum())
        counts.append((cw, cg))
        assert tsum[t, 0].item() == cw / 4 and tsum[t, 1].item() == cg / 4, (t, tsum[t], cw, cg)
        if not ad:
            assert table[t, 0].item() == 1.0 and table[t, 1].item() == 0.0
            continue
        wn, gn = math.sqrt(cw / 4), _f32(GS) * math.sqrt(cg / 4)
        want = _f32(_f32(LARS_KW["trust_coef"]) * wn / (gn + _f32(LARS_KW["weight_decay"]) * wn +
                                                       _f32(LARS_KW["eps"])))
        print(f"tensor {t}: ratio {table[t, 0].item()!r} want {want!r}")
        assert _ulps(table[t, 0].item(), want) <= 1
        assert table[t, 1].item() == _f32(LARS_KW["weight_decay"])
    assert all(a != b for a, b in zip(counts, counts[1:]))  # neighbours differ: a shifted boundary shows
    part = opt._item_part.cpu()
    assert (part * 4 == (part * 4).round()).all() and part.double().sum(0).tolist() == tsum.double().sum(0).tolist()


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_three_runs_give_identical_bits(cuda, kind):
    g = torch.Generator().manual_seed(3)
    w0 = torch.randn(N, generator=g)
    grads = [torch.randn(N, generator=g).to(cuda) for _ in range(2)]
    runs = []
    for _ in range(3):
        opt = _make(kind, w0.to(cuda), clip_norm=CLIP, ema_decay=0.9)
        out = torch.zeros(N, dtype=torch.bfloat16, device=cuda)
        for gr in grads:
            opt.step(gr, out_bf16=out)
        torch.cuda.synchronize()
        runs.append([opt._item_part, opt.tsum, opt.table, opt.w, opt.ema, out] + _states(opt))
    for run in runs[1:]:
        for a, b in zip(run, runs[0]):
            assert torch.equal(_bits(a), _bits(b))
    assert (runs[0][2][:, 0] != 1.0).sum().item() == sum(ADAPT)


@pytest.mark.parametrize("copy", [True, False], ids=["bf16-copy", "no-copy"])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
def test_never_adapted_lars_is_bit_identical_to_sgd(cuda, grad_dtype, copy):
    from tony_amd.ops import FlatLARS, FlatSGD

    g = torch.Generator().manual_seed(17)
    w0 = torch.randn(N, generator=g)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=0.0, nesterov=True, resync=copy)
    a = FlatLARS(w0.to(cuda), segments=_segments(adapt=[False] * len(SIZES)), **kw)
    b = FlatSGD(w0.to(cuda), **kw)
    oa = w0.to(cuda).to(torch.bfloat16) if copy else None
    ob = w0.to(cuda).to(torch.bfloat16) if copy else None
    for opt in (a, b):
        opt.grad_scale = GS
    for _ in range(3):
        gr = torch.randn(N, generator=g).to(grad_dtype).to(cuda)
        a.step(gr, out_bf16=oa)
        b.step(gr, out_bf16=ob)
    torch.cuda.synchronize()
    assert (a.table[:, 0] == 1.0).all() and (a.table[:, 1] == 0.0).all()
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(a.v), _bits(b.v))
    assert not torch.equal(a.w.cpu(), w0)
    if copy:
        assert torch.equal(_bits(oa), _bits(ob))


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "clip-ema"])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_kernels_match_cpu_class_and_float64_loop_inside_poison(cuda, kind, grad_dtype, extras):
    """Everything the kernels write lives inside NaN-patterned buffers.  After 3 steps: the CPU class (FALLBACK);
    after 5: the float64 per-tensor loop (VS_TORCH); all guards and the gradient unchanged."""
    kw = dict(clip_norm=CLIP, ema_decay=0.9) if extras else {}
    g = torch.Generator().manual_seed(29)
    w0 = torch.randn(N, generator=g)
    w0[SIZES[0]:SIZES[0] + SIZES[1]] *= 3.0
    wbig, w = _poisoned(cuda, N)
    w.copy_(w0)
    dev, cpu, ref = _make(kind, w, **kw), _make(kind, w0.clone(), **kw), _ref(kind, w0, **kw)
    bigs = _poison_state(cuda, dev)
    bigs["w"] = (wbig, N)
    obig, out = _poisoned(cuda, N, torch.bfloat16)
    gbig, grad = _poisoned(cuda, N, grad_dtype)
    before = {k: b.clone() for k, (b, _) in bigs.items()}
    obefore = obig.clone()
    clipped = []
    for s in range(5):
        gr = (torch.randn(N, generator=g) * SCALES[s]).to(grad_dtype)
        grad.copy_(gr)
        gbefore = gbig.clone()
        dev.step(grad, out_bf16=out)
        ref.step(gr)
        torch.cuda.synchronize()
        assert torch.equal(_bits(gbig), _bits(gbefore))
        if s < 3:
            cpu.step(gr)
        if extras:
            clipped.append(ref.norm > CLIP)
            assert dev.last_norm() == pytest.approx(ref.norm, rel=1e-6)
        if s == 2:
            _close(dev.w, cpu.w, FALLBACK, f"{kind} w vs CPU class")
            _close(dev.table, cpu.table, FALLBACK, f"{kind} (ratio, wd) vs CPU class")
            for i, (a, b) in enumerate(zip(_states(dev), _states(cpu))):
                _close(a, b, FALLBACK, f"{kind} state {i} vs CPU class")
            if extras:
                _close(dev.ema, cpu.ema, FALLBACK, f"{kind} ema vs CPU class")
    if extras:
        assert clipped == [True, False, True, False, True]
    _close(dev.w, ref.w, VS_TORCH, f"{kind} w vs float64 loop")
    _close(dev.ratios(), torch.tensor(ref.ratios), VS_TORCH, f"{kind} ratios vs float64 loop")
    _close(_states(dev)[-1], ref.v, VS_TORCH, f"{kind} v vs float64 loop")
    if extras:
        _close(dev.ema, ref.ema, VS_TORCH, f"{kind} ema vs float64 loop")
        assert not torch.equal(dev.ema, dev.w)
    ratios = dev.ratios().cpu()
    assert [r != 1.0 for r in ratios.tolist()] == ADAPT
    assert (w0.double() - ref.w).abs().max() > 1e-2  # the steps moved the weights far beyond the tolerance
    assert torch.equal(out, dev.w.to(torch.bfloat16))
    for k, (big, numel) in bigs.items():
        assert _guards_intact(big, before[k], numel), k
    assert _guards_intact(obig, obefore, N)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_range_calls_on_segment_boundaries_equal_one_whole_step(cuda, kind):
    """A sharded caller drives the stages bucket by bucket: the same bits as ``step``."""
    g = torch.Generator().manual_seed(31)
    w0 = torch.randn(N, generator=g)
    a, b = _make(kind, w0.to(cuda), ema_decay=0.9), _make(kind, w0.to(cuda), ema_decay=0.9)
    oa, ob = (torch.zeros(N, dtype=torch.bfloat16, device=cuda) for _ in range(2))
    _, starts = segs_of(SIZES)
    cuts = [0, starts[2], starts[3] + 4096, N]  # a segment boundary and an item boundary inside a segment
    for _ in range(2):
        gr = torch.randn(N, generator=g).to(torch.bfloat16).to(cuda)
        a.step(gr, out_bf16=oa)
        b.begin_step()
        for lo, hi in zip(cuts, cuts[1:]):
            b.norm_range(gr[lo:hi], lo, oa[lo:hi])
        b.fold_norms()
        b.finish_ratios()
        for lo, hi in reversed(list(zip(cuts, cuts[1:]))):
            b.apply_range(gr[lo:hi], lo, ob[lo:hi])
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob))
    assert torch.equal(_bits(a.ema), _bits(b.ema)) and torch.equal(_bits(a.table), _bits(b.table))
    with pytest.raises(ValueError, match="work-item boundaries"):
        b.apply_range(gr[8:72], 8, ob[8:72])


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_nan_gradient_skips_the_step_on_the_device(cuda, kind):
    g = torch.Generator().manual_seed(4)
    opt = _make(kind, torch.randn(N, generator=g).to(cuda), clip_norm=CLIP, skip_nonfinite=True, ema_decay=0.9)
    out = torch.zeros(N, dtype=torch.bfloat16, device=cuda)
    grads = [torch.randn(N, generator=g).to(torch.bfloat16).to(cuda) for _ in range(3)]
    opt.step(grads[0], out_bf16=out)
    tensors = [opt.w, opt.ema, out, opt.table] + _states(opt)
    before = [t.clone() for t in tensors]
    grads[1][2049] = float("nan")
    opt.step(grads[1], out_bf16=out)
    torch.cuda.synchronize()
    assert opt._ctl[1].item() == 1.0 and opt.skipped_steps() == 1
    for a, b in zip(tensors, before):
        assert torch.equal(_bits(a), _bits(b))
    opt.step(grads[2], out_bf16=out)
    assert opt.skipped_steps() == 1 and torch.isfinite(opt.w).all()
    for a, b in zip(tensors, before):
        assert not torch.equal(_bits(a), _bits(b))


def test_resync_enters_the_norm_and_the_update_with_the_copys_value(cuda):
    """Tensor 0 (64 floats) has its bf16 copy overwritten with 3.0 behind the optimizer: sum w^2 is 64 * 9 exactly,
    and the update starts from 3.0 -- as a FlatLARS whose master held 3.0 all along."""
    g = torch.Generator().manual_seed(21)
    w0 = torch.randn(N, generator=g)
    gr = torch.randn(N, generator=g).to(torch.bfloat16).to(cuda)
    a = _make("lars", w0.to(cuda), resync=True)
    oa = w0.to(cuda).to(torch.bfloat16)
    oa[:SIZES[0]] = 3.0
    w1 = w0.clone()
    w1[:SIZES[0]] = 3.0
    b = _make("lars", w1.to(cuda), resync=True)
    ob = w1.to(cuda).to(torch.bfloat16)
    plain = _make("lars", w0.to(cuda), resync=False)
    op = oa.clone()
    a.step(gr, out_bf16=oa)
    b.step(gr, out_bf16=ob)
    plain.step(gr, out_bf16=op)
    torch.cuda.synchronize()
    assert a.tsum[0, 0].item() == 64 * 9.0 and plain.tsum[0, 0].item() != 64 * 9.0
    assert torch.equal(_bits(a.table), _bits(b.table))
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob))
    assert (a.w[:SIZES[0]] - 3.0).abs().max() < 0.5 and (plain.w[:SIZES[0]] - w0[:SIZES[0]].to(cuda)).abs().max() < 0.5


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_graph_replay_takes_a_new_gradient_and_a_new_lr(cuda, kind):
    g = torch.Generator().manual_seed(9)
    w0 = torch.randn(N, generator=g)
    kw = dict(clip_norm=CLIP, ema_decay=0.9)
    _make(kind, w0.to(cuda), **kw).step(torch.randn(N, generator=g).to(cuda))  # every kernel has run once
    dev, eager = _make(kind, w0.to(cuda), **kw), _make(kind, w0.to(cuda), **kw)
    dev.partials(1)
    static_g = torch.zeros(N, dtype=torch.float32, device=cuda)
    out = torch.zeros(N, dtype=torch.bfloat16, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.accumulate_sumsq(static_g, 0)
        dev.finish_norm(1)
        dev.norm_range(static_g, 0, out)
        dev.fold_norms()
        dev.finish_ratios()
        dev.apply_range(static_g, 0, out_bf16=out)
    if kind == "lamb":  # the captured launches are not run, but make sure of it: the moments are still zero
        assert not dev.m.any()
    for scale, lr in ((0.2, 0.05), (1.5, 0.01), (1.0, 0.03)):
        gr = (torch.randn(N, generator=g) * scale).to(cuda)
        static_g.copy_(gr)
        dev.lr = eager.lr = lr
        dev.begin_step()  # the hyper-parameters of this replay (as Trainer._refresh_hp does)
        graph.replay()
        eager.step(gr)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dev.w), _bits(eager.w)) and torch.equal(_bits(dev.table), _bits(eager.table))
    assert torch.equal(_bits(dev.ema), _bits(eager.ema)) and torch.equal(out, dev.w.to(torch.bfloat16))
    cpu = _make(kind, w0.clone(), **kw)
    assert not torch.equal(dev.w.cpu(), cpu.w)


def _two_linear(seed, dev, dtype):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16)).to(dev).to(dtype)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_hvd_fused_layerwise_follows_the_float64_loop(cuda, kind, monkeypatch):
    """One rank: ``lars_coef`` on a bf16 model (fp32 master, resync) and ``lamb`` on an fp32 model.  The float64 loop
    is fed the gradients the model produced, per parameter tensor; biases are not adapted."""
    import tony_amd.hvd as hvd
    from tony_amd.ops import FlatLAMB, FlatLARS

    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    hvd.init()
    try:
        g = torch.Generator(device=cuda).manual_seed(1)
        dtype = torch.bfloat16 if kind == "lars" else torch.float32
        x = torch.randn((8, 64), generator=g, device=cuda).to(dtype)
        y = torch.randint(0, 16, (8,), generator=g, device=cuda)
        model = _two_linear(0, cuda, dtype)
        if kind == "lars":
            base = torch.optim.SGD(model.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-3, nesterov=True)
            fused = hvd.DistributedOptimizer(base, named_parameters=model.named_parameters(), fused=True,
                                             lars_coef=0.02)
        else:
            base = torch.optim.AdamW(model.parameters(), lr=0.02, eps=1e-6, weight_decay=1e-2)
            fused = hvd.DistributedOptimizer(base, named_parameters=model.named_parameters(), fused=True, lamb=True)
        flat, opt = fused._fused[0]
        assert isinstance(opt, FlatLARS if kind == "lars" else FlatLAMB) and len(fused._fused) == 1
        assert opt.segments.adapt == [True, False, True, False]
        segs = [(s.offset, nxt, i) for i, (s, nxt) in enumerate(
            zip(flat.slots, [t.offset for t in flat.slots[1:]] + [flat.numel]))]
        if kind == "lars":
            assert opt.resync and opt.w.data_ptr() != flat.data.data_ptr()
            ref = RefLARS(opt.w, segs, opt.segments.adapt, lr=0.5, momentum=0.9, weight_decay=1e-3, nesterov=True,
                          trust_coef=0.02)
        else:
            assert opt.w.data_ptr() == flat.data.data_ptr()
            ref = RefLAMB(opt.w, segs, opt.segments.adapt, lr=0.02, eps=1e-6, weight_decay=1e-2)
        w0 = opt.w.clone()
        for step in range(5):
            fused.zero_grad()
            torch.nn.functional.cross_entropy(model(x).float(), y).backward()
            if step == 3:
                base.param_groups[0]["lr"] *= 0.5  # a schedule edits the wrapped optimizer's group
                ref.lr *= 0.5
            ref.step(flat.grad)
            fused.step()
        torch.cuda.synchronize()
        _close(opt.w, ref.w, VS_TORCH, f"hvd {kind} masters vs float64 loop")
        _close(opt.ratios(), torch.tensor(ref.ratios), VS_TORCH, f"hvd {kind} ratios")
        assert (opt.w - w0).abs().max() > 1e-2
        assert torch.equal(flat.data, opt.w.to(dtype))
        sd = fused.state_dict()
        key = "momentum_buffer" if kind == "lars" else "exp_avg"
        assert torch.equal(sd["state"][0][key].reshape(-1), flat.slots[0].view(_states(opt)[0]).reshape(-1))
        fused.load_state_dict(sd)
        assert torch.equal(sd["state"][2][key].reshape(-1), flat.slots[2].view(_states(opt)[0]).reshape(-1))
    finally:
        hvd.shutdown()
