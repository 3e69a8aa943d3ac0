"""Global-norm clipping, non-finite skip and EMA on the GPU (csrc/optim.hip tony_grad_sumsq / tony_clip_ctl /
tony_optim_apply_x): an exact sum of squares inside poisoned guards, its determinism, the coefficient against the
float64 formula, bit-identity of the new apply to the existing kernels when nothing clips, the kernels against
each class's CPU fallback (poisoned surroundings included), the skip, a graph replay that reads the coefficient on
the device, the single-rank ParameterServer with ``ema_weights()`` and the Horovod wrapper.

Tolerances are the project's two (tests/test_optim_family_gpu.py): FALLBACK kernel vs CPU class over 3 steps,
VS_TORCH GPU vs torch.optim over 5 steps.
"""
import math
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

FALLBACK = dict(rtol=1e-5, atol=1e-5)
VS_TORCH = dict(rtol=1e-4, atol=1e-5)
N_SMALL = 4 * (3 * 256 + 1)      # several workgroups, the last one partial; most of the fixed grid has no element
N_TRIP = 4 * (8192 * 256 + 3)    # grid_for's cap: a second grid-stride trip of the apply, many of the sum's
GUARD = 512
CLIP = 30.0                      # randn(3076) has norm ~55
SCALES = [1.0, 0.2, 1.5]         # steps 0 and 2 clip at 30, step 1 does not
KINDS = ["sgd", "adam", "adamw", "adagrad", "rmsprop", "rmsprop_tf"]


def _make(kind, w, **kw):
    from tony_amd.ops import FlatAdagrad, FlatAdam, FlatRMSProp, FlatSGD

    if kind == "sgd":
        return FlatSGD(w, lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True, **kw)
    if kind in ("adam", "adamw"):
        return FlatAdam(w, lr=1e-2, weight_decay=1e-2, decoupled=(kind == "adamw"), **kw)
    if kind == "adagrad":
        return FlatAdagrad(w, lr=0.05, eps=1e-5, weight_decay=1e-3, **kw)
    tf = kind == "rmsprop_tf"
    return FlatRMSProp(w, lr=0.05, alpha=0.9, momentum=0.9, eps=1.0 if tf else 1e-8, weight_decay=1e-3, tf_style=tf,
                       **kw)


def _states(opt):
    return [t for t in opt.plane_state()[1:] if t is not None]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(a, b, **tol), f"{what}: max abs err {err}"


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


def _norm_launches(cuda, grad, xhp_vals, n_blocks=1, partials=None, ctl=None):
    """tony_grad_sumsq into block 0 (unless ``partials`` is given ready-made) + tony_clip_ctl: (partials, ctl)."""
    from tony_amd.ops import _lib
    from tony_amd.ops.optim import N_XHP, SUMSQ_BLOCKS

    L, st = _lib.lib(), _lib.stream_ptr(cuda)
    assert L.tony_grad_sumsq_blocks() == SUMSQ_BLOCKS
    if partials is None:
        partials = torch.zeros(n_blocks * SUMSQ_BLOCKS, dtype=torch.float32, device=cuda)
        _lib.check(L.tony_grad_sumsq(grad.data_ptr(), int(grad.dtype == torch.bfloat16), grad.numel(),
                                     partials.data_ptr(), st), "tony_grad_sumsq")
    xhp = torch.tensor(list(xhp_vals) + [0.0] * (N_XHP - len(xhp_vals)), dtype=torch.float32, device=cuda)
    if ctl is None:
        ctl = torch.zeros(4, dtype=torch.float32, device=cuda)
    _lib.check(L.tony_clip_ctl(partials.data_ptr(), partials.numel(), xhp.data_ptr(), ctl.data_ptr(), st),
               "tony_clip_ctl")
    torch.cuda.synchronize()
    return partials, ctl


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
@pytest.mark.parametrize("n", [N_SMALL, N_TRIP], ids=["small", "trip"])
def test_sum_of_squares_is_exact_inside_poisoned_guards(cuda, n, grad_dtype):
    """Elements from {-0.5, 0, 0.5}: every partial sum is a multiple of 0.25 below 2^24 units, exact in fp32 in any
    order, so the partials must add up to count/4 exactly and the norm be sqrt(count/4) to the last place."""
    from tony_amd.ops import _lib
    from tony_amd.ops.optim import SUMSQ_BLOCKS

    g = torch.Generator().manual_seed(n % 997)
    vals = (torch.randint(0, 3, (n,), generator=g).float() - 1.0) * 0.5
    count = int((vals != 0).sum())
    gbig, grad = _poisoned(cuda, n, grad_dtype)
    grad.copy_(vals)
    pbig, part = _poisoned(cuda, SUMSQ_BLOCKS)
    gbefore, pbefore = gbig.clone(), pbig.clone()
    L = _lib.lib()
    _lib.check(L.tony_grad_sumsq(grad.data_ptr(), int(grad_dtype == torch.bfloat16), n, part.data_ptr(),
                                 _lib.stream_ptr(cuda)), "tony_grad_sumsq")
    _, ctl = _norm_launches(cuda, None, [0.0, 1.0, 0.0], partials=part)
    assert torch.equal(_bits(gbig), _bits(gbefore))  # the gradient and its guards: read only
    assert torch.equal(_bits(pbig[:GUARD]), _bits(pbefore[:GUARD]))
    assert torch.equal(_bits(pbig[GUARD + SUMSQ_BLOCKS:]), _bits(pbefore[GUARD + SUMSQ_BLOCKS:]))
    p = part.cpu()
    assert torch.isfinite(p).all() and p.double().sum().item() == count / 4
    assert (p * 4 == (p * 4).round()).all()
    if n == N_SMALL:  # 769 float4 groups: workgroups 4.. of the fixed grid have no element and store their 0
        assert (p[4:] == 0).all() and (p[:3] > 0).all()
    want = struct.unpack("<f", struct.pack("<f", math.sqrt(count / 4)))[0]
    got = ctl[2].item()
    print(f"norm {got!r} want {want!r}")
    assert _ulps(got, want) <= 1
    assert ctl[0].item() == 1.0 and ctl[1].item() == 0.0 and ctl[3].item() == 0.0
    assert L.tony_grad_sumsq(grad.data_ptr(), 0, 6, part.data_ptr(), _lib.stream_ptr(cuda)) == -1  # n % 4 != 0


def test_sum_of_squares_is_deterministic(cuda):
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(N_TRIP, generator=g).to(cuda)
    runs = [_norm_launches(cuda, grad, [1.0, 0.5, 1.0]) for _ in range(3)]
    for part, ctl in runs[1:]:
        assert torch.equal(_bits(part), _bits(runs[0][0])) and torch.equal(_bits(ctl), _bits(runs[0][1]))
    norm = runs[0][1][2].item()
    assert norm == pytest.approx(0.5 * grad.double().norm().item(), rel=1e-5)


@pytest.mark.parametrize("blocks", [1, 3], ids=["one-bucket", "three-buckets"])
def test_coefficient_matches_the_float64_formula(cuda, blocks):
    """coef = clip / max(gs * sqrt(S), clip): three correctly rounded fp32 operations at most (4 ulp), exactly 1
    when nothing clips; S is the sum over every bucket's partial block."""
    from tony_amd.ops.optim import SUMSQ_BLOCKS

    clip, gs = 2.0, 0.5
    g = torch.Generator().manual_seed(blocks)
    base = torch.rand(blocks * SUMSQ_BLOCKS, generator=g)
    seen = set()
    for target in (0.25, 1.9999, 2.0001, 3.0, 1e3, 1e-3):  # norms on both sides of clip
        part = (base * (target / gs) ** 2 / base.double().sum().item()).float()
        S = part.double().sum().item()
        norm64 = struct.unpack("<f", struct.pack("<f", gs))[0] * math.sqrt(S)
        coef64 = clip / max(norm64, clip)
        _, ctl = _norm_launches(cuda, None, [clip, gs, 0.0], partials=part.to(cuda))
        coef, norm = ctl[0].item(), ctl[2].item()
        print(f"target {target}: norm {norm!r} coef {coef!r} (float64 {coef64!r})")
        assert _ulps(norm, struct.unpack("<f", struct.pack("<f", norm64))[0]) <= 1
        assert _ulps(coef, struct.unpack("<f", struct.pack("<f", coef64))[0]) <= 4
        if norm <= clip:
            assert coef == 1.0
        else:
            assert coef < 1.0
        seen.add(coef == 1.0)
    assert seen == {True, False}
    # clip_norm 0: no clipping at all
    _, ctl = _norm_launches(cuda, None, [0.0, gs, 0.0], partials=(base * 1e6).to(cuda))
    assert ctl[0].item() == 1.0


def _run_pair(cuda, kind, n, steps, grad_dtype, **kw):
    """The optimizer with ``kw`` and the default one (existing kernels) from the same start, same gradients."""
    g = torch.Generator().manual_seed(n % 1000 + 7)
    w0 = torch.randn(n, generator=g)
    a, b = _make(kind, w0.to(cuda), **kw), _make(kind, w0.to(cuda))
    oa = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    ob = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    for _ in range(steps):
        gr = torch.randn(n, generator=g).to(grad_dtype).to(cuda)
        a.step(gr, out_bf16=oa)
        b.step(gr, out_bf16=ob)
    torch.cuda.synchronize()
    return a, b, oa, ob


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_apply_x_is_bit_identical_to_the_existing_kernels_when_nothing_clips(cuda, kind, grad_dtype):
    a, b, oa, ob = _run_pair(cuda, kind, N_SMALL, 2, grad_dtype, clip_norm=1e30, skip_nonfinite=True)
    assert a._ctl[0].item() == 1.0 and a.last_norm() > 10.0
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob))
    for sa, sb in zip(_states(a), _states(b)):
        assert torch.equal(_bits(sa), _bits(sb))


def test_apply_x_is_bit_identical_on_the_second_grid_stride_trip(cuda):
    a, b, oa, ob = _run_pair(cuda, "rmsprop_tf", N_TRIP, 1, torch.bfloat16, clip_norm=1e30)
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob))
    for sa, sb in zip(_states(a), _states(b)):
        assert torch.equal(_bits(sa), _bits(sb))


@pytest.mark.parametrize("kind", ["sgd", "rmsprop_tf"])
def test_ema_alone_leaves_the_update_bit_identical(cuda, kind):
    """``ema_decay`` only: no norm launches, ctl is not read, the update itself is the existing kernel's."""
    a, b, oa, ob = _run_pair(cuda, kind, N_SMALL, 2, torch.bfloat16, ema_decay=0.9)
    assert a._partials is None
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob))
    assert not torch.equal(a.ema, a.w) and torch.isfinite(a.ema).all()


def test_sgd_resync_survives_in_apply_x(cuda):
    """Elements of the bf16 copy overwritten behind the optimizer re-seed the master, as in tony_sgd_step."""
    from tony_amd.ops import FlatSGD

    n = N_SMALL
    g = torch.Generator().manual_seed(21)
    w0 = torch.randn(n, generator=g).to(cuda)
    gr = torch.randn(n, generator=g).to(torch.bfloat16).to(cuda)
    a = FlatSGD(w0.clone(), 0.05, resync=True, clip_norm=1e30)
    b = FlatSGD(w0.clone(), 0.05, resync=True)
    oa, ob = w0.to(torch.bfloat16), w0.to(torch.bfloat16)
    for o in (oa, ob):
        o[5:100] = 3.0
    a.step(gr, out_bf16=oa)
    b.step(gr, out_bf16=ob)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.w), _bits(b.w)) and torch.equal(_bits(oa), _bits(ob)) and torch.equal(a.v, b.v)
    assert (a.w[5:100] - 3.0).abs().max() < 0.5 and (a.w[5:100] - w0[5:100]).abs().max() > 1.0


def _versus_fallback(cuda, kind, grad_dtype, n, steps=3, **kw):
    g = torch.Generator().manual_seed(n % 1000 + steps)
    w0 = torch.randn(n, generator=g)
    dev, ref = _make(kind, w0.to(cuda), **kw), _make(kind, w0.clone(), **kw)
    out = torch.empty(n, dtype=torch.bfloat16, device=cuda)
    clipped = []
    for s in range(steps):
        gr = (torch.randn(n, generator=g) * SCALES[s % 3]).to(grad_dtype)
        dev.step(gr.to(cuda), out_bf16=out)
        ref.step(gr)
        assert dev.last_norm() == pytest.approx(ref.last_norm(), rel=1e-6)
        clipped.append(ref.last_norm() > CLIP)
    assert any(clipped) and not all(clipped)
    _close(dev.w, ref.w, FALLBACK, f"{kind} w")
    _close(dev.ema, ref.ema, FALLBACK, f"{kind} ema")
    for i, (a, b) in enumerate(zip(_states(dev), _states(ref))):
        _close(a, b, FALLBACK, f"{kind} state {i}")
    assert torch.equal(out, dev.w.to(torch.bfloat16))
    assert not torch.equal(dev.ema, dev.w)


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_clipped_ema_kernel_matches_cpu_fallback(cuda, kind, grad_dtype):
    _versus_fallback(cuda, kind, grad_dtype, N_SMALL, clip_norm=CLIP, ema_decay=0.9, ema_warmup=(kind == "adam"))


@pytest.mark.parametrize("kind", ["sgd", "adam", "adagrad", "rmsprop_tf"])
def test_range_apply_leaves_poisoned_surroundings_untouched(cuda, kind):
    """w, the states, the EMA and the bf16 copy live inside larger NaN-patterned buffers; a clipped range update of
    [1024, 1024 + 3076) of the 8192-element shard changes nothing else, guards included, nor the gradient."""
    shard, lo, n = 8192, 1024, N_SMALL
    g = torch.Generator().manual_seed(11)
    wbig, w = _poisoned(cuda, shard)
    w.copy_(torch.randn(shard, generator=g))
    opt = _make(kind, w, clip_norm=CLIP, ema_decay=0.9)
    assert opt.w.data_ptr() == w.data_ptr()
    bigs = [wbig]
    for name in ("v", "m", "h", "ms", "mom", "ema"):
        if hasattr(opt, name):
            sbig, s = _poisoned(cuda, shard)
            s.copy_(getattr(opt, name))
            setattr(opt, name, s)
            bigs.append(sbig)
    assert len(bigs) == 2 + len(_states(opt))
    obig, out_full = _poisoned(cuda, shard, torch.bfloat16)
    out = out_full[lo:lo + n]
    bigs.append(obig)
    gbig, grad = _poisoned(cuda, n, torch.bfloat16)
    grad.copy_(torch.randn(n, generator=g))
    before = [b.clone() for b in bigs]
    gbefore = gbig.clone()
    opt.begin_step()
    opt.accumulate_sumsq(grad, 0)
    opt.finish_norm(1)
    opt.apply_range(grad, lo, out_bf16=out)
    torch.cuda.synchronize()
    assert opt.last_norm() > CLIP
    for b, a in zip(before, bigs):
        a0, a1 = GUARD + lo, GUARD + lo + n
        assert torch.equal(_bits(a[:a0]), _bits(b[:a0])) and torch.equal(_bits(a[a1:]), _bits(b[a1:]))
        assert torch.isfinite(a[a0:a1].float()).all() and not torch.equal(_bits(a[a0:a1]), _bits(b[a0:a1]))
    assert torch.equal(_bits(gbig), _bits(gbefore))
    assert torch.equal(out, opt.w[lo:lo + n].to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["sgd", "adam", "rmsprop_tf"])
def test_inf_gradient_skips_the_step_on_the_device(cuda, kind):
    n = N_SMALL
    g = torch.Generator().manual_seed(4)
    opt = _make(kind, torch.randn(n, generator=g).to(cuda), clip_norm=CLIP, skip_nonfinite=True, ema_decay=0.9)
    out = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    grads = [torch.randn(n, generator=g).to(torch.bfloat16).to(cuda) for _ in range(3)]
    opt.step(grads[0], out_bf16=out)
    tensors = [opt.w, opt.ema, out] + _states(opt)
    before = [t.clone() for t in tensors]
    grads[1][2049] = float("inf")
    opt.step(grads[1], out_bf16=out)
    torch.cuda.synchronize()
    assert opt._ctl[3].item() == 1.0 and opt._ctl[1].item() == 1.0 and opt.skipped_steps() == 1
    for a, b in zip(tensors, before):
        assert torch.equal(_bits(a), _bits(b))
    opt.step(grads[2], out_bf16=out)
    assert opt.skipped_steps() == 1 and torch.isfinite(opt.w).all()
    for a, b in zip(tensors, before):
        assert not torch.equal(_bits(a), _bits(b))


def test_graph_replay_reads_the_coefficient_on_the_device(cuda):
    """sumsq -> ctl -> apply captured on one stream; the first replay sees a small gradient (no clipping), the
    second a large one (clipped): both follow the CPU fallback, so the coefficient is not baked into the graph."""
    n, kind = N_SMALL, "rmsprop_tf"
    g = torch.Generator().manual_seed(9)
    w0 = torch.randn(n, generator=g)
    kw = dict(clip_norm=CLIP, ema_decay=0.9)
    _make(kind, w0.to(cuda), **kw).step(torch.randn(n, generator=g).to(cuda))  # the three kernels have run once
    dev, ref = _make(kind, w0.to(cuda), **kw), _make(kind, w0.clone(), **kw)
    dev.partials(1)
    static_g = torch.zeros(n, dtype=torch.float32, device=cuda)
    out = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.accumulate_sumsq(static_g, 0)
        dev.finish_norm(1)
        dev.apply_range(static_g, 0, out_bf16=out)
    coefs = []
    for scale in (0.2, 1.5):
        gr = torch.randn(n, generator=g) * scale
        static_g.copy_(gr.to(cuda))
        dev.begin_step()  # the hyper-parameters of this replay (as Trainer._refresh_hp does)
        graph.replay()
        torch.cuda.synchronize()
        ref.step(gr)
        coefs.append(dev._ctl[0].item())
        assert dev.last_norm() == pytest.approx(ref.last_norm(), rel=1e-6)
        _close(dev.w, ref.w, FALLBACK, f"replay with gradient scale {scale}")
    assert coefs[0] == 1.0 and coefs[1] < 0.6
    _close(dev.ema, ref.ema, FALLBACK, "ema after two replays")
    assert torch.equal(out, dev.w.to(torch.bfloat16))


class _Net(torch.nn.Module):
    def __init__(self, sizes=(11000, 12000, 4136, 13000, 3000, 11008, 64)):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in sizes])


@pytest.mark.parametrize("bucketed", [False, True], ids=["one-apply", "bucketed"])
def test_single_rank_parameter_server_clips_and_swaps_the_ema(cuda, bucketed):
    from tony_amd.parallel.ps import ParameterServer, make_optimizer

    torch.manual_seed(0)
    net = _Net()
    with torch.no_grad():
        for p in net.ps:
            p.copy_(torch.randn(p.shape).mul_(0.5))
    ps = ParameterServer(net, optimizer="rmsprop_tf", lr=0.05, momentum=0.9, weight_decay=1e-3, dtype=torch.bfloat16,
                         device=cuda, clip_norm=2.0, ema_decay=0.99, bucketed_single=bucketed, bucket_mb=0.02)
    assert ps.single != bucketed
    n = ps.flat.numel
    opt = ps.optimizers[0]
    ref = make_optimizer("rmsprop_tf", opt.w.cpu().clone(), 0.05, 0.9, 1e-3, clip_norm=2.0, ema_decay=0.99)
    idx = torch.arange(n, dtype=torch.float32)
    clipped = []
    for s in range(3):
        # multiples of 1/8 (exact in bf16) over 54208 elements: norm above 100; x 2^-8 at step 1, below 2 there
        gr = (float(s % 3 + 1) * 0.25 + idx.remainder(4) * 0.125) * (2.0 ** -8 if s == 1 else 1.0)
        ps.zero_grad()
        ps.flat.grad.copy_(gr.to(cuda))
        ps.step()
        ref.step(gr)
        clipped.append(ref.last_norm() > 2.0)
        assert opt.last_norm() == pytest.approx(ref.last_norm(), rel=1e-6)
    torch.cuda.synchronize()
    assert clipped == [True, False, True]
    # masters in bucket order (bucketed) or flat order (one apply): the reference is in flat order
    master = torch.zeros(n)
    for b in ps.buckets:
        m, k = ps._master_range[b.index]
        master[b.lo:b.hi] = opt.w[m:m + k].cpu()
    _close(master, ref.w, FALLBACK, "rmsprop_tf PS masters")
    before = ps.flat.data.clone()
    assert torch.equal(before.cpu(), master.to(torch.bfloat16))
    ema = torch.zeros(n)
    for b in ps.buckets:
        m, k = ps._master_range[b.index]
        ema[b.lo:b.hi] = opt.ema[m:m + k].cpu()
    _close(ema, ref.ema, FALLBACK, "rmsprop_tf PS ema")
    with ps.ema_weights():
        assert torch.equal(ps.flat.data.cpu(), ema.to(torch.bfloat16))
        assert not torch.equal(ps.flat.data, before)
        s0, p0 = ps.flat.slots[0], ps.flat.params[0]  # the model's parameters are views: they hold the EMA now
        assert torch.equal(p0.detach().reshape(-1).cpu(), ema[s0.offset:s0.offset + p0.numel()].to(torch.bfloat16))
    assert torch.equal(_bits(ps.flat.data), _bits(before))


def _two_linear(seed, dev):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16)).to(dev)


HVD_CASES = {
    "sgd": (torch.optim.SGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
    "adam": (torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-2)),
    "adamw": (torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2)),
    "adagrad": (torch.optim.Adagrad, dict(lr=0.05, eps=1e-5, initial_accumulator_value=0.1)),
    "rmsprop": (torch.optim.RMSprop, dict(lr=1e-2, momentum=0.9, weight_decay=1e-2)),
}


@pytest.mark.parametrize("name", list(HVD_CASES))
def test_hvd_fused_clip_norm_matches_clip_grad_norm_and_torch(cuda, name, monkeypatch):
    import tony_amd.hvd as hvd

    cls, kw = HVD_CASES[name]
    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    hvd.init()
    try:
        g = torch.Generator(device=cuda).manual_seed(1)
        x = torch.randn((8, 64), generator=g, device=cuda)
        y = torch.randint(0, 16, (8,), generator=g, device=cuda)

        def flat(model):
            return torch.cat([p.detach().reshape(-1) for p in model.parameters()])

        fm, rm, um = _two_linear(0, cuda), _two_linear(0, cuda), _two_linear(0, cuda)
        # the threshold comes from the reference model alone: 0.6 x its first gradient's norm
        torch.nn.functional.cross_entropy(rm(x), y).backward()
        clip = 0.6 * torch.cat([p.grad.reshape(-1) for p in rm.parameters()]).norm().item()
        fused = hvd.DistributedOptimizer(cls(fm.parameters(), **kw), named_parameters=fm.named_parameters(),
                                         fused=True, clip_norm=clip)
        assert fused._fused and fused._clip
        ref, unclipped = cls(rm.parameters(), **kw), cls(um.parameters(), **kw)
        norms = []
        for _ in range(5):
            fused.zero_grad()
            torch.nn.functional.cross_entropy(fm(x), y).backward()
            fused.step()
            norms.append(fused._fused[0][1].last_norm())
            ref.zero_grad()
            torch.nn.functional.cross_entropy(rm(x), y).backward()
            tn = torch.nn.utils.clip_grad_norm_(rm.parameters(), clip).item()
            ref.step()
            assert norms[-1] == pytest.approx(tn, rel=1e-4)
            unclipped.zero_grad()
            torch.nn.functional.cross_entropy(um(x), y).backward()
            unclipped.step()
        print(f"hvd {name}: clip {clip:.4f}, norms {norms}")
        assert norms[0] > clip
        _close(flat(fm), flat(rm), VS_TORCH, f"hvd fused {name} with clip_norm, 5 steps")
        if name == "sgd":  # the adaptive kinds' normalised steps hide most of a rescaled gradient
            assert not torch.allclose(flat(um), flat(rm), **VS_TORCH)
    finally:
        hvd.shutdown()
