"""LARS and LAMB (ops/optim.py FlatLARS / FlatLAMB) without a GPU: the segment table of a master shard, the CPU
fallbacks against an independent float64 per-tensor loop (tests/layerwise_ref.py), the ratio's corner cases, the
untouched defaults, checkpoints, what the Horovod wrapper and the parameter server refuse, the warm-up schedule and
the colocated PS over two gloo ranks, where piece boundaries cut parameter tensors.

Tolerances are the project's two (tests/test_optim_family_gpu.py); the CPU classes are compared with the float64 loop
under VS_TORCH over 5 steps.
"""
import multiprocessing as mp
import socket

import pytest
import torch

from layerwise_ref import RefLAMB, RefLARS, segs_of

VS_TORCH = dict(rtol=1e-4, atol=1e-5)
SIZES = [64, 64, 4 * (3 * 256 + 1), 8192 * 2 + 64, 4]
ADAPT = [True, False, True, True, False]
N = sum(SIZES)
LARS_KW = dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=False, trust_coef=0.02)
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


def _close(a, b, tol, what):
    err = (a.double() - b.double()).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(a.double(), b.double(), **tol), f"{what}: max abs err {err}"


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 10, 3)          # weight 270 (slot 320), bias 10
        self.bn = torch.nn.BatchNorm2d(10)             # scale, shift: 10 each
        self.fc = torch.nn.Linear(25, 20)              # weight 500 (slot 512), bias 20


def _toy_flat(world):
    from tony_amd.parallel.flat import FlatParams

    torch.manual_seed(0)
    return FlatParams(_Toy(), dtype=torch.float32, world=world, align=64)


def _check_cover(seg, n):
    seg.validate(n)
    assert seg.starts[0] == 0 and seg.starts[-1] == n and all(a % 4 == 0 for a in seg.starts)
    assert all(b > a for a, b in zip(seg.starts, seg.starts[1:]))


def test_segments_of_the_whole_buffer_and_the_default_rule():
    from tony_amd.parallel.flat import build_segments

    f = _toy_flat(1)
    seg = build_segments(f, [(0, f.numel)])
    _check_cover(seg, f.numel)
    assert [s.name for s in f.slots] == ["conv.weight", "conv.bias", "bn.weight", "bn.bias", "fc.weight", "fc.bias"]
    assert seg.tensor == [0, 1, 2, 3, 4, 5] and seg.names == [s.name for s in f.slots]
    assert seg.adapt == [True, False, False, False, True, False]  # ndim <= 1: not adapted
    # a slot's padding (and the buffer's tail) belongs to the slot before it
    assert seg.starts == [s.offset for s in f.slots] + [f.numel]
    assert seg.starts[1] - seg.starts[0] == 320 and f.slots[0].numel == 270
    assert not f.data[270:320].any() and not f.grad[270:320].any()
    only_bn = build_segments(f, [(0, f.numel)], adapt_filter=lambda name, p: name.startswith("bn."))
    assert only_bn.adapt == [False, False, True, True, False, False]
    for bad in ([(0, 6)], [(8, 8)], [(0, f.numel + 4)]):
        with pytest.raises(ValueError, match="master range"):
            build_segments(f, bad)


@pytest.mark.parametrize("world", [1, 2])
def test_segments_of_colocated_pieces_cut_tensors_and_keep_their_ids(world):
    """Rank r owns the r-th piece of every bucket: the pieces of all ranks cover every flat element once, and a
    tensor cut by a piece boundary has segments with one id on two ranks."""
    from tony_amd.parallel.buckets import make_buckets
    from tony_amd.parallel.flat import FlatParams, build_segments

    torch.manual_seed(0)
    f = FlatParams(_Toy(), dtype=torch.float32, world=world, align=64)
    buckets = make_buckets(f, 0.0002, multiple=8 * world)  # 52 floats: a bucket per tensor
    assert len(buckets) >= 3
    seen = torch.zeros(f.numel, dtype=torch.int32)
    ids_by_rank = []
    for r in range(world):
        ranges = [(b.lo + r * (b.numel // world), b.lo + (r + 1) * (b.numel // world))
                  for b in sorted(buckets, key=lambda b: b.lo)]
        seg = build_segments(f, ranges)
        _check_cover(seg, f.numel // world)
        ids_by_rank.append(set(seg.tensor))
        m = 0
        for lo, hi in ranges:  # every range begins a segment; inside it the segments follow the slots
            assert m in seg.starts
            k = seg.starts.index(m)
            pos = lo
            while pos < hi:
                t = seg.tensor[k]
                slot_end = f.slots[t + 1].offset if t + 1 < len(f.slots) else f.numel
                assert f.slots[t].offset <= pos < slot_end
                length = seg.starts[k + 1] - seg.starts[k]
                assert pos + length <= min(hi, slot_end)
                seen[pos:pos + length] += 1
                pos, k = pos + length, k + 1
            m += hi - lo
    assert (seen == 1).all()
    if world == 2:
        assert ids_by_rank[0] & ids_by_rank[1]  # some tensor lies on both ranks


def test_segments_of_dedicated_ownership():
    """Two ps tasks own the buckets round-robin: each owner's table holds whole tensors, every tensor once."""
    from tony_amd.parallel.buckets import make_buckets
    from tony_amd.parallel.flat import build_segments

    f = _toy_flat(1)
    buckets = make_buckets(f, 0.0002)
    owned = [[(b.lo, b.hi) for b in buckets if b.index % 2 == o] for o in range(2)]
    segs = [build_segments(f, r) for r in owned]
    for seg, r in zip(segs, owned):
        _check_cover(seg, sum(hi - lo for lo, hi in r))
    assert sorted(segs[0].tensor + segs[1].tensor) == list(range(len(f.slots)))
    assert segs[0].adapt == segs[1].adapt


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "clip-ema"])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_cpu_fallback_follows_the_float64_loop(kind, extras):
    kw = dict(clip_norm=30.0, ema_decay=0.9) if extras else {}
    g = torch.Generator().manual_seed(0)
    w0 = torch.randn(N, generator=g)
    opt, ref = _make(kind, w0.clone(), **kw), _ref(kind, w0, **kw)
    out = torch.zeros(N, dtype=torch.bfloat16)
    clipped = []
    for s in range(5):
        gr = torch.randn(N, generator=g) * [1.0, 0.2, 1.5, 0.3, 0.8][s]
        opt.step(gr, out_bf16=out)
        ref.step(gr)
        clipped.append(ref.norm > 30.0)
    _close(opt.w, ref.w, VS_TORCH, f"{kind} w")
    _close(opt.ratios(), torch.tensor(ref.ratios), VS_TORCH, f"{kind} ratios")
    assert [r != 1.0 for r in opt.ratios().tolist()] == ADAPT
    assert (ref.w - w0.double()).abs().max() > 1e-2 and torch.equal(out, opt.w.to(torch.bfloat16))
    if extras:
        assert clipped == [True, False, True, False, True]
        assert opt.last_norm() == pytest.approx(ref.norm, rel=1e-6)
        _close(opt.ema, ref.ema, VS_TORCH, f"{kind} ema")
    # and the ratios did something: plain SGD / Adam over the same data ends elsewhere
    plain = _make(kind, w0.clone(), _segments(adapt=[False] * 5), **kw)
    g = torch.Generator().manual_seed(0)
    torch.randn(N, generator=g)
    for s in range(5):
        plain.step(torch.randn(N, generator=g) * [1.0, 0.2, 1.5, 0.3, 0.8][s])
    assert not torch.allclose(plain.w.double(), ref.w, **VS_TORCH)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_zero_weights_and_zero_gradient_take_ratio_exactly_one(kind):
    g = torch.Generator().manual_seed(2)
    _, starts = segs_of(SIZES)
    w0 = torch.randn(N, generator=g)
    w0[starts[0]:starts[1]] = 0.0            # tensor 0: zero weights
    gr = torch.randn(N, generator=g)
    gr[starts[2]:starts[3]] = 0.0            # tensor 2: zero gradient (LAMB: m, v and so u stay 0 with wd 0)
    opt = _make(kind, w0.clone(), weight_decay=0.0)
    opt.step(gr)
    r = opt.ratios().tolist()
    assert r[0] == 1.0 and r[2] == 1.0 and r[1] == 1.0 and r[4] == 1.0 and r[3] != 1.0
    assert torch.equal(opt.w[starts[2]:starts[3]], w0[starts[2]:starts[3]])  # nothing to apply there
    assert torch.isfinite(opt.w).all() and opt.w[starts[0]:starts[1]].abs().max() > 0


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_a_tensor_that_is_not_adapted_gets_no_weight_decay(kind):
    """Zero gradient, weight decay 0.5: adapted tensors shrink, the others do not move at all."""
    g = torch.Generator().manual_seed(3)
    _, starts = segs_of(SIZES)
    w0 = torch.randn(N, generator=g)
    opt = _make(kind, w0.clone(), weight_decay=0.5)
    opt.step(torch.zeros(N))
    for t, ad in enumerate(ADAPT):
        a, b = starts[t], starts[t + 1]
        if ad:
            assert (opt.w[a:b].abs() < w0[a:b].abs()).all()
        else:
            assert torch.equal(opt.w[a:b], w0[a:b])
    assert opt.table[:, 1].tolist() == [0.5 if ad else 0.0 for ad in ADAPT]


def test_defaults_are_untouched(monkeypatch):
    """FlatSGD / FlatAdam built without the new arguments hold nothing new, and on the GPU path they call exactly the
    entry points they called before (a recording stand-in for the library: no GPU needed)."""
    from tony_amd.ops import FlatAdam, FlatSGD, _lib, optim

    w = torch.randn(256)
    for opt in (FlatSGD(w.clone(), 0.1), FlatAdam(w.clone(), 1e-3)):
        for name in ("segments", "tsum", "table", "_items", "_item_part", "_order", "_tstart", "_adapt"):
            assert not hasattr(opt, name), name
        assert opt._xhp_dev is None and opt._ctl is None and opt._partials is None and opt.ema is None
        opt.step(torch.randn(256))
        assert set(opt.state_dict()) <= {"kind", "step", "momentum_buffer", "exp_avg", "exp_avg_sq", "lr"}

    calls = []

    class _Recorder:
        def __getattr__(self, name):
            def fn(*a):
                calls.append(name)
                return 0
            return fn

    class _FakeCuda(torch.Tensor):
        is_cuda = True

    monkeypatch.setattr(_lib, "lib", lambda: _Recorder())
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev: 0)
    monkeypatch.setattr(optim._FlatOptimizer, "_push_hp", lambda self: None)
    for cls, entry in ((FlatSGD, "tony_sgd_step"), (FlatAdam, "tony_adam_step")):
        opt = cls(w.clone(), 0.1)
        opt.w = opt.w.as_subclass(_FakeCuda)
        del calls[:]
        opt.step(torch.randn(256))
        assert calls == [entry], calls


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_state_dict_round_trip(kind):
    g = torch.Generator().manual_seed(5)
    w0 = torch.randn(N, generator=g)
    grads = [torch.randn(N, generator=g) for _ in range(3)]
    kw = dict(clip_norm=60.0, skip_nonfinite=True, ema_decay=0.9)
    a = _make(kind, w0.clone(), **kw)
    for gr in grads[:2]:
        a.step(gr)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    assert sd["kind"] == kind and sd["step"] == 2 and "ema" in sd and sd["skipped"] == 0
    assert ("momentum_buffer" in sd) == (kind == "lars") and ("exp_avg_sq" in sd) == (kind == "lamb")
    b = _make(kind, a.w.clone(), **kw)
    b.load_state_dict(sd)
    a.step(grads[2])
    b.step(grads[2])
    assert torch.equal(a.w, b.w) and torch.equal(a.ema, b.ema) and torch.equal(a.table, b.table)


def test_ranges_must_follow_the_segments():
    opt = _make("lars", torch.zeros(N))
    with pytest.raises(ValueError, match="segment boundaries"):
        opt.norm_range(torch.zeros(64), 8)
    from tony_amd.ops import FlatLARS, Segments

    with pytest.raises(ValueError, match="cover"):
        FlatLARS(torch.zeros(N), 0.1, segments=Segments([0, 64], [0], [True]))
    with pytest.raises(ValueError, match="multiples of 4"):
        FlatLARS(torch.zeros(8), 0.1, segments=Segments([0, 6, 8], [0, 1], [True, True]))
    whole = FlatLARS(torch.ones(N), 0.1)  # no table: the shard is one adapted tensor
    whole.step(torch.ones(N))
    assert whole.ratios().tolist() == [pytest.approx(0.001 * 1.0, rel=1e-6)]


@pytest.fixture
def hvd1(monkeypatch):
    import tony_amd.hvd as hvd

    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    monkeypatch.setenv("TONY_DIST_BACKEND", "gloo")
    hvd.init()
    yield hvd
    hvd.shutdown()


def test_hvd_refuses_what_the_fused_layerwise_path_cannot_do(hvd1):
    def params():
        return [torch.nn.Parameter(torch.zeros(16))]

    with pytest.raises(ValueError, match="AdamW"):
        hvd1.DistributedOptimizer(torch.optim.Adam(params(), lr=0.1), fused=True, lamb=True)
    for fused in (None, False):
        with pytest.raises(ValueError, match="fused=True"):
            hvd1.DistributedOptimizer(torch.optim.SGD(params(), lr=0.1), fused=fused, lars_coef=0.001)
        with pytest.raises(ValueError, match="fused=True"):
            hvd1.DistributedOptimizer(torch.optim.AdamW(params(), lr=0.1), fused=fused, lamb=True)
    with pytest.raises(ValueError, match="torch.optim.SGD"):
        hvd1.DistributedOptimizer(torch.optim.AdamW(params(), lr=0.1), fused=True, lars_coef=0.001)
    assert not hvd1.DistributedOptimizer(torch.optim.SGD(params(), lr=0.1))._fused  # no new option: as before


def test_parameter_server_refuses_lars_and_lamb_on_the_xgmi_plane():
    from tony_amd.parallel.ps import ParameterServer

    def net():
        return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))

    for kind in ("lars", "lamb"):
        with pytest.raises(ValueError, match='chunk by chunk.*plane="rccl"'):
            ParameterServer(net(), optimizer=kind, dtype=torch.float32, device="cpu", mode="dedicated", plane="xgmi")


@pytest.mark.parametrize("bucketed", [False, True], ids=["one-apply", "bucketed"])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_single_rank_parameter_server_matches_the_class(kind, bucketed):
    from tony_amd.parallel.flat import build_segments
    from tony_amd.parallel.ps import ParameterServer, make_optimizer

    def net():
        torch.manual_seed(3)
        return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))

    kw = dict(clip_norm=2.0, skip_nonfinite=True, ema_decay=0.9)
    ps = ParameterServer(net(), optimizer=kind, lr=0.05, momentum=0.9, weight_decay=1e-3, dtype=torch.float32,
                         device="cpu", trust_coef=0.02, bucketed_single=bucketed, bucket_mb=0.0001, **kw)
    assert ps.single != bucketed and ps.optimizers[0].segments.adapt == [True, False, True, False]
    hand = make_optimizer(kind, ps.flat.data.clone(), 0.05, 0.9, 1e-3, trust_coef=0.02,
                          segments=build_segments(ps.flat, [(0, ps.flat.numel)]), **kw)
    g = torch.Generator().manual_seed(1)
    for s in range(3):
        gr = torch.randn(ps.flat.numel, generator=g) * (0.1 if s == 1 else 1.0)
        ps.zero_grad()
        ps.flat.grad.copy_(gr)
        ps.step()
        hand.step(gr)
    _close(ps.flat.data, hand.w, dict(rtol=1e-5, atol=1e-5), f"{kind} PS variables")
    assert (hand.ratios() != 1.0).tolist() == [True, False, True, False]


def test_poly_warmup_lr_corners():
    from tony_amd.jobs.common import poly_warmup_lr

    assert poly_warmup_lr(0, 2.0, 4, 20) == pytest.approx(0.5)       # linear warm-up: (step + 1) / warmup
    assert poly_warmup_lr(3, 2.0, 4, 20) == pytest.approx(2.0)       # its last step reaches the base rate
    assert poly_warmup_lr(4, 2.0, 4, 20) == pytest.approx(2.0)       # the decay starts from it
    assert poly_warmup_lr(12, 2.0, 4, 20) == pytest.approx(2.0 * 0.25)  # half way, power 2
    assert poly_warmup_lr(12, 2.0, 4, 20, power=1.0) == pytest.approx(1.0)
    assert poly_warmup_lr(20, 2.0, 4, 20) == 0.0 and poly_warmup_lr(10 ** 6, 2.0, 4, 20) == 0.0
    assert poly_warmup_lr(20, 2.0, 4, 20, end_lr=0.1) == pytest.approx(0.1)
    assert poly_warmup_lr(12, 2.0, 4, 20, end_lr=0.4) == pytest.approx(0.4 + 1.6 * 0.25)
    assert poly_warmup_lr(0, 2.0, 0, 10) == pytest.approx(2.0)       # no warm-up
    seq = [poly_warmup_lr(s, 2.0, 4, 20) for s in range(21)]
    assert all(a <= b for a, b in zip(seq[:4], seq[1:4])) and all(a >= b for a, b in zip(seq[4:], seq[5:]))
    with pytest.raises(ValueError):
        poly_warmup_lr(0, 2.0, 8, 4)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(180)
def test_two_gloo_ranks_take_whole_tensor_ratios():
    """Colocated PS, more than 3 buckets, each rank owning half of every bucket, so several tensors lie on both
    ranks: both end bit-identical with identical ratio tables, the masters follow the float64 loop over WHOLE tensors
    and do not follow the loop that takes every rank's piece as a tensor of its own."""
    import layerwise_worker as W

    world, port = 2, _port()
    ctx = mp.get_context("spawn")
    with ctx.Pool(world) as pool:
        res = [pool.apply_async(W.cpu_rank, (r, world, port)) for r in range(world)]
        outs = [r.get(150) for r in res]
    for name in W.CONFIGS:
        a, b = outs[0][name], outs[1][name]
        for o in (a, b):
            print(name, {k: v for k, v in o.items() if not isinstance(v, bytes)})
        assert a["flat"] == b["flat"] and len(a["flat"]) > 4 * 54000     # the variables, bit for bit
        assert a["table"] == b["table"] and len(a["table"]) == 8 * 7     # (ratio_t, wd_t) of the 7 tensors
        for o in (a, b):
            bad = [k for k, v in o.items() if v is False]
            assert not bad, (name, bad, {k: v for k, v in o.items() if not isinstance(v, bytes)})
            tol_here = 1e-5 + 1e-4 * 16
            assert o["refs_err"] > 100 * tol_here  # the two references are far apart
