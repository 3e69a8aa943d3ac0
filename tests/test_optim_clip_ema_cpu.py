"""Global-norm clipping, non-finite step skip and EMA of the flat optimizers (ops/optim.py) on CPU tensors:
against ``clip_grad_norm_`` + torch.optim, a float64 replay of the EMA, the skip, the checkpoint formats, what the
parameter server and the Horovod wrapper refuse, and the colocated PS over two gloo ranks (one global norm).

Tolerances are the project's two (tests/test_optim_family_gpu.py): VS_TORCH against torch.optim over 5 steps
(it also absorbs the 1e-6 torch adds to the norm before dividing), FALLBACK against a float64 replay.
"""
import multiprocessing as mp
import socket
import warnings

import pytest
import torch

FALLBACK = dict(rtol=1e-5, atol=1e-5)
VS_TORCH = dict(rtol=1e-4, atol=1e-5)
N = 3076
CLIP = 30.0
SCALES = [1.0, 0.2, 1.5, 0.3, 0.8]  # randn(3076) has norm ~55: steps 0, 2, 4 clip at 30, steps 1 and 3 do not


def _data(steps=5, n=N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * SCALES[i % 5] for i in range(steps)]


def _make(kind, w, **kw):
    from tony_amd.ops import FlatAdagrad, FlatAdam, FlatRMSProp, FlatSGD

    if kind == "sgd":
        return FlatSGD(w, lr=0.05, momentum=0.9, weight_decay=1e-2, **kw)
    if kind in ("adam", "adamw"):
        return FlatAdam(w, lr=1e-2, weight_decay=1e-2, decoupled=(kind == "adamw"), **kw)
    if kind == "adagrad":
        return FlatAdagrad(w, lr=0.05, eps=1e-5, initial_accumulator_value=0.1, weight_decay=1e-2, **kw)
    tf = kind == "rmsprop_tf"
    return FlatRMSProp(w, lr=0.01, alpha=0.9, momentum=0.9, eps=1.0 if tf else 1e-8, weight_decay=1e-2, tf_style=tf,
                       **kw)


TORCH = {
    "sgd": (torch.optim.SGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
    "adam": (torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-2)),
    "adamw": (torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2)),
    "adagrad": (torch.optim.Adagrad, dict(lr=0.05, eps=1e-5, initial_accumulator_value=0.1, weight_decay=1e-2)),
    "rmsprop": (torch.optim.RMSprop, dict(lr=0.01, alpha=0.9, momentum=0.9, eps=1e-8, weight_decay=1e-2)),
}
ALL_KINDS = ["sgd", "adam", "adamw", "adagrad", "rmsprop", "rmsprop_tf"]


def _states(opt):
    return [t for t in opt.plane_state()[1:] if t is not None]


def _close(a, b, tol, what):
    err = (a.double() - b.double()).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(a.double(), b.double(), **tol), f"{what}: max abs err {err}"


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_clipping_matches_clip_grad_norm_and_torch_optim(kind):
    w0, grads = _data()
    opt = _make(kind, w0.clone(), clip_norm=CLIP)
    norms = []
    for g in grads:
        opt.step(g)
        norms.append(opt.last_norm())
    for g, nrm in zip(grads, norms):
        assert nrm == pytest.approx(g.double().norm().item(), rel=1e-6)
    assert any(x > CLIP for x in norms) and any(x <= CLIP for x in norms), norms
    if kind == "rmsprop_tf":  # TF's form in float64, tf.clip_by_global_norm before the weight decay
        lr, alpha, mu, eps, wd = 0.01, 0.9, 0.9, 1.0, 1e-2
        w, ms, mom = w0.double(), torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
        for g in grads:
            g = g.double()
            g = g * (CLIP / max(g.norm().item(), CLIP))
            gp = g + wd * w
            ms = alpha * ms + (1 - alpha) * gp * gp
            mom = mu * mom + lr * gp / (ms + eps).sqrt()
            w = w - mom
        ref = w
    else:
        cls, kw = TORCH[kind]
        p = torch.nn.Parameter(w0.clone())
        topt = cls([p], **kw)
        for g in grads:
            p.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([p], CLIP)
            topt.step()
        ref = p.detach()
    _close(opt.w, ref, VS_TORCH, f"{kind} clipped vs torch")
    # and clipping did something: the unclipped run ends elsewhere
    plain = _make(kind, w0.clone())
    for g in grads:
        plain.step(g)
    assert not torch.allclose(plain.w.double(), ref.double(), **VS_TORCH)


def test_unclipped_step_uses_a_coefficient_of_exactly_one():
    w0, grads = _data()
    a, b = _make("sgd", w0.clone(), clip_norm=1e6), _make("sgd", w0.clone())
    for g in grads:
        a.step(g)
        b.step(g)
    assert torch.equal(a.w, b.w) and torch.equal(a.v, b.v)


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed-decay", "warmup"])
@pytest.mark.parametrize("kind", ["sgd", "rmsprop_tf"])
def test_ema_matches_float64_replay(kind, warmup):
    decay = 0.99
    w0, grads = _data()
    opt = _make(kind, w0.clone(), ema_decay=decay, ema_warmup=warmup)
    assert torch.equal(opt.ema, w0) and opt.ema.data_ptr() != opt.w.data_ptr()  # TF: the shadow starts at the value
    ema = w0.double()
    moved = 0.0
    for t, g in enumerate(grads, start=1):
        opt.step(g)
        d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
        ema = ema - (1.0 - d) * (ema - opt.w.double())
        moved = max(moved, (ema - w0.double()).abs().max().item())
    _close(opt.ema, ema, FALLBACK, f"{kind} ema warmup={warmup}")
    assert moved > 1e-3
    if warmup:  # (1 + t) / (10 + t) is far below 0.99 in the first steps: the warmed-up EMA follows much faster
        fixed = _make(kind, w0.clone(), ema_decay=decay)
        for g in grads:
            fixed.step(g)
        assert (opt.ema - opt.w).abs().max() < 0.8 * (fixed.ema - fixed.w).abs().max()


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_defaults_allocate_nothing_and_keep_the_state_dict(kind):
    w0, grads = _data(steps=1)
    opt = _make(kind, w0.clone())
    assert opt.ema is None and opt._xhp_dev is None and opt._ctl is None and opt._partials is None
    opt.step(grads[0])
    assert opt._partials is None and "ema" not in opt.state_dict() and "skipped" not in opt.state_dict()
    assert opt.skipped_steps() == 0
    only_clip = _make(kind, w0.clone(), clip_norm=1.0)
    assert only_clip.ema is None
    with pytest.raises(ValueError, match="clip_norm must be positive"):
        _make(kind, w0.clone(), clip_norm=0.0)
    with pytest.raises(ValueError, match="ema_decay must be in"):
        _make(kind, w0.clone(), ema_decay=1.0)
    with pytest.raises(ValueError, match="ema_warmup needs ema_decay"):
        _make(kind, w0.clone(), ema_warmup=True)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("kind", ["sgd", "adam", "rmsprop_tf"])
def test_nonfinite_gradient_skips_the_step(kind, bad):
    w0, grads = _data(steps=3)
    opt = _make(kind, w0.clone(), skip_nonfinite=True, ema_decay=0.9, clip_norm=CLIP)
    out = torch.zeros(N, dtype=torch.bfloat16)
    opt.step(grads[0], out_bf16=out)
    tensors = [opt.w, opt.ema, out] + _states(opt)
    before = [t.clone() for t in tensors]
    g = grads[1].clone()
    g[1234] = bad
    opt.step(g, out_bf16=out)
    assert opt.skipped_steps() == 1
    for a, b in zip(tensors, before):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))
    opt.step(grads[2], out_bf16=out)  # the next finite step proceeds
    assert opt.skipped_steps() == 1 and torch.isfinite(opt.w).all()
    for a, b in zip(tensors, before):
        assert not torch.equal(a, b)
    # without the option the same gradient goes through (and poisons the shard, as it always did)
    plain = _make(kind, w0.clone())
    plain.step(g)
    assert not torch.isfinite(plain.w).all()


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "rmsprop_tf"])
def test_checkpoint_round_trip_old_format_and_mismatch(kind):
    w0, grads = _data(steps=4, n=512)
    kw = dict(clip_norm=CLIP / 4, skip_nonfinite=True, ema_decay=0.9)
    a = _make(kind, w0.clone(), **kw)
    for g in grads[:2]:
        a.step(g)
    a.step(torch.full((512,), float("inf")))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    assert sd["skipped"] == 1 and torch.equal(sd["ema"], a.ema) and sd["step"] == 3
    b = _make(kind, a.w.clone(), **kw)
    b.load_state_dict(sd)
    assert b.skipped_steps() == 1 and torch.equal(b.ema, a.ema)
    a.step(grads[3])
    b.step(grads[3])
    assert torch.equal(a.w, b.w) and torch.equal(a.ema, b.ema)
    for sa, sb in zip(_states(a), _states(b)):
        assert torch.equal(sa, sb)
    # a checkpoint written before the EMA existed: accepted, the EMA re-seeds from the (restored) master
    old = {k: v for k, v in sd.items() if k not in ("ema", "skipped")}
    c = _make(kind, a.w.clone(), **kw)
    c.ema.add_(1.0)
    with pytest.warns(RuntimeWarning, match="re-seeding"):
        c.load_state_dict(old)
    assert torch.equal(c.ema, c.w) and c.skipped_steps() == 0
    # a checkpoint with an EMA into an optimizer that keeps none: refused
    with pytest.raises(ValueError, match="holds an EMA"):
        _make(kind, a.w.clone()).load_state_dict(sd)
    # and an old checkpoint into a default optimizer: as before, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _make(kind, a.w.clone()).load_state_dict(old)


def _ps_net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))


@pytest.mark.parametrize("bucketed", [False, True], ids=["one-apply", "bucketed"])
def test_parameter_server_cpu_clips_by_the_global_norm_and_swaps_the_ema(bucketed, tmp_path):
    from tony_amd.parallel.ps import ParameterServer, make_optimizer
    from tony_amd.utils.checkpoint import CheckpointManager

    def make_ps():
        return ParameterServer(_ps_net(), optimizer="rmsprop_tf", lr=0.05, momentum=0.9, weight_decay=1e-3,
                               dtype=torch.float32, device="cpu", clip_norm=2.0, ema_decay=0.9, skip_nonfinite=True,
                               bucketed_single=bucketed, bucket_mb=0.0001)

    ps = make_ps()
    assert ps.single != bucketed and (len(ps.buckets) > 1 or not bucketed)
    hand = make_optimizer("rmsprop_tf", ps.flat.data.clone(), 0.05, 0.9, 1e-3, clip_norm=2.0, ema_decay=0.9)
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(ps.flat.numel, generator=g) * s for s in (1.0, 0.1, 1.0, 0.1)]
    for gr in grads[:3]:
        ps.zero_grad()
        ps.flat.grad.copy_(gr)
        ps.step()
        hand.step(gr)
    # bucket masters are laid out in flat order with one rank: the bucketed step computes the same global norm
    _close(ps.flat.data, hand.w, FALLBACK, "PS variables")
    _close(ps.optimizers[0].ema, hand.ema, FALLBACK, "PS ema")
    before = ps.flat.data.clone()
    with ps.ema_weights():
        assert torch.equal(ps.flat.data, ps.optimizers[0].ema) and not torch.equal(ps.flat.data, before)
    assert torch.equal(ps.flat.data, before)
    # the sharded resume path (utils/checkpoint.py) carries the EMA and the skipped count
    ps.zero_grad()
    ps.flat.grad.fill_(float("nan"))
    ps.step()
    assert ps.optimizers[0].skipped_steps() == 1 and torch.equal(ps.flat.data, before)
    ck = CheckpointManager(str(tmp_path), save_steps=1, rank=0, async_write=False, sharded=True, world=1)
    ck.save(4, {"ps": ps.state_dict()}, force=True)
    state = ck.restore()
    other = make_ps()
    other.load_state_dict(state["ps"])
    assert other.optimizers[0].skipped_steps() == 1
    assert torch.equal(other.optimizers[0].ema, ps.optimizers[0].ema)
    for p in (ps, other):
        p.zero_grad()
        p.flat.grad.copy_(grads[3])
        p.step()
    assert torch.equal(other.flat.data, ps.flat.data) and torch.equal(other.optimizers[0].ema, ps.optimizers[0].ema)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with ParameterServer(_ps_net(), dtype=torch.float32, device="cpu").ema_weights():
            pass


def test_parameter_server_refuses_the_new_options_on_the_xgmi_plane():
    from tony_amd.parallel.ps import ParameterServer

    for kw in (dict(clip_norm=2.0), dict(skip_nonfinite=True), dict(ema_decay=0.99)):
        with pytest.raises(ValueError):
            ParameterServer(_ps_net(), dtype=torch.float32, device="cpu", mode="dedicated", plane="xgmi", **kw)
    with pytest.raises(ValueError, match='chunk by chunk.*plane="rccl"'):
        ParameterServer(_ps_net(), dtype=torch.float32, device="cpu", plane="xgmi", clip_norm=2.0)


@pytest.fixture
def hvd1(monkeypatch):
    import tony_amd.hvd as hvd

    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    monkeypatch.setenv("TONY_DIST_BACKEND", "gloo")
    hvd.init()
    yield hvd
    hvd.shutdown()


def test_hvd_clip_norm_needs_the_fused_path(hvd1):
    def params():
        return [torch.nn.Parameter(torch.zeros(16))]

    with pytest.raises(ValueError, match="fused=True"):
        hvd1.DistributedOptimizer(torch.optim.SGD(params(), lr=0.1), fused=False, clip_norm=1.0)
    with pytest.raises(ValueError, match="fused=True"):  # CPU tensors: nothing is fused, so nothing would clip
        hvd1.DistributedOptimizer(torch.optim.SGD(params(), lr=0.1), clip_norm=1.0)
    assert not hvd1.DistributedOptimizer(torch.optim.SGD(params(), lr=0.1))._fused  # no clip_norm: as before


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(180)
def test_two_gloo_ranks_clip_by_one_global_norm():
    """Colocated PS, more than 3 buckets, each rank owning half of every bucket: both ranks end with bit-identical
    variables that follow the CPU class clipping by the norm of the WHOLE averaged gradient -- and do not follow a
    reference that clips each rank's shard by the shard's own norm."""
    import clip_ema_worker as W

    world, port = 2, _port()
    ctx = mp.get_context("spawn")
    with ctx.Pool(world) as pool:
        res = [pool.apply_async(W.cpu_rank, (r, world, port)) for r in range(world)]
        outs = [r.get(150) for r in res]
    for o in outs:
        print({k: v for k, v in o.items() if k.endswith("_err") or k.endswith("norms")})
    assert torch.equal(outs[0]["flat"], outs[1]["flat"])
    assert torch.equal(outs[0]["ema_flat"], outs[1]["ema_flat"])
    for o in outs:
        assert o["norms"] == outs[0]["norms"]  # every rank computed the same norm, to the bit
        assert o["norms"] == pytest.approx(o["ref_norms"], rel=1e-6)
        assert any(o["clipped"]) and not all(o["clipped"])
        bad = [k for k, v in o.items() if v is False]
        assert not bad, (bad, {k: v for k, v in o.items() if not torch.is_tensor(v)})


@pytest.mark.timeout(180)
def test_dedicated_two_ps_tasks_and_two_workers_share_one_norm():
    """Dedicated PS, buckets placed round-robin on two ps tasks: each owner holds the partial blocks of its own
    buckets only, their sum over the ranks is the whole norm -- every step, so the other owner's blocks must not
    linger from the step before (4 steps, the norm differs from step to step)."""
    import clip_ema_worker as W

    world, port = 4, _port()
    ctx = mp.get_context("spawn")
    with ctx.Pool(world) as pool:
        res = [pool.apply_async(W.cpu_rank, (r, world, port, "dedicated", (0, 1))) for r in range(world)]
        outs = [r.get(150) for r in res]
    for o in outs:
        print({k: v for k, v in o.items() if k.endswith("_err") or k.endswith("norms")})
        assert torch.equal(o["flat"], outs[0]["flat"]) and torch.equal(o["ema_flat"], outs[0]["ema_flat"])
        assert any(o["clipped"]) and not all(o["clipped"])
        bad = [k for k, v in o.items() if v is False]
        assert not bad, (bad, {k: v for k, v in o.items() if not torch.is_tensor(v)})
    for o in outs[:2]:  # the two owners computed the same norm, to the bit, and it is the whole gradient's
        assert o["norms"] == outs[0]["norms"] and "master_match" in o
        assert o["norms"] == pytest.approx(o["ref_norms"], rel=1e-6)
    assert all("master_match" not in o and not o["norms"] for o in outs[2:])
