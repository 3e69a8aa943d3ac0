"""FlatAdagrad / FlatRMSProp (ops/optim.py) on CPU tensors: the PyTorch-op fallback against torch.optim and
against the TF-style formula in float64, ``apply_range``, the checkpoint round trip, the three new
``ParameterServer`` optimizer kinds, and what ``hvd.DistributedOptimizer(fused=True)`` refuses before it
touches a GPU."""
import pytest
import torch

N = 4096
TOL = dict(rtol=1e-5, atol=1e-5)


def _data(steps=5, n=N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]


def _torch_run(cls, w0, grads, **kw):
    p = torch.nn.Parameter(w0.clone())
    opt = cls([p], **kw)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p.detach(), opt


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adagrad_matches_torch(wd):
    from tony_amd.ops import FlatAdagrad

    w0, grads = _data()
    opt = FlatAdagrad(w0.clone(), lr=0.05, eps=1e-5, initial_accumulator_value=0.1, weight_decay=wd)
    assert torch.equal(opt.h, torch.full((N,), 0.1))
    for g in grads:
        opt.step(g)
    ref, topt = _torch_run(torch.optim.Adagrad, w0, grads, lr=0.05, eps=1e-5, initial_accumulator_value=0.1,
                           weight_decay=wd)
    print("adagrad max abs err", (opt.w - ref).abs().max().item())
    assert torch.allclose(opt.w, ref, **TOL)
    assert torch.allclose(opt.h, next(iter(topt.state.values()))["sum"], **TOL)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_torch_style_matches_torch(momentum):
    from tony_amd.ops import FlatRMSProp

    w0, grads = _data()
    opt = FlatRMSProp(w0.clone(), lr=0.01, alpha=0.9, momentum=momentum, eps=1e-8, weight_decay=1e-2)
    assert not opt.tf_style and torch.equal(opt.ms, torch.zeros(N))
    for g in grads:
        opt.step(g)
    ref, topt = _torch_run(torch.optim.RMSprop, w0, grads, lr=0.01, alpha=0.9, momentum=momentum, eps=1e-8,
                           weight_decay=1e-2)
    print("rmsprop max abs err", (opt.w - ref).abs().max().item())
    assert torch.allclose(opt.w, ref, **TOL)
    assert torch.allclose(opt.ms, next(iter(topt.state.values()))["square_avg"], **TOL)


def test_rmsprop_tf_style_matches_float64_formula():
    from tony_amd.ops import FlatRMSProp

    lr, alpha, mu, eps, wd = 0.045, 0.9, 0.9, 1.0, 4e-5
    w0, grads = _data()
    opt = FlatRMSProp(w0.clone(), lr=lr, alpha=alpha, momentum=mu, eps=eps, weight_decay=wd, tf_style=True)
    assert torch.equal(opt.ms, torch.ones(N)) and torch.equal(opt.mom, torch.zeros(N))
    w, ms, mom = w0.double(), torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for g in grads:
        opt.step(g)
        gp = g.double() + wd * w
        ms = alpha * ms + (1 - alpha) * gp * gp
        mom = mu * mom + lr * gp / (ms + eps).sqrt()
        w = w - mom
    print("rmsprop_tf max abs err", (opt.w.double() - w).abs().max().item())
    assert torch.allclose(opt.w.double(), w, **TOL)
    assert torch.allclose(opt.ms.double(), ms, **TOL) and torch.allclose(opt.mom.double(), mom, **TOL)


def _make(kind, w):
    from tony_amd.ops import FlatAdagrad, FlatRMSProp

    if kind == "adagrad":
        return FlatAdagrad(w, lr=0.05, eps=1e-5, weight_decay=1e-3)
    return FlatRMSProp(w, lr=0.01, momentum=0.9, weight_decay=1e-3, tf_style=(kind == "rmsprop_tf"),
                       eps=1.0 if kind == "rmsprop_tf" else 1e-8)


def _states(opt):
    return [t for t in opt.plane_state()[1:] if t is not None]


KINDS = ["adagrad", "rmsprop", "rmsprop_tf"]


@pytest.mark.parametrize("kind", KINDS)
def test_apply_range_checks_and_touches_only_its_range(kind):
    w0, grads = _data(steps=1, n=256)
    opt = _make(kind, w0.clone())
    g = grads[0]
    for lo, n in ((2, 64), (0, 6), (-4, 64), (224, 64), (256, 4)):
        with pytest.raises(ValueError, match="outside the 256-element shard or not 4-aligned"):
            opt.apply_range(g[:n], lo)
    before = [opt.w.clone()] + [s.clone() for s in _states(opt)]
    lo, n = 64, 100
    opt.begin_step()
    opt.apply_range(g[:n], lo)
    for b, a in zip(before, [opt.w] + _states(opt)):
        assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[lo + n:], b[lo + n:])
        assert not torch.equal(a[lo:lo + n], b[lo:lo + n])
    # the range update is the whole-shard update restricted to it
    whole = _make(kind, w0.clone())
    full = torch.zeros(256)
    full[lo:lo + n] = g[:n]
    whole.step(full)
    assert torch.equal(whole.w[lo:lo + n], opt.w[lo:lo + n])


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_round_trip_is_bit_exact(kind):
    w0, grads = _data(steps=4, n=512)
    a = _make(kind, w0.clone())
    for g in grads[:3]:
        a.step(g)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    assert sd["kind"] == ("adagrad" if kind == "adagrad" else "rmsprop") and sd["step"] == 3 and "lr" in sd
    if kind == "adagrad":
        assert set(sd) == {"kind", "step", "sum", "lr"}
    else:
        assert set(sd) == {"kind", "step", "square_avg", "momentum_buffer", "tf_style", "lr"}
        assert sd["tf_style"] == (kind == "rmsprop_tf")
    b = _make(kind, a.w.clone())
    b.load_state_dict(sd)
    assert b.step_count == 3
    a.step(grads[3])
    b.step(grads[3])
    assert torch.equal(a.w, b.w)
    for sa, sb in zip(_states(a), _states(b)):
        assert torch.equal(sa, sb)


def test_plane_state_of_sgd_and_adam_is_what_the_plane_passed_before():
    from tony_amd.ops import FlatAdam, FlatSGD

    w = torch.zeros(8)
    sgd, adam = FlatSGD(w.clone(), 0.1), FlatAdam(w.clone())
    code, s0, s1 = sgd.plane_state()
    assert code == 0 and s0 is sgd.v and s1 is None
    code, s0, s1 = adam.plane_state()
    assert code == 1 and s0 is adam.m and s1 is adam.v


def _ps_net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_server_cpu_steps_and_checkpoint(kind):
    from tony_amd.ops import FlatAdagrad, FlatRMSProp
    from tony_amd.parallel.ps import ParameterServer

    def make_ps():
        return ParameterServer(_ps_net(), optimizer=kind, lr=0.05, momentum=0.9, weight_decay=1e-3,
                               dtype=torch.float32, device="cpu")

    ps = make_ps()
    opt = ps.optimizers[0]
    if kind == "adagrad":
        assert isinstance(opt, FlatAdagrad) and opt.eps == 1e-7 and float(opt.h[0]) == pytest.approx(0.1)
        hand = FlatAdagrad(ps.flat.data.clone(), lr=0.05, weight_decay=1e-3)
    else:
        tf = kind == "rmsprop_tf"
        assert isinstance(opt, FlatRMSProp) and opt.tf_style == tf and opt.momentum == 0.9
        assert opt.eps == (1.0 if tf else 1e-8)  # rmsprop_tf: the Inception recipe's epsilon by default
        hand = FlatRMSProp(ps.flat.data.clone(), lr=0.05, momentum=0.9, weight_decay=1e-3, tf_style=tf,
                           eps=1.0 if tf else 1e-8)
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(ps.flat.numel, generator=g) for _ in range(4)]
    for gr in grads[:3]:
        ps.zero_grad()
        ps.flat.grad.copy_(gr)
        ps.step()
        hand.step(gr)
    assert torch.equal(opt.w, hand.w) and torch.equal(ps.flat.data, hand.w)
    sd = ps.state_dict()
    other = make_ps()
    other.load_state_dict(sd)
    for p in (ps, other):
        p.zero_grad()
        p.flat.grad.copy_(grads[3])
        p.step()
    assert other.steps == 4 and torch.equal(other.flat.data, ps.flat.data)
    assert torch.equal(other.optimizers[0].w, ps.optimizers[0].w)


def test_parameter_server_kw_and_unknown_kind():
    from tony_amd.parallel.ps import ParameterServer, make_optimizer

    w = torch.zeros(8)
    o = make_optimizer("adagrad", w.clone(), 0.1, eps=1e-5, initial_accumulator_value=0.5)
    assert o.eps == 1e-5 and float(o.h[0]) == 0.5
    o = make_optimizer("rmsprop_tf", w.clone(), 0.1, momentum=0.5, alpha=0.8, eps=0.25)
    assert (o.alpha, o.momentum, o.eps, o.tf_style) == (0.8, 0.5, 0.25, True)
    with pytest.raises(ValueError, match="unknown optimizer"):
        ParameterServer(_ps_net(), optimizer="adadelta", dtype=torch.float32, device="cpu")


@pytest.fixture
def hvd1(monkeypatch):
    import tony_amd.hvd as hvd

    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    monkeypatch.setenv("TONY_DIST_BACKEND", "gloo")
    hvd.init()
    yield hvd
    hvd.shutdown()


def test_hvd_fused_family_rejections_on_cpu(hvd1):
    def params(dtype=torch.float32):
        return [torch.nn.Parameter(torch.zeros(16, dtype=dtype))]

    # CPU tensors: nothing to fuse, as before
    with pytest.raises(ValueError, match="needs a single-group"):
        hvd1.DistributedOptimizer(torch.optim.Adam(params()), fused=True)
    # unsupported options and bf16 parameters are named before any GPU call
    with pytest.raises(ValueError, match="amsgrad"):
        hvd1.DistributedOptimizer(torch.optim.Adam(params(), amsgrad=True), fused=True)
    with pytest.raises(ValueError, match="centered"):
        hvd1.DistributedOptimizer(torch.optim.RMSprop(params(), centered=True), fused=True)
    with pytest.raises(ValueError, match="maximize"):
        hvd1.DistributedOptimizer(torch.optim.Adagrad(params(), maximize=True), fused=True)
    with pytest.raises(ValueError, match="lr_decay"):
        hvd1.DistributedOptimizer(torch.optim.Adagrad(params(), lr_decay=0.1), fused=True)
    with pytest.raises(ValueError, match="fp32 parameters"):
        hvd1.DistributedOptimizer(torch.optim.Adam(params(torch.bfloat16)), fused=True)
    # fused=None still auto-fuses SGD only: these keep torch's own step
    for opt in (torch.optim.Adam(params()), torch.optim.Adagrad(params()), torch.optim.RMSprop(params())):
        assert not hvd1.DistributedOptimizer(opt)._fused
