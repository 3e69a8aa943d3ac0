"""The fused Adagrad / RMSProp kernels (csrc/optim.hip tony_adagrad_step / tony_rmsprop_step) on the GPU:
against each class's own CPU fallback and against torch.optim, with poisoned surroundings, the bf16 compute
copy, hyper-parameters read on the device, the single-rank ParameterServer and the Horovod wrapper.

Tolerances are the project's two for this kind of check: kernel vs fallback (1e-5, 1e-5) over 3 steps
(test_fused_sgd_matches_reference), GPU vs torch.optim (1e-4, 1e-5) over 5 steps (test_fused_adam_matches_torch).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FALLBACK = dict(rtol=1e-5, atol=1e-5)
VS_TORCH = dict(rtol=1e-4, atol=1e-5)
N_SMALL = 4 * (3 * 256 + 1)      # several workgroups, the last one partial
N_TRIP = 4 * (8192 * 256 + 3)    # first size at which grid_for's cap gives a thread a second grid-stride trip

CASES = [("adagrad", 0.0), ("rmsprop", 0.0), ("rmsprop", 0.9), ("rmsprop_tf", 0.0), ("rmsprop_tf", 0.9)]


def _make(kind, w, momentum=0.9, lr=0.05):
    from tony_amd.ops import FlatAdagrad, FlatRMSProp

    if kind == "adagrad":
        return FlatAdagrad(w, lr=lr, eps=1e-5, weight_decay=1e-3)
    tf = kind == "rmsprop_tf"
    return FlatRMSProp(w, lr=lr, alpha=0.9, momentum=momentum, eps=1.0 if tf else 1e-8, weight_decay=1e-3,
                       tf_style=tf)


def _states(opt):
    return [t for t in opt.plane_state()[1:] if t is not None]


def _close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(a, b, **tol), f"{what}: max abs err {err}"


def _versus_fallback(cuda, kind, momentum, grad_dtype, n, steps=3):
    g = torch.Generator().manual_seed(n % 1000 + steps)
    w0 = torch.randn(n, generator=g)
    dev, ref = _make(kind, w0.to(cuda), momentum), _make(kind, w0.clone(), momentum)
    out = torch.empty(n, dtype=torch.bfloat16, device=cuda)
    for _ in range(steps):
        gr = torch.randn(n, generator=g).to(grad_dtype)
        dev.step(gr.to(cuda), out_bf16=out)
        ref.step(gr)
    _close(dev.w, ref.w, FALLBACK, f"{kind} w")
    for i, (a, b) in enumerate(zip(_states(dev), _states(ref))):
        _close(a, b, FALLBACK, f"{kind} state {i}")
    assert torch.equal(out, dev.w.to(torch.bfloat16))


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32], ids=["g-bf16", "g-fp32"])
@pytest.mark.parametrize("kind,momentum", CASES)
def test_kernel_matches_cpu_fallback(cuda, kind, momentum, grad_dtype):
    _versus_fallback(cuda, kind, momentum, grad_dtype, N_SMALL)


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop_tf"])
def test_kernel_matches_cpu_fallback_second_grid_stride_trip(cuda, kind):
    _versus_fallback(cuda, kind, 0.9, torch.bfloat16, N_TRIP)


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop", "rmsprop_tf"])
def test_apply_range_leaves_poisoned_surroundings_untouched(cuda, kind):
    """w, the states and the bf16 copy live inside larger NaN-patterned buffers; a range update of
    [1024, 1024 + 3076) of the 8192-element shard changes nothing else, guards included, nor the gradient."""
    shard, guard, lo, n = 8192, 512, 1024, N_SMALL

    def poisoned(numel, dtype=torch.float32):
        if dtype == torch.float32:
            big = torch.full((numel + 2 * guard,), 0x7FC0BEEF, dtype=torch.int32, device=cuda).view(torch.float32)
        else:
            big = torch.full((numel + 2 * guard,), 0x7FC5, dtype=torch.int16, device=cuda).view(torch.bfloat16)
        return big, big[guard:guard + numel]

    g = torch.Generator().manual_seed(11)
    wbig, w = poisoned(shard)
    w.copy_(torch.randn(shard, generator=g))
    opt = _make(kind, w)
    assert opt.w.data_ptr() == w.data_ptr()
    bigs = [wbig]
    for name in ("h", "ms", "mom"):
        if hasattr(opt, name):
            sbig, s = poisoned(shard)
            s.copy_(getattr(opt, name))
            setattr(opt, name, s)
            bigs.append(sbig)
    obig, out_full = poisoned(shard, torch.bfloat16)
    out = out_full[lo:lo + n]
    bigs.append(obig)
    gbig, grad = poisoned(n, torch.bfloat16)
    grad.copy_(torch.randn(n, generator=g))
    before = [b.clone() for b in bigs]
    gbefore = gbig.clone()
    opt.begin_step()
    opt.apply_range(grad, lo, out_bf16=out)
    torch.cuda.synchronize()

    def bits(t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    for b, a in zip(before, bigs):
        a0, a1 = guard + lo, guard + lo + n
        assert torch.equal(bits(a[:a0]), bits(b[:a0])) and torch.equal(bits(a[a1:]), bits(b[a1:]))
        assert torch.isfinite(a[a0:a1].float()).all() and not torch.equal(bits(a[a0:a1]), bits(b[a0:a1]))
    assert torch.equal(bits(gbig), bits(gbefore))
    assert torch.equal(out, opt.w[lo:lo + n].to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop", "rmsprop_tf"])
def test_bf16_copy_is_the_rounded_master_and_optional(cuda, kind):
    n = N_SMALL
    g = torch.Generator().manual_seed(5)
    w0 = torch.randn(n, generator=g)
    a, b = _make(kind, w0.to(cuda)), _make(kind, w0.to(cuda))
    out = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    for _ in range(3):
        gr = torch.randn(n, generator=g).to(cuda)
        a.step(gr, out_bf16=out)
        b.step(gr, out_bf16=None)
        assert torch.equal(out, a.w.to(torch.bfloat16))  # f2bf and torch's cast: both round to nearest even
    assert torch.equal(a.w, b.w)
    for sa, sb in zip(_states(a), _states(b)):
        assert torch.equal(sa, sb)


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop_tf"])
def test_learning_rate_is_read_on_the_device_each_step(cuda, kind):
    n = N_SMALL
    g = torch.Generator().manual_seed(6)
    w0 = torch.randn(n, generator=g)
    dev, ref = _make(kind, w0.to(cuda)), _make(kind, w0.clone())
    for lr in (0.05, 0.5):
        gr = torch.randn(n, generator=g)
        dev.lr = ref.lr = lr
        before = ref.w.clone()
        dev.step(gr.to(cuda))
        ref.step(gr)
    _close(dev.w, ref.w, FALLBACK, f"{kind} after an lr change")
    assert (ref.w - before).abs().max() > 0.1  # the second step's size is the new lr's


def _torch_run(cls, w0, grads, **kw):
    p = torch.nn.Parameter(w0.clone())
    opt = cls([p], **kw)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
    return p.detach()


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop"])
def test_kernel_matches_torch_optim(cuda, kind):
    from tony_amd.ops import FlatAdagrad, FlatRMSProp

    n = 4096
    g = torch.Generator().manual_seed(2)
    w0 = torch.randn(n, generator=g).to(cuda)
    grads = [torch.randn(n, generator=g).to(cuda) for _ in range(5)]
    if kind == "adagrad":
        opt = FlatAdagrad(w0.clone(), lr=0.05, eps=1e-5, initial_accumulator_value=0.1, weight_decay=1e-2)
        ref = _torch_run(torch.optim.Adagrad, w0, grads, lr=0.05, eps=1e-5, initial_accumulator_value=0.1,
                         weight_decay=1e-2)
    else:
        opt = FlatRMSProp(w0.clone(), lr=0.01, alpha=0.9, momentum=0.9, eps=1e-8, weight_decay=1e-2)
        ref = _torch_run(torch.optim.RMSprop, w0, grads, lr=0.01, alpha=0.9, momentum=0.9, eps=1e-8,
                         weight_decay=1e-2)
    for gr in grads:
        opt.step(gr)
    _close(opt.w, ref, VS_TORCH, f"{kind} vs torch.optim")


class _Net(torch.nn.Module):
    """Parameters only: the small net of tests/ps_plane_worker.py."""

    def __init__(self, sizes=(11000, 12000, 4136, 13000, 3000, 11008, 64)):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in sizes])


@pytest.mark.parametrize("kind", ["rmsprop_tf", "adagrad"])
def test_single_rank_parameter_server(cuda, kind):
    from tony_amd.parallel.ps import ParameterServer, make_optimizer

    torch.manual_seed(0)
    net = _Net()
    with torch.no_grad():
        for p in net.ps:
            p.copy_(torch.randn(p.shape).mul_(0.5))
    ps = ParameterServer(net, optimizer=kind, lr=0.05, momentum=0.9, weight_decay=1e-3, dtype=torch.bfloat16,
                         device=cuda)
    n = ps.flat.numel
    ref = make_optimizer(kind, ps.optimizers[0].w.cpu().clone(), 0.05, 0.9, 1e-3)
    idx = torch.arange(n, dtype=torch.float32)
    for s in range(3):
        gr = float(s % 3 + 1) * 0.25 + idx.remainder(4) * 0.125  # multiples of 1/8: exact in bf16
        ps.zero_grad()
        ps.flat.grad.copy_(gr.to(cuda))
        ps.step()
        ref.step(gr)
    torch.cuda.synchronize()
    _close(ps.optimizers[0].w, ref.w, FALLBACK, f"{kind} PS masters")
    assert torch.equal(ps.flat.data, ps.optimizers[0].w.to(torch.bfloat16))


def _two_linear(seed, dev):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16)).to(dev)


HVD_CASES = {
    "adam": (torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-2)),
    "adamw": (torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2)),
    "adagrad": (torch.optim.Adagrad, dict(lr=0.05, eps=1e-5, initial_accumulator_value=0.1)),
    "rmsprop": (torch.optim.RMSprop, dict(lr=1e-2, momentum=0.9, weight_decay=1e-2)),
}


@pytest.mark.parametrize("name", list(HVD_CASES))
def test_hvd_fused_family_matches_torch_and_state_dict_loads_into_torch(cuda, name, monkeypatch):
    import tony_amd.hvd as hvd

    cls, kw = HVD_CASES[name]
    monkeypatch.setenv("HOROVOD_RANK", "0")
    monkeypatch.setenv("HOROVOD_SIZE", "1")
    hvd.init()
    try:
        g = torch.Generator(device=cuda).manual_seed(1)
        x = torch.randn((8, 64), generator=g, device=cuda)
        y = torch.randint(0, 16, (8,), generator=g, device=cuda)

        def step(model, opt):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(model(x), y).backward()
            opt.step()

        def flat(model):
            return torch.cat([p.detach().reshape(-1) for p in model.parameters()])

        fm, rm = _two_linear(0, cuda), _two_linear(0, cuda)
        fused = hvd.DistributedOptimizer(cls(fm.parameters(), **kw), named_parameters=fm.named_parameters(),
                                         fused=True)
        assert fused._fused
        ref = cls(rm.parameters(), **kw)
        for _ in range(5):
            step(fm, fused)
            step(rm, ref)
        _close(flat(fm), flat(rm), VS_TORCH, f"hvd fused {name}, 5 steps")
        # torch's per-parameter format: loads into a plain torch optimizer, whose next step matches
        sd = fused.state_dict()
        assert len(sd["state"]) == 4 and all("step" in st for st in sd["state"].values())
        pm = _two_linear(0, cuda)
        pm.load_state_dict(fm.state_dict())
        plain = cls(pm.parameters(), **kw)
        plain.load_state_dict(sd)
        step(pm, plain)
        step(fm, fused)
        _close(flat(pm), flat(fm), VS_TORCH, f"hvd {name}: torch step after loading the fused state")
        # and back: a fresh fused wrapper continues from the same state
        om = _two_linear(0, cuda)
        om.load_state_dict(rm.state_dict())
        other = hvd.DistributedOptimizer(cls(om.parameters(), **kw), fused=True)
        other.load_state_dict(ref.state_dict())
        step(om, other)
        step(rm, ref)
        _close(flat(om), flat(rm), VS_TORCH, f"hvd {name}: fused step after loading torch's state")
    finally:
        hvd.shutdown()
