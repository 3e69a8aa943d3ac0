"""Multi-precision kvstore keys on the CPU: the torch path of ``Optimizer.update`` bit for bit against the numpy
contract (tests/kv_mp_ref.py), the setting's serialisation, 16-bit keys without the flag, the master's save / load
round trip and the refusal of a missized gradient.  ``problem`` and the tensor helpers are shared with
test_kv_mp_gpu.py."""
import json

import numpy as np
import pytest
import torch

import kv_mp_ref as mp

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}


def t16(bits, dtype, dev="cpu"):
    return torch.from_numpy(np.array(bits, np.uint16).view(np.int16)).to(dev).view(TD[dtype])  # (a copy)


def bits16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def f32(t):
    return t.detach().contiguous().cpu().numpy()


def source(s, dtype, dev):
    return t16(s[0], dtype, dev) if isinstance(s, tuple) else torch.from_numpy(s.copy()).to(dev)


def problem(n, nsrc, dtype, steps=3, seed=0):
    """The stored bits of a key of ``n`` elements and, per step, ``nsrc`` sources: 16-bit ones of ``dtype`` but the
    second, which is fp32 (when there are at least three); the first holds a NaN and values the clip cuts."""
    rng = np.random.default_rng(1000 * nsrc + n % 997 + seed)
    w = mp.rne16(np.resize(rng.standard_normal(min(n, 8191)).astype(np.float32), n), dtype)
    rounds = []
    for _ in range(steps):
        srcs = []
        for k in range(nsrc):
            g = np.resize((rng.standard_normal(min(n, 8191)) * 3).astype(np.float32), n)  # (a large key repeats a block)
            if k == 0 and n >= 3:
                g[0], g[1], g[n - 1] = np.nan, 100.0, -100.0
            srcs.append(g if (k == 1 and nsrc >= 3) else (mp.rne16(g, dtype), dtype))
        rounds.append(srcs)
    return w, rounds


def run_dense(kv, case, n, nsrc, dtype, dev, counted):
    """Three updates of an mp key on ``dev`` through ``Optimizer.update``, every tensor compared with the contract
    after each; ``counted``: the ``tony_kv_mp_dense`` launches expected per update (0: the torch path)."""
    name, cfg = mp.KINDS[case]
    opt = kv.create_optimizer(name, multi_precision=True, **cfg)
    wbits, rounds = problem(n, nsrc, dtype)
    weight = t16(wbits, dtype, dev)
    w32, st = mp.widen(wbits, dtype), {}
    for step, srcs in enumerate(rounds):
        opt.update(0, weight, [source(s, dtype, dev) for s in srcs])
        w32, st, stored = mp.step(case, w32, st, None, srcs, dtype)
        what = f"{case} {dtype} n {n} x{nsrc} step {step}"
        mp.same_bits(bits16(weight), stored, f"{what}: stored value", dtype)
        mp.same_bits(f32(opt.state[0]["w32"]), w32, f"{what}: w32")
        assert sorted(k for k in opt.state[0] if k not in ("t", "w32")) == sorted(st)
        for k in st:
            mp.same_bits(f32(opt.state[0][k]), st[k], f"{what}: {k}")
        assert opt.kernel_ops == [0, 0, counted * (step + 1), 0], opt.kernel_ops


@pytest.mark.parametrize("n", [9, 2053])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(mp.KINDS))
def test_cpu_path_equals_the_contract(case, dtype, n):
    import tony_amd.kv as kv

    run_dense(kv, case, n, 3, dtype, "cpu", 0)


def test_flag_is_in_the_setting_only_when_true():
    import tony_amd.kv as kv

    plain = kv.create_optimizer("nag", momentum=0.9)
    assert "multi_precision" not in plain.cfg and "multi_precision" not in json.loads(plain.to_json())
    assert kv.create_optimizer("nag", momentum=0.9, multi_precision=False).to_json() == plain.to_json()
    flagged = kv.Optimizer.from_json(kv.create_optimizer("nag", momentum=0.9, multi_precision=True).to_json())
    assert flagged.cfg["multi_precision"] is True and {k: v for k, v in flagged.cfg.items()
                                                       if k != "multi_precision"} == plain.cfg


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_key_without_the_flag_is_unchanged(dtype):
    """No master: computed in fp32 from the stored value, rounded once on the store -- the torch lines of
    ``Optimizer.update`` as they have always run; an fp32 key ignores the flag."""
    import tony_amd.kv as kv

    wbits, rounds = problem(2053, 1, dtype)
    weight, want = t16(wbits, dtype), t16(wbits, dtype)
    opt = kv.create_optimizer("sgd", learning_rate=0.1, momentum=0.5)
    m = torch.zeros(2053)
    for (s,) in rounds:
        g = t16(s[0], dtype)
        opt.update(0, weight, g)
        m.mul_(0.5).add_((g.float() * 1.0).add_(want.float(), alpha=0.0), alpha=-0.1)
        want = want.float().add_(m).to(TD[dtype])
        mp.same_bits(bits16(weight), bits16(want), f"sgd {dtype}", dtype)
    assert "w32" not in opt.state[0] and opt.kernel_ops == [0, 0]
    w, wf = torch.ones(8), torch.ones(8)
    kv.create_optimizer("sgd").update(0, w, torch.ones(8))
    flagged = kv.create_optimizer("sgd", multi_precision=True)
    flagged.update(0, wf, torch.ones(8))
    assert torch.equal(w, wf) and "w32" not in flagged.state[0]


def test_save_and_load_carry_the_master(tmp_path):
    import tony_amd.kv as kv

    store = kv.create("local")
    store.init("k", torch.ones(9, dtype=torch.bfloat16))
    store.set_optimizer(kv.create_optimizer("sgd", learning_rate=1.0, momentum=0.5, multi_precision=True))
    g = torch.full((9,), 2.0 ** -10)
    store.push("k", [g.bfloat16(), g])
    kid = store._key("k")
    w32, mom = (store._opt.state[kid][k].clone() for k in ("w32", "mom"))
    assert float(w32[0]) == 1 - 2.0 ** -9  # below half an ulp of the stored 1.0: only the master holds it
    store.save_optimizer_states(str(tmp_path / "opt.pt"))
    other = kv.create("local")
    other.init("k", torch.ones(9, dtype=torch.bfloat16))
    other.load_optimizer_states(str(tmp_path / "opt.pt"))
    assert other._opt.cfg == store._opt.cfg
    assert torch.equal(other._opt.state[kid]["w32"], w32) and torch.equal(other._opt.state[kid]["mom"], mom)
    for s in (store, other):
        s.push("k", g)
    assert torch.equal(other._opt.state[kid]["w32"], store._opt.state[kid]["w32"])
    assert torch.equal(other._store[kid], store._store[kid])


def test_a_missized_gradient_raises():
    import tony_amd.kv as kv

    opt = kv.create_optimizer("adagrad", multi_precision=True)
    w, tab = torch.ones(16, dtype=torch.float16), torch.ones(4, 8, dtype=torch.float16)
    with pytest.raises(ValueError):
        opt.update(0, w, [torch.ones(16), torch.ones(15)])
    with pytest.raises(ValueError):
        opt.update_rows(1, tab, torch.tensor([1, 2]), torch.ones(1, 8))
    assert bool((w == 1).all()) and bool((tab == 1).all())
