"""The kvstore's 2-bit gradient compression without a GPU: the torch implementation of parallel/kvstore.py
against the numpy reference (tests/kv_compress_ref.py) bit for bit, error-feedback conservation, parameter
validation, and dist_sync / dist_async runs with the words over gloo."""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import kv_compress_ref as ref
import kv_compress_workers as W


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same_f32(got, want, what):
    """Bit equality of two float32 arrays (NaN payloads and the sign of zero included)."""
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:8]}: got {got[bad[:8]]} want {want[bad[:8]]}"


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1025])
def test_torch_implementation_equals_the_reference_bit_for_bit(n, thr):
    from tony_amd.parallel import kvstore as kvs

    rng = np.random.default_rng(n)
    r_ref = (np.float32(0.4 * thr) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    r_ref[:15] = 0  # the first copy of the special values meets a zero residual (the denormals stay denormal)
    r = torch.from_numpy(r_ref.copy())
    for push in range(3):
        g = ref.gradient(n, thr, seed=7 * n + push)
        words_ref, r_ref = ref.quantise(g, r_ref, thr)
        words = kvs._quant2_torch(torch.from_numpy(g.copy()), r, thr)
        assert words.dtype == torch.int32 and words.shape == (ref.n_words(n),)
        got_words = words.numpy().view(np.uint32)
        assert np.array_equal(got_words, words_ref), f"push {push}: words differ"
        assert n % 16 == 0 or got_words[-1] >> np.uint32(2 * (n % 16)) == 0  # the unused pairs are 0
        _same_f32(r.numpy(), r_ref, f"push {push}: residual")
        _same_f32(kvs._dequant2_torch(words, n, thr).numpy(), ref.decode(words_ref, n, thr), f"push {push}: decoded")


def test_special_values_take_the_codes_the_contract_names():
    """The reference itself on the edge values, from a zero residual: pins the contract's NaN / infinity /
    threshold-neighbour rules, which the implementations are then compared with above."""
    thr = np.float32(0.5)
    s = ref.specials(thr)[:15]
    words, r = ref.quantise(s, np.zeros(15, np.float32), thr)
    #       thr -thr  <thr >-thr >thr <-thr  0  -0  inf -inf nan 1e-40 -1e-40 3thr -3thr
    want = [1, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0, 0, 1, 2]
    assert ref.codes(words, 15).tolist() == want
    assert np.isnan(r[10]) and r[8] == np.inf and r[9] == -np.inf and r[0] == 0 and r[13] == 2 * thr
    assert r[11] == np.float32(1e-40) and r[11] != 0  # a denormal survives
    # code 3 is never produced and decodes to 0
    assert ref.decode(np.array([0b11_10_01_00], np.uint32), 4, thr).tolist() == [0.0, 0.5, -0.5, 0.0]


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_error_feedback_conserves_the_gradient_sum(thr):
    """Gradients that are multiples of thr / 4 with |g| <= 2 thr, at thresholds that are powers of two: every
    intermediate is a small integer multiple of thr / 4, so the fp32 arithmetic is exact and the decoded pushes
    plus the final residual equal the sum of the gradients exactly (a threshold like 0.3, whose fp32 value
    fills the mantissa, has inexact multiples: its runs are covered bit for bit above, not by this identity)."""
    from tony_amd.parallel import kvstore as kvs

    n, pushes = 1025, 12
    t32 = np.float32(thr)
    rng = np.random.default_rng(3)
    r = torch.zeros(n)
    total_g, total_sent = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for _ in range(pushes):
        g = (rng.integers(-8, 9, n).astype(np.float32) * (t32 / np.float32(4))).astype(np.float32)
        words = kvs._quant2_torch(torch.from_numpy(g), r, float(t32))
        total_g += g
        total_sent += kvs._dequant2_torch(words, n, float(t32)).numpy()
    assert np.array_equal(total_sent + r.numpy(), total_g)
    assert np.abs(total_sent).max() > 0


def test_parameter_validation():
    import tony_amd.kv as kv

    s = kv.create("local")
    s.set_gradient_compression({"type": "none"})
    s.set_gradient_compression({"type": None, "threshold": 0.25})
    s.set_gradient_compression({})
    for kind in ("local", "device"):
        with pytest.raises(NotImplementedError):  # a one-process store has no wire
            kv.create(kind).set_gradient_compression({"type": "2bit", "threshold": 0.5})
    with pytest.raises(NotImplementedError):
        s.set_gradient_compression({"type": "1bit"})
    for bad in ({"type": "2bit", "threshold": 0.0}, {"type": "2bit", "threshold": -1.0},
                {"type": "2bit", "threshold": float("nan")}, {"type": "2bit", "treshold": 0.5},
                {"type": "none", "bits": 2}, {"type": 2}, {"type": "2bit", "threshold": "half"}):
        with pytest.raises(ValueError):
            s.set_gradient_compression(bad)
    from tony_amd.parallel import kvstore as kvs

    assert kvs._gc_threshold({"type": "2bit"}) == 0.5
    assert kvs._gc_threshold({"type": "2bit", "threshold": 0.3}) == float(np.float32(0.3))
    assert (kvs.OP_INIT, kvs.OP_PUSH, kvs.OP_PULL, kvs.OP_OPT, kvs.OP_STOP, kvs.OP_PUSH_X, kvs.OP_PULL_X) == tuple(
        range(7)) and min(kvs.OP_GC, kvs.OP_PUSH_C, kvs.OP_PUSH_CX) > kvs.OP_PULL_X


def test_server_parks_a_compressed_push_until_the_setting_and_the_init(monkeypatch):
    """A worker's compressed push can reach the server before rank 0's setting and before worker 0's INIT of the
    key (the server polls any worker first): it is parked, with its words, and decoded once both are there."""
    import json

    from tony_amd.parallel import kvstore as kvs

    monkeypatch.setenv("DMLC_ROLE", "server")
    monkeypatch.setenv("DMLC_NUM_SERVER", "1")
    monkeypatch.setenv("DMLC_NUM_WORKER", "2")
    srv = kvs._Server(kvs._Topology(), sync=False, plane=None)
    kid, n, thr = 5, 20, 0.5
    g = np.tile(np.float32([1.5, -1.5, 0.2, -0.2]), n // 4) * np.float32(thr)  # codes 1, 2, 0, 0
    words_ref, _ = ref.quantise(g, np.zeros(n, np.float32), thr)
    words = torch.from_numpy(words_ref.view(np.int32).copy())
    f32 = kvs._dcode(torch.float32)
    assert srv.handle(2, [kvs.OP_PUSH_C, kid, n, f32], words) is True
    assert len(srv.early_gc) == 1 and kid not in srv.early
    cfg = torch.tensor(list(json.dumps({"type": "2bit", "threshold": thr}).encode()), dtype=torch.uint8)
    srv.handle(1, [kvs.OP_GC, 0, cfg.numel(), kvs._dcode(torch.uint8)], cfg)
    assert srv.gc == thr and not srv.early_gc and kid in srv.early  # now it waits for the key
    srv.handle(1, [kvs.OP_INIT, kid, n, f32], torch.zeros(n))
    assert kid not in srv.early
    # an async server without an optimizer: the decoded push replaces the stored value
    _same_f32(srv.values[kid].numpy(), ref.decode(words_ref, n, thr), "decoded push")
    assert np.abs(srv.values[kid].numpy()).max() == thr


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(kind, steps, thr, big_n):
    port = _port()
    args = [(role, i, 1, 2, port, kind, steps, "cpu", thr, big_n)
            for role, i in (("scheduler", 0), ("server", 0), ("worker", 0), ("worker", 1))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(len(args)) as pool:
        outs = [r.get(150) for r in [pool.apply_async(W.kv_gc_rank, a) for a in args]]
    workers = sorted((o for o in outs if o["role"] == "worker"), key=lambda o: o["rank"])
    assert [o["rank"] for o in workers] == [0, 1]
    return workers


def test_dist_sync_over_gloo_follows_the_reference():
    """A scheduler, one server and two workers with the words over gloo: three steps of keys of 3 and 4099 fp32
    elements and a bf16 key.  The pulled fp32 values are what the reference predicts through the server's
    sgd; the bf16 key is pushed as without compression; a call after a push raises."""
    steps, thr, big_n = 3, 0.3, 4099
    workers = _run("dist_sync", steps, thr, big_n)
    want = W.predict(steps, 2, thr, [("a", 3), ("big", big_n)])
    for o in workers:
        for s in range(steps):
            for key in ("a", "big"):
                np.testing.assert_allclose(o["seen"][s][key], want[key][s], rtol=1e-6, atol=0,
                                           err_msg=f"worker {o['rank']} step {s} key {key}")
            assert o["seen"][s]["h"] == [-0.75 * (s + 1)] * W.HALF_N  # (1 + 2) / 2 * lr per round, in bf16
        assert o["compressed_ops"] == [0, 6], o["compressed_ops"]
        assert o["late"] == "RuntimeError", o["late"]
    assert np.abs(want["big"][-1]).max() > 0  # the run moved the weights


def test_dist_async_over_gloo_final_value():
    """dist_async applies every decoded push on arrival: after the globally last push of a key its value is
    -lr / 2 x the sum of all decoded pushes (exact at threshold 0.5), which the worker that made that push
    pulls last."""
    steps, thr, big_n = 3, 0.5, 4099
    workers = _run("dist_async", steps, thr, big_n)
    want = W.predict(steps, 2, thr, [("a", 3), ("big", big_n)])
    for key in ("a", "big"):
        assert any(np.array_equal(o["seen"][-1][key], want[key][-1]) for o in workers), key
    for o in workers:
        assert o["compressed_ops"] == [0, 6], o["compressed_ops"]
