"""``tony_image_preprocess`` (csrc/image.hip) on the GPU: the float64 reference within the derived bound, the
exact identities by bit pattern, poisoned surroundings, the host refusals, and ``ImageBatches`` feeding the
``Trainer`` from its one persistent buffer."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from exact_helpers import assert_equal
from image_ref import GEOMETRIES, INCEPTION, RESNET, assert_close, box_tables, pixels, reference

pytestmark = pytest.mark.gpu

NORMS = {"inception": INCEPTION, "resnet": RESNET}
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _case(gi, norm):
    """(src, [(boxes, float64 reference)]) of geometry ``gi``: computed once, shared, never modified."""
    N, (H, W), size = GEOMETRIES[gi]
    src = pixels(N, H, W, seed=gi)
    return src, [(b, reference(src, b, size, *NORMS[norm])) for b in box_tables(N, H, W, seed=gi)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)), ids=lambda i: "geo%d" % i)
def test_matches_float64_reference(cuda, gi, norm, dtype):
    from tony_amd.ops.image import preprocess

    size = GEOMETRIES[gi][2]
    src, tables = _case(gi, norm)
    dsrc = src.to(cuda)
    for i, (boxes, ref) in enumerate(tables):
        got = preprocess(dsrc, boxes.to(cuda), size, dtype, *NORMS[norm])
        assert got.shape == ref.shape and got.dtype == dtype and got.permute(0, 2, 3, 1).is_contiguous()
        assert_close(got, ref, *NORMS[norm], f"geo{gi} {norm} {dtype} table {i}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_largest_dimensions(cuda, dtype):
    """4096 is the host's limit: (2*o+1)*h comes up to 2^25 here, the whole range of the kernel's multiply-shift
    division by 2*OH / 2*OW.  Thin images keep the case small."""
    from tony_amd.ops.image import preprocess

    for (H, W), size, box in [((4096, 3), (4096, 2), [0, 0, 4096, 3, 0]), ((4096, 2), (4095, 3), [1, 0, 4095, 2, 1]),
                              ((3, 4096), (2, 4096), [0, 0, 3, 4096, 1]), ((2, 4096), (3, 4077), [0, 5, 2, 4091, 0]),
                              ((4096, 2), (7, 5), [0, 0, 4096, 2, 0]), ((5, 4096), (4096, 3), [0, 0, 5, 4096, 1])]:
        src = pixels(1, H, W, seed=H + size[1])
        boxes = torch.tensor([box], dtype=torch.int32)
        ref = reference(src, boxes, size, *RESNET)
        got = preprocess(src.to(cuda), boxes.to(cuda), size, dtype, *RESNET)
        assert_close(got, ref, *RESNET, f"{H}x{W} -> {size} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_identity_flip_and_determinism_are_exact(cuda, dtype):
    from tony_amd.ops.image import preprocess

    N, H, W = 3, 37, 53  # 3 * 37 * 53 * 3 = 17649 elements: a tail, and groups that straddle rows and samples
    src = pixels(N, H, W, seed=11).to(cuda)
    full = torch.tensor([[0, 0, H, W, 0]] * N, dtype=torch.int32, device=cuda)
    got = preprocess(src, full, (H, W), dtype, 1.0, 0.0)
    assert_equal(got, src.permute(0, 3, 1, 2).to(dtype), "identity")  # integers <= 255 are exact in bf16
    for boxes in box_tables(N, H, W, seed=12):
        plain, flipped = boxes.clone(), boxes.clone()
        plain[:, 4], flipped[:, 4] = 0, 1
        a = preprocess(src, plain.to(cuda), (19, 23), dtype, *RESNET)
        b = preprocess(src, flipped.to(cuda), (19, 23), dtype, *RESNET)
        assert_equal(_bits(b), _bits(a.flip(-1)), "flip")
        again = preprocess(src, flipped.to(cuda), (19, 23), dtype, *RESNET)
        assert_equal(_bits(again), _bits(b), "two launches")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_poisoned_surroundings_and_buffer_reuse(cuda, dtype):
    from tony_amd.ops.image import preprocess

    N, (H, W), (OH, OW) = GEOMETRIES[0]
    n, guard = N * OH * OW * 3, 4096
    alloc = torch.full((2 * guard + n + 8,), float("nan"), dtype=dtype, device=cuda)
    poison = _bits(alloc).clone()
    out = alloc[guard:guard + n].view(N, OH, OW, 3).permute(0, 3, 1, 2)
    for step, seed in enumerate((21, 22)):  # the second, different batch reuses the buffer: nothing stale survives
        src = pixels(N, H, W, seed=seed).to(cuda)
        boxes = box_tables(N, H, W, seed=seed)[step].to(cuda)
        assert preprocess(src, boxes, (OH, OW), dtype, *INCEPTION, out=out) is out
        fresh = preprocess(src, boxes, (OH, OW), dtype, *INCEPTION)
        assert_equal(_bits(out), _bits(fresh), f"step {step}: out= against a fresh output")
        assert not torch.isnan(out.float()).any().item()
        now = _bits(alloc)
        assert torch.equal(now[:guard], poison[:guard]) and torch.equal(now[guard + n:], poison[guard + n:]), \
            f"step {step}: guard elements changed"


def test_host_refusals_have_their_own_codes(cuda):
    from tony_amd.ops import KernelError
    from tony_amd.ops.image import preprocess

    src = pixels(1, 6, 6).to(cuda)
    box = torch.tensor([[0, 0, 6, 6, 0]], dtype=torch.int32, device=cuda)
    flat = torch.full((4 * 4 * 3 + 16,), 7.0, dtype=torch.bfloat16, device=cuda)
    unaligned = flat[1:1 + 48].view(1, 4, 4, 3).permute(0, 3, 1, 2)  # 2 bytes past a 16-byte boundary
    with pytest.raises(KernelError, match=r"code -3\b"):
        preprocess(src, box, 4, torch.bfloat16, out=unaligned)
    with pytest.raises(KernelError, match=r"code -2\b"):
        preprocess(src, box, (5000, 1), torch.float32)
    with pytest.raises(KernelError, match=r"code -5\b"):
        preprocess(src.to(torch.int8), box, 4, torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(flat, torch.full_like(flat, 7.0))  # refused before any launch


class _Net(nn.Module):
    """A 3-channel image stem (as Inception's: 3x3 stride 2), one fused conv, classifier."""

    def __init__(self):
        super().__init__()
        from tony_amd.models.layers import ConvBNAct

        self.stem = ConvBNAct(3, 32, 3, 2, 0)
        self.c1 = ConvBNAct(32, 32, 3, 1, 1)
        self.fc = nn.Linear(32, 10)

    def forward(self, x):
        from tony_amd.ops.pool import global_avg_pool

        return self.fc(global_avg_pool(self.c1(self.stem(x))))


@pytest.fixture(scope="module")
def shard_dir(tmp_path_factory):
    from tony_amd.data.images import write_shards

    d = str(tmp_path_factory.mktemp("shards"))
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, (24, 40, 44, 3), dtype=np.uint8)
    write_shards(d, images, np.arange(24) % 10, per_shard=7)
    return d, images


def _losses(dev, use_graph, feed):
    from tony_amd.models.layers import init_weights
    from tony_amd.ops import cross_entropy
    from tony_amd.parallel.ps import ParameterServer
    from tony_amd.parallel.trainer import Trainer

    model = init_weights(_Net(), seed=0).to(dev).to(memory_format=torch.channels_last).train()
    ps = ParameterServer(model, optimizer="sgd", lr=0.05, momentum=0.9, device=dev)
    tr = Trainer(model, ps, lambda o, y: cross_entropy(o, y), use_graph=use_graph, warmup_eager=1)
    # no host synchronisation between the steps (a replayed step returns its one static loss tensor: clone it)
    out = [tr.step(*feed()).float().clone() for _ in range(3)]
    torch.cuda.synchronize()
    return [float(v) for v in out], tr


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_loader_feeds_the_trainer_from_one_buffer(cuda, shard_dir, use_graph):
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.image import normalisation, preprocess

    d, images = shard_dir
    kw = dict(train=True, model="inception", device=cuda, dtype=torch.bfloat16, seed=5)
    with ImageBatches(d, 8, 35, **kw) as b:
        clones = []
        for t in range(3):
            idx, boxes = b.plan(t)
            x, y = b.next()
            clones.append((x.clone(memory_format=torch.preserve_format), y.clone()))
            want = preprocess(torch.from_numpy(images[idx]).to(cuda), torch.from_numpy(boxes).to(cuda), 35,
                              torch.bfloat16, *normalisation("inception"))
            assert_equal(_bits(x), _bits(want), f"batch {t} through the staging slots")
            assert torch.equal(y.cpu(), torch.from_numpy(idx % 10))
        assert x.data_ptr() == b.x.data_ptr()  # the one persistent buffer
    it = iter(clones)
    ref, _ = _losses(cuda, use_graph, lambda: next(it))
    with ImageBatches(d, 8, 35, **kw) as b:
        got, tr = _losses(cuda, use_graph, b.next)
        if use_graph:
            assert tr.static_x.data_ptr() == b.x.data_ptr()  # adopted: the replay never copies the input
        assert isinstance(b.wait_ms, float)
    print(f"losses from the loader {got}, from clones {ref}")
    for a, r in zip(got, ref):  # the bound of test_trainer_gpu.py's eager against graph
        assert abs(a - r) <= 2e-2 * max(1.0, abs(r)), (got, ref)
