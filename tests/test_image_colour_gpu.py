"""``tony_image_preprocess_colour`` (csrc/image.hip) on the GPU: the float64 reference of the colour-distortion
contract within the derived bound (tests/image_colour_ref.py), rows of order -1 bit for bit as without a table, the
exact identities by bit pattern, poisoned surroundings and buffer reuse, the host refusals, and ``ImageBatches``
with a colour table feeding the ``Trainer`` from its one persistent buffer.

Worst error / bound on an MI355X (each test prints its own): fp32 0.23 (the 299 x 299 full form; 0.16 over the small
geometries), bf16 0.998, where the half ulp of the output dominates."""
import functools

import numpy as np
import pytest
import torch

from exact_helpers import assert_equal
from image_colour_ref import adversarial_pixels, assert_close, bound, colour_tables, reference
from image_ref import GEOMETRIES, INCEPTION, RESNET, box_tables, halfulp_bf16, pixels
from test_image_gpu import _losses, shard_dir  # noqa: F401 - shard_dir is a fixture

pytestmark = pytest.mark.gpu

NORMS = {"inception": INCEPTION, "resnet": RESNET}
DTYPES = [torch.float32, torch.bfloat16]
B32 = float(np.float32(32 / 255))


@functools.lru_cache(maxsize=None)
def _case(gi, norm):
    """(src, [(boxes, colour table, float64 reference)]) of geometry ``gi``: computed once, shared, never modified.
    The real-sized geometry gets one table for the full form and one for the fast form."""
    N, (H, W), size = GEOMETRIES[gi]
    src = adversarial_pixels(pixels(N, H, W, seed=gi))
    boxes, tables = box_tables(N, H, W, seed=gi), colour_tables(N, seed=gi)
    if H * W > 10000:
        fast = torch.tensor([[4, B32, 1.4, 0, 1], [5, -B32, 0.6, 0, 1]], dtype=torch.float32)
        tables = [tables[0], fast]
    return src, [(boxes[i % len(boxes)], c, reference(src, boxes[i % len(boxes)], c, size, *NORMS[norm]))
                 for i, c in enumerate(tables)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("gi", range(3), ids=lambda i: "geo%d" % i)
def test_matches_float64_reference(cuda, gi, norm, dtype):
    from tony_amd.ops.image import preprocess

    size = GEOMETRIES[gi][2]
    src, cases = _case(gi, norm)
    dsrc = src.to(cuda)
    worst = 0.0
    for i, (boxes, colour, ref) in enumerate(cases):
        got = preprocess(dsrc, boxes.to(cuda), size, dtype, *NORMS[norm], colour=colour.to(cuda))
        assert got.shape == ref.shape and got.dtype == dtype and got.permute(0, 2, 3, 1).is_contiguous()
        worst = max(worst, assert_close(got, ref, colour, *NORMS[norm], f"geo{gi} {norm} {dtype} table {i}"))
    print(f"geo{gi} {norm} {dtype}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_real_size_matches_float64_reference(cuda, mode):
    """299 x 299 once per mode: 350 workgroups in the apply pass, 64 partial sums per sample in the statistics."""
    from tony_amd.ops.image import preprocess

    size = GEOMETRIES[3][2]
    src, cases = _case(3, "inception")
    boxes, colour, ref = cases[0 if mode == "full" else 1]
    for dtype in DTYPES:
        got = preprocess(src.to(cuda), boxes.to(cuda), size, dtype, *INCEPTION, colour=colour.to(cuda),
                         colour_has_contrast=mode == "full")
        assert_close(got, ref, colour, *INCEPTION, f"299 {mode} {dtype}")


def test_one_column_and_one_pixel_outputs(cuda):
    """OW == 1 (the statistics pass divides by OW) and a 1 x 1 output (a lane's 8 pixels lie in 8 samples)."""
    from tony_amd.ops.image import preprocess

    for N, size in ((2, (7, 1)), (11, (1, 1))):
        src = pixels(N, 9, 6, seed=N)
        boxes = torch.tensor([[1, 1, 7, 4, n % 2] for n in range(N)], dtype=torch.int32)
        colour = torch.tensor([[n % 7 - 1, 0.1, 1.3, -0.15, 0.6 + 0.05 * n] for n in range(N)], dtype=torch.float32)
        ref = reference(src, boxes, colour, size, *RESNET)
        got = preprocess(src.to(cuda), boxes.to(cuda), size, torch.float32, *RESNET, colour=colour.to(cuda))
        assert_close(got, ref, colour, *RESNET, f"{N} x {size}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rows_without_an_order_keep_their_bits(cuda, dtype):
    from tony_amd.ops.image import preprocess

    N, (H, W), size = GEOMETRIES[0]  # 437 pixels per sample: lanes straddle a plain and a distorted sample
    src = pixels(N, H, W, seed=31).to(cuda)
    for boxes in box_tables(N, H, W, seed=31)[:2]:
        plain = preprocess(src, boxes.to(cuda), size, dtype, *RESNET)
        for rows in ([[-1, 0.1, 1.3, 0.1, 0.7], [2, 0.1, 1.3, 0.1, 0.7], [-1, 0, 1, 0, 1]],
                     [[4, 0.1, 1.3, 0, 1], [-1, 0.1, 1.3, 0.1, 0.7], [1, -0.1, 0.6, 0.2, 1.4]]):
            colour = torch.tensor(rows, dtype=torch.float32)
            got = preprocess(src, boxes.to(cuda), size, dtype, *RESNET, colour=colour.to(cuda))
            for n in range(N):
                if rows[n][0] < 0:
                    assert_equal(_bits(got[n]), _bits(plain[n]), f"sample {n} of {rows}")
                else:
                    assert not torch.equal(_bits(got[n]), _bits(plain[n]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_determinism_and_flip(cuda, dtype):
    from tony_amd.ops.image import preprocess

    N, (H, W), size = GEOMETRIES[0]
    src = pixels(N, H, W, seed=11).to(cuda)
    fast = torch.tensor([[4, 0.1, 1.4, 0, 1], [5, -0.12, 0.6, 0, 1], [4, -0.05, 0.9, 0, 1]], dtype=torch.float32)
    full = torch.tensor([[0, 0.1, 1.4, 0.15, 0.6], [3, -0.12, 0.6, -0.2, 1.45], [2, 0.05, 1.2, 0.1, 1.3]],
                        dtype=torch.float32)
    for boxes in box_tables(N, H, W, seed=12)[:3]:
        plain, flipped = boxes.clone(), boxes.clone()
        plain[:, 4], flipped[:, 4] = 0, 1
        for colour in (fast, full):
            a = preprocess(src, plain.to(cuda), size, dtype, *RESNET, colour=colour.to(cuda))
            b = preprocess(src, flipped.to(cuda), size, dtype, *RESNET, colour=colour.to(cuda))
            again = preprocess(src, flipped.to(cuda), size, dtype, *RESNET, colour=colour.to(cuda))
            assert_equal(_bits(again), _bits(b), "two launches")
            if colour is fast:  # per-pixel ops only
                assert_equal(_bits(b), _bits(a.flip(-1)), "flip, fast orders")
            else:  # the mean's summation order differs: both lie within the bound of one exact value
                ref = reference(src.cpu(), plain, colour, size, *RESNET)
                lim = 2 * bound(colour, *RESNET).expand_as(ref)
                if dtype == torch.bfloat16:
                    lim = lim + 2 * halfulp_bf16(ref)
                err = (b.flip(-1).double().cpu() - a.double().cpu()).abs()
                assert bool((err <= lim).all()), f"flip, full orders: worst {float((err / lim).max()):.3f}x"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_grey_ignores_saturation_and_the_clip_is_exact(cuda, dtype):
    from tony_amd.ops.image import preprocess

    N, (H, W), size = GEOMETRIES[0]
    boxes = box_tables(N, H, W, seed=5)[0].to(cuda)
    grey = pixels(N, H, W, seed=6)[..., :1].expand(N, H, W, 3).contiguous().to(cuda)  # r = g = b
    for order in (4, 5):
        one = torch.tensor([[order, d, 1.0, 0, 1] for d in (0.1, -0.1, 0.02)], dtype=torch.float32)
        want = preprocess(grey, boxes, size, dtype, *RESNET, colour=one.to(cuda), colour_has_contrast=False)
        for f in (0.5, 1.37, float(np.nextafter(np.float32(1.5), np.float32(0)))):
            other = one.clone()
            other[:, 2] = f
            got = preprocess(grey, boxes, size, dtype, *RESNET, colour=other.to(cuda), colour_has_contrast=False)
            assert_equal(_bits(got), _bits(want), f"grey, order {order}, saturation {f}")
    white = torch.full((N, H, W, 3), 255, dtype=torch.uint8, device=cuda)
    black = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=cuda)
    for scale, bias in (INCEPTION, RESNET):
        k = np.float32(255) * np.array(scale, dtype=np.float32)  # the fp32 product 255 * scale_c
        top = torch.tensor(k + np.array(bias, dtype=np.float32)).to(dtype)  # fmaf(1, k, bias): one rounding
        low = torch.tensor(np.array(bias, dtype=np.float32)).to(dtype)
        for orders in ((0, 1, 2), (3, 4, 5)):
            up = torch.tensor([[o, B32, 1.3, 0.1, 1.4] for o in orders], dtype=torch.float32, device=cuda)
            down = torch.tensor([[o, -B32, 0.7, -0.1, 0.6] for o in orders], dtype=torch.float32, device=cuda)
            got = preprocess(white, boxes, size, dtype, scale, bias, colour=up)
            assert_equal(_bits(got), _bits(top.to(cuda)[None, :, None, None].expand_as(got)), f"white {orders}")
            got = preprocess(black, boxes, size, dtype, scale, bias, colour=down)
            assert_equal(_bits(got), _bits(low.to(cuda)[None, :, None, None].expand_as(got)), f"black {orders}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_poisoned_surroundings_and_buffer_reuse(cuda, dtype):
    from tony_amd.ops.image import colour_scratch_floats, preprocess

    N, (H, W), (OH, OW) = GEOMETRIES[0]
    n, guard, need = N * OH * OW * 3, 4096, colour_scratch_floats(N, OH, OW)
    assert need == N * (2 + 1) * 3  # 437 pixels: two partial sums per sample and channel, then the means
    alloc = torch.full((2 * guard + n + 8,), float("nan"), dtype=dtype, device=cuda)
    salloc = torch.full((2 * guard + need,), float("nan"), dtype=torch.float32, device=cuda)
    poison, spoison = _bits(alloc).clone(), _bits(salloc).clone()
    out = alloc[guard:guard + n].view(N, OH, OW, 3).permute(0, 3, 1, 2)
    scratch = salloc[guard:guard + need]
    tables = [torch.tensor([[0, 0.1, 1.4, 0.15, 0.6], [3, -0.12, 0.6, -0.2, 1.45], [2, 0.05, 1.2, 0.1, 1.3]]),
              torch.tensor([[-1, 0, 1, 0, 1], [1, 0.03, 0.8, 0.05, 1.2], [5, -0.1, 1.1, 0, 1]])]
    for step, seed in enumerate((21, 22)):  # batch B, of other orders, reuses out and the scratch of batch A
        src = pixels(N, H, W, seed=seed).to(cuda)
        boxes = box_tables(N, H, W, seed=seed)[step].to(cuda)
        colour = tables[step].to(cuda)
        assert preprocess(src, boxes, (OH, OW), dtype, *INCEPTION, out=out, colour=colour, scratch=scratch) is out
        fresh = preprocess(src, boxes, (OH, OW), dtype, *INCEPTION, colour=colour)
        assert_equal(_bits(out), _bits(fresh), f"step {step}: out= and scratch= against a fresh run")
        assert not torch.isnan(out.float()).any().item()
        now, snow = _bits(alloc), _bits(salloc)
        assert torch.equal(now[:guard], poison[:guard]) and torch.equal(now[guard + n:], poison[guard + n:]), \
            f"step {step}: guard elements of out changed"
        assert torch.equal(snow[:guard], spoison[:guard]), f"step {step}: the scratch's front guard changed"
        assert torch.equal(snow[guard + need:], spoison[guard + need:]), \
            f"step {step}: the scratch changed beyond its stated size"


def test_host_refusals_have_their_own_codes(cuda):
    from tony_amd.ops import KernelError
    from tony_amd.ops.image import colour_scratch_floats, preprocess

    src = pixels(1, 6, 6).to(cuda)
    box = torch.tensor([[0, 0, 6, 6, 0]], dtype=torch.int32, device=cuda)
    colour = torch.tensor([[0, 0.1, 1.2, 0.1, 0.8]], dtype=torch.float32, device=cuda)
    flat = torch.full((4 * 4 * 3 + 16,), 7.0, dtype=torch.bfloat16, device=cuda)
    aligned = flat[:48].view(1, 4, 4, 3).permute(0, 3, 1, 2)
    unaligned = flat[1:1 + 48].view(1, 4, 4, 3).permute(0, 3, 1, 2)  # 2 bytes past a 16-byte boundary
    need = colour_scratch_floats(1, 4, 4)
    assert need == 6
    small = torch.full((need - 1,), 5.0, device=cuda)
    with pytest.raises(KernelError, match=r"code -3\b"):
        preprocess(src, box, 4, torch.bfloat16, out=unaligned, colour=colour)
    with pytest.raises(KernelError, match=r"code -8\b"):
        preprocess(src, box, 4, torch.bfloat16, out=aligned, colour=colour, scratch=small)
    with pytest.raises(KernelError, match=r"code -2\b"):
        preprocess(src, box, (5000, 1), torch.float32, colour=colour, colour_has_contrast=False)
    with pytest.raises(KernelError, match=r"code -5\b"):
        preprocess(src.to(torch.int8), box, 4, torch.bfloat16, out=aligned, colour=colour)
    for bad in (colour.double(), colour.to(torch.int32), colour[:, :4].contiguous(), colour.repeat(2, 1),
                colour.cpu()):
        with pytest.raises(ValueError, match="colour must be"):
            preprocess(src, box, 4, torch.bfloat16, out=aligned, colour=bad)
    with pytest.raises(ValueError, match="scratch must be"):
        preprocess(src, box, 4, torch.bfloat16, out=aligned, colour=colour, scratch=small.double())
    torch.cuda.synchronize()
    assert torch.equal(flat, torch.full_like(flat, 7.0)) and torch.equal(small, torch.full_like(small, 5.0))
    # the fast form needs no scratch at all
    preprocess(src, box, 4, torch.bfloat16, out=aligned, colour=torch.tensor([[4, 0.1, 1.2, 0, 1]], device=cuda),
               colour_has_contrast=False)


def test_loader_distorts_from_its_plan(cuda, shard_dir):  # noqa: F811
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.image import normalisation, preprocess

    d, images = shard_dir
    kw = dict(train=True, model="inception", device=cuda, dtype=torch.bfloat16, seed=5)
    with ImageBatches(d, 8, 35, colour="full", **kw) as b:
        for t in range(3):
            idx, boxes = b.plan(t)
            colour = b.plan_colour(t)
            x, y = b.next()
            want = preprocess(torch.from_numpy(images[idx]).to(cuda), torch.from_numpy(boxes).to(cuda), 35,
                              torch.bfloat16, *normalisation("inception"), colour=torch.from_numpy(colour).to(cuda))
            assert_equal(_bits(x), _bits(want), f"batch {t} through the staging slots")
            assert torch.equal(y.cpu(), torch.from_numpy(idx % 10))
        assert x.data_ptr() == b.x.data_ptr()  # the one persistent buffer


def test_graph_trainer_adopts_the_buffer_with_fast_colour(cuda, shard_dir):  # noqa: F811
    from tony_amd.data.images import ImageBatches

    d, _ = shard_dir
    kw = dict(train=True, model="inception", device=cuda, dtype=torch.bfloat16, seed=5, colour="fast")
    with ImageBatches(d, 8, 35, **kw) as b:
        got, tr = _losses(cuda, True, b.next)
        assert tr.static_x.data_ptr() == b.x.data_ptr()  # adopted: the replay never copies the input
    assert all(np.isfinite(v) for v in got), got
